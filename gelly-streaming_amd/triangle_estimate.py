"""The streaming triangle-count estimators (example/BroadcastTriangleCount.java,
example/IncidenceSamplingTriangleCount.java) on the engine.

The reference pipelines are
    edges.broadcast().flatMap(TriangleSampler(samples / p, vertexCount))
         .flatMap(TriangleSummer(samples, vertexCount)).setParallelism(1)        (Broadcast :38-45)
    edges.flatMap(EdgeSampleMapper).keyBy(0).flatMap(TriangleSampleMapper(samples / p, vertexCount))
         .flatMap(TriangleSummer(samples, vertexCount)).setParallelism(1)        (Incidence :36-44)
Here the samplers of one subtask are a device-resident state (Engine.triangle_sampler, gs_trisample.hip) that
emits that subtask's TriangleEstimate records; TriangleSummer stays on the host, line for line.

The reference draws its third vertices (and Broadcast's coins) from Math.random(), so no two of its runs
agree; this path's random numbers are counter-based and its own (include/gelly_hip.h), fixed by `seed`.
"""
from __future__ import annotations

import numpy as np

from .stream import DataStream, SimpleEdgeStream, WindowOutput

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def _int32(x: int) -> int:
    """Java int arithmetic: wrap to 32 bits."""
    return ((int(x) - INT_MIN) & 0xFFFFFFFF) + INT_MIN


def java_int_cast(x: float) -> int:
    """(int) of a double as Java casts (JLS 5.1.3): NaN -> 0, saturating at the int range, else toward zero."""
    if x != x:
        return 0
    if x >= INT_MAX:
        return INT_MAX
    if x <= INT_MIN:
        return INT_MIN
    return int(x)


class TriangleSummer:
    """BroadcastTriangleCount.java:138-174 (IncidenceSamplingTriangleCount.java:205-242 is the same class)."""

    def __init__(self, sample_size: int, vertices: int):
        self.results = {}            # :140 source -> its last (edgeCount, beta)
        self.maxEdges = 0
        self.sampleSize = int(sample_size)
        self.previousResult = 0
        self.vertices = int(vertices)

    def flatMap(self, source: int, edge_count: int, beta: int, out: list):
        """:155-173 -- one TriangleEstimate(source, edgeCount, beta); appends (maxEdges, result) to out when
        the result changes."""
        self.results[int(source)] = (int(edge_count), int(beta))   # :156
        if edge_count > self.maxEdges:                              # :158-160
            self.maxEdges = int(edge_count)
        globalBetaSum = 0                                           # :162-165
        for _, b in self.results.values():
            globalBetaSum = _int32(globalBetaSum + b)
        # :167 -- evaluated left to right in double: ((1.0 / S) * sum) * maxEdges) * (vertices - 2)
        result = java_int_cast((1.0 / float(self.sampleSize)) * float(globalBetaSum) * float(self.maxEdges)
                               * float(_int32(self.vertices - 2)))
        if result != self.previousResult:                           # :168-171
            self.previousResult = result
            out.append((self.maxEdges, result))

    def feed(self, source: int, edge_counts, betas) -> list:
        """The estimates of one source, in order, through flatMap; returns the records they emit."""
        out = []
        for k, b in zip(_host(edge_counts), _host(betas)):
            self.flatMap(source, int(k), int(b), out)
        return out


def _host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


def merge_estimates(parts) -> list:
    """The estimates of several subtasks over the same stretch of the stream -> one sequence for the summer.
    parts: [(source, edge_counts, betas)].  Flink interleaves the subtasks' records as they arrive, which no
    run pins; this path merges by (edge count, source), each source's records in their own order."""
    rows = []
    for source, ks, bs in parts:
        rows.extend((int(k), int(source), i, int(b)) for i, (k, b) in enumerate(zip(_host(ks), _host(bs))))
    rows.sort()
    return [(source, k, b) for k, source, _, b in rows]


def _count(edges: SimpleEdgeStream, mode: str, vertex_count: int, samples: int, seed: int) -> DataStream:
    env = edges.getContext()
    p = env.getParallelism()
    local = int(samples) // p            # :38 int localSamples = samples / env.getParallelism()
    eng = env.engine
    states = [eng.triangle_sampler(mode, local, vertex_count, seed, first_sampler=q * local) for q in range(p)]
    summer = TriangleSummer(samples, vertex_count)
    out = DataStream()
    try:
        for src, dst in edges._micro_batches():
            parts = [(q,) + tuple(st.edges(src, dst)) for q, st in enumerate(states)]
            records = []
            for source, k, b in merge_estimates(parts):
                summer.flatMap(source, k, b, records)
            out.windows.append(WindowOutput(0, 0, ("records", records)))
    finally:
        for st in states:
            st.close()
    return out


def broadcast_triangle_count(edges: SimpleEdgeStream, vertex_count: int, samples: int, seed: int = 0) -> DataStream:
    """BroadcastTriangleCount.main (:31-55): the (edges so far, estimated triangles) records of the stream,
    emitted whenever the estimate changes.  The stream goes through env.getParallelism() device states of
    samples / parallelism samplers each, in env.getMicroBatch()-sized batches; the result does not depend
    on that size."""
    return _count(edges, "broadcast", vertex_count, samples, seed)


def incidence_sampling_triangle_count(edges: SimpleEdgeStream, vertex_count: int, samples: int, seed: int = 0) -> DataStream:
    """IncidenceSamplingTriangleCount.main (:31-54): as broadcast_triangle_count, but a subtask reports its
    beta sum only when one of its samplers finds its triangle (TriangleSampleMapper :188-201), so several
    records may carry one edge count and a drop shows with the next find."""
    return _count(edges, "incidence", vertex_count, samples, seed)
