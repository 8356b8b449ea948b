"""example/IterativeConnectedComponents.java on the engine.

The reference pipeline is
    edges.iterate() -> keyBy(0).flatMap(new AssignComponents()) -> closeWith(...)                (:56-58)
one mapper per subtask that keeps the partition of the vertices seen so far and emits a (vertex, componentId)
record per vertex whose component id changes; its own output returns to it over the feedback edge.

What is built (include/gelly_hip.h "AssignComponents"): the mapper as its comments describe it,
at parallelism 1.  The literal addToExistingComponent (:136-139) emits a vertex that joins a component with a
smaller id without adding it to the set, so that vertex's own record, fed back, is emitted again for ever; read
as "add the target to the source's component", a fed-back record has both ends in one component and is a no-op
wherever it is interleaved, and the output is a function of the edge stream alone.  Inside one edge's emission
the records come ascending by vertex (the reference: HashSet iteration order).  At parallelism P the reference's
subtasks exchange state through the feedback edge and the result depends on its timing: that is not built, and
IterativeConnectedComponents.run raises there.
"""
from __future__ import annotations

import numpy as np

from .stream import DataStream, EdgeColumns, StreamExecutionEnvironment, WindowOutput


def _host(x):
    return x.cpu().numpy() if hasattr(x, "is_cuda") else np.asarray(x)


class AssignComponents:
    """The mapper (:67-168) over a device-resident partition (Engine.assign_components): flatMap takes a batch of
    edges where the reference's takes one, and returns their (vertex, componentId) records in stream order."""

    def __init__(self, env: StreamExecutionEnvironment):
        self.state = env.engine.assign_components()

    def flatMap(self, src, dst) -> list:
        v, c, _ = self.state.edges(src, dst)
        return list(zip(_host(v).tolist(), _host(c).tolist()))

    def close(self):
        self.state.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class IterativeConnectedComponents:
    """IterativeConnectedComponents.run (:44-64) without its text input (split("\\\\t") stays on the host: pass the
    parsed edges)."""

    def __init__(self, env: StreamExecutionEnvironment = None):
        self.env = env or StreamExecutionEnvironment.getExecutionEnvironment()

    @staticmethod
    def getEdgesDataSet() -> list:
        """the built-in data (:212-221): generateSequence(1, 10).flatMap(key -> (key, key + 1), (key, key + 2))"""
        return [(key, key + i) for key in range(1, 11) for i in range(1, 3)]

    def run(self, edges=None) -> DataStream:
        """The (vertex, component) records of the edge stream -- (src, dst) tuples, EdgeColumns or None for the
        built-in data -- fed through one fresh state in env.getMicroBatch()-sized batches; the records do not
        depend on that size."""
        if self.env.getParallelism() != 1:
            raise ValueError("IterativeConnectedComponents runs at parallelism 1: at parallelism P the reference's "
                             "AssignComponents subtasks exchange their state through the feedback edge, and its "
                             "timing decides the output (DESIGN.md §7)")
        if edges is None:
            edges = self.getEdgesDataSet()
        if isinstance(edges, EdgeColumns):
            src, dst = edges.src, edges.dst
        else:
            edges = list(edges)
            src = np.array([e[0] for e in edges], dtype=np.int64)
            dst = np.array([e[1] for e in edges], dtype=np.int64)
        n = len(src)
        mb = self.env.getMicroBatch() or max(n, 1)
        out = DataStream()
        with AssignComponents(self.env) as mapper:
            for a in range(0, n, mb):
                out.windows.append(WindowOutput(0, 0, ("records", mapper.flatMap(src[a:a + mb], dst[a:a + mb]))))
        return out
