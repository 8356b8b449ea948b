"""Host-side mirror of the reference's windowed graph-stream API, backed by libgellyhip.so.

  SimpleEdgeStream   <- streaming/SimpleEdgeStream.java:59-540 (constructors :73-94, slice :139-171,
                        distinct :305-327, reverse :332-341, undirected :354-365; the continuous operators
                        getVertices :119-125,
                        numberOfVertices :370-387, numberOfEdges :392-408, getDegrees / getInDegrees /
                        getOutDegrees :416-442)
  GraphWindowStream  <- streaming/GraphWindowStream.java:47-183 (foldNeighbors :62, reduceOnEdges :101,
                        applyOnNeighbors :130)

Same names, argument meaning and error behaviour as the Java API (camelCase kept on purpose so a
reference test reads the same here).  Windowing follows Flink 1.0.3 tumbling windows: a record with
timestamp ts belongs to [ts - ts % size, ... + size) (Java remainder), a window's results carry
timestamp end - 1.  A stream built without a time extractor behaves like the reference's
ingestion-time tests (TestSlice): every record lands in the first window.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from enum import IntEnum

import numpy as np

from . import _lib as L
from .engine import Engine, GsError, _gs_dtype, _is_torch
from .functions import (Collector, EdgesApply, EdgesFold, EdgesReduce, DegreeMaxNeighborFold, EdgeValueSeparator,
                        _BuiltinFold, _BuiltinGlobalRunning, _BuiltinReduce, _BuiltinRunning, java_equals)


class EdgeDirection(IntEnum):
    """org.apache.flink.graph.EdgeDirection (ordinals IN, OUT, ALL)."""
    IN = 0
    OUT = 1
    ALL = 2


class TimeUnit(IntEnum):
    MILLISECONDS = 1
    SECONDS = 1000
    MINUTES = 60000


@dataclass(frozen=True)
class Time:
    """org.apache.flink.streaming.api.windowing.time.Time."""
    ms: int

    @staticmethod
    def of(size: int, unit: TimeUnit = TimeUnit.MILLISECONDS) -> "Time":
        return Time(int(size) * int(unit))

    @staticmethod
    def milliseconds(n: int) -> "Time":
        return Time(int(n))

    @staticmethod
    def seconds(n: int) -> "Time":
        return Time(int(n) * 1000)

    def toMilliseconds(self) -> int:
        return self.ms


@dataclass
class EdgeColumns:
    """A DataStream<Edge<Long, EV>> laid out as columns (Tuple3 f0 = src, f1 = dst, f2 = value) plus an
    optional event-time column.  Columns are numpy (host) or torch CUDA tensors (device)."""
    src: object
    dst: object
    val: object = None
    ts: object = None

    def __len__(self):
        return len(self.src)


# ---- slice(): one engine call per window, or one for all of them (gs_slice_reduce) -----------------------
# Mean (direction-expanded) records per window below which "auto" takes the one batched call: the largest measured
# mean at which every batched repetition beat every repetition of the per-window loop on an MI355X, 2^20 records
# (I64 SUM OUT; the degree fold ALL still won at 2^21), halved because boxes differ by about 5 %
# (profiles/slice_batched/README.md).  At 2^22 records per window the loop won every repetition.
SLICE_CROSSOVER = 1 << 19
SLICE_MAX_RECORDS = (1 << 32) - 1   # direction-expanded records of one batched call (check_batch)


@dataclass(frozen=True)
class SlicePlan:
    """What plan_slice decided: batched (one gs_slice_* call) or the per-window loop, and why."""
    batched: bool
    reason: str
    windows: int = 0          # windows the timestamps span (an upper bound on the non-empty ones)


def window_span(ts_min: int, ts_max: int, size_ms: int) -> int:
    """Windows between the first and the last timestamp's, both included (window number = ts / size truncated,
    i.e. start = ts - ts % size with the Java remainder)."""
    def q(t):
        t = int(t)
        return t // size_ms if t >= 0 else -((-t) // size_ms)
    return q(ts_max) - q(ts_min) + 1


def plan_slice(mode, kind: str, op: int, val_dtype: int, has_ts: bool, records: int, windows: int,
               crossover: int = None) -> SlicePlan:
    """Route one slice().reduceOnEdges / foldNeighbors.  Pure: no GPU, no engine.

    mode: env.getSliceBatching() ("auto", True or False); kind: "reduce", "fold", "degree_max" (the built-ins) or
    "user"; op / val_dtype: the GS_OP_* / GS_* of a reduce or fold; records: direction-expanded records of the
    stream; windows: window_span of its timestamps.  The key-width limit of the batched call is not known here:
    a call it refuses (GS_EUNSUPPORTED) falls back to the loop at run time."""
    if crossover is None:
        crossover = SLICE_CROSSOVER
    if mode is False:
        return SlicePlan(False, "batching is off", windows)
    if kind not in ("reduce", "fold", "degree_max"):
        return SlicePlan(False, "user function: grouped per window", windows)
    if not has_ts:
        return SlicePlan(False, "no timestamp column: one window", windows)
    if windows <= 1:
        return SlicePlan(False, "a single window", windows)
    if records > SLICE_MAX_RECORDS:
        return SlicePlan(False, "more records than one batched call takes", windows)
    if mode is True:
        return SlicePlan(True, "batching is on", windows)
    float_sum = kind != "degree_max" and op == L.GS_OP_SUM and val_dtype in (L.GS_F32, L.GS_F64)
    if float_sum:
        return SlicePlan(False, "float SUM is not bit-stable across paths", windows)
    if records >= crossover * windows:   # mean records per window >= the crossover
        return SlicePlan(False, "windows at or above the measured crossover", windows)
    return SlicePlan(True, "windows below the measured crossover", windows)


class StreamExecutionEnvironment:
    """Holds the engine (one gs_ctx) — the role of the Flink environment for this path."""
    _default = None

    def __init__(self, device: int = 0):
        self.device = device
        self._engine = None
        self._parallelism = 1
        self._micro_batch = None
        self._slice_batching = "auto"
        self.last_slice_plan = None                                   # the last slice() operator's SlicePlan
        self.slice_counts = {"batched": 0, "loop": 0, "refused": 0}   # operators per route; refused: batched -> loop

    def setSliceBatching(self, mode="auto") -> "StreamExecutionEnvironment":
        """How slice(size).reduceOnEdges / foldNeighbors with a built-in function run a stream of many windows:
        True = all windows in one engine call (gs_slice_reduce) whenever the stream allows it, False = one call
        per window, "auto" (default) = batched where that was measured faster and the result is the loop's bit for
        bit (integers, COUNT, float MIN / MAX, the degree fold; float SUM only under True)."""
        if mode not in ("auto", True, False) or (mode != "auto" and not isinstance(mode, bool)):
            raise ValueError('slice batching is "auto", True or False')
        self._slice_batching = mode
        return self

    def getSliceBatching(self):
        return self._slice_batching

    def setParallelism(self, parallelism: int) -> "StreamExecutionEnvironment":
        """env.setParallelism: the operators' parallelism; on this path it changes what the windowed
        graph aggregation emits (one running state per partition's partial, aggregation.py)."""
        if int(parallelism) < 1:
            raise ValueError("parallelism must be at least 1")
        self._parallelism = int(parallelism)
        return self

    def getParallelism(self) -> int:
        return self._parallelism

    def setMicroBatch(self, edges: int = None) -> "StreamExecutionEnvironment":
        """Edges per engine call of the continuous operators (getDegrees, getVertices, ...): the stream goes
        through their device state in batches of this size (None = the whole stream at once).  The records
        they emit do not depend on it."""
        if edges is not None and int(edges) < 1:
            raise ValueError("a micro-batch holds at least one edge")
        self._micro_batch = None if edges is None else int(edges)
        return self

    def getMicroBatch(self):
        return self._micro_batch

    @classmethod
    def getExecutionEnvironment(cls) -> "StreamExecutionEnvironment":
        if cls._default is None:
            cls._default = cls()
        return cls._default

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            self._engine = Engine(self.device)
        return self._engine

    def fromCollection(self, edges, value_dtype=np.int64) -> EdgeColumns:
        """env.fromCollection(List<Edge<Long, EV>>): tuples (src, dst[, value[, ts]])."""
        edges = list(edges)
        src = np.array([e[0] for e in edges], dtype=np.int64)
        dst = np.array([e[1] for e in edges], dtype=np.int64)
        val = np.array([e[2] for e in edges], dtype=value_dtype) if edges and len(edges[0]) > 2 else None
        ts = np.array([e[3] for e in edges], dtype=np.int64) if edges and len(edges[0]) > 3 else None
        return EdgeColumns(src, dst, val, ts)


class AscendingTimestampExtractor:
    """Marks a stream as event-time (SimpleEdgeStream.java:90-94).  extract(cols) -> int64 timestamps."""

    def extractAscendingTimestamp(self, cols: EdgeColumns):
        raise NotImplementedError


class EdgeValueTimestampExtractor(AscendingTimestampExtractor):
    """WindowTriangles.EdgeValueTimestampExtractor (WindowTriangles.java:224-230): ts = edge value."""

    def extractAscendingTimestamp(self, cols: EdgeColumns):
        v = cols.val
        return v.cpu().numpy().astype(np.int64) if _is_torch(v) else np.asarray(v, dtype=np.int64)


@dataclass
class WindowOutput:
    start: int
    end: int
    columns: tuple            # columnar results (keys, values...) or ('records', list)

    @property
    def max_timestamp(self) -> int:
        return self.end - 1


@dataclass
class DataStream:
    """Result stream: per window, the records emitted at window end (timestamp end - 1)."""
    windows: list = field(default_factory=list)

    def collect(self) -> list:
        """All records as Python tuples, window by window (vertices ascending inside a window)."""
        out = []
        for w in self.windows:
            out.extend(_rows(w.columns))
        return out

    def collectWithTimestamps(self) -> list:
        out = []
        for w in self.windows:
            out.extend((r, w.max_timestamp) for r in _rows(w.columns))
        return out


def _to_np(x):
    if x is None:
        return None
    return x.cpu().numpy() if _is_torch(x) else np.asarray(x)


def _rows(cols):
    if cols and isinstance(cols[0], str) and cols[0] == "records":
        return list(cols[1])
    arrs = [_to_np(c) for c in cols]
    return [tuple(v.item() for v in row) for row in zip(*arrs)]


def _take(x, idx):
    if x is None:
        return None
    if _is_torch(x):
        import torch

        return x.index_select(0, torch.as_tensor(idx, device=x.device))
    return np.asarray(x)[idx]


class SimpleEdgeStream:
    """streaming/SimpleEdgeStream.java — the windowed-neighbourhood part of it and the continuous degree /
    vertex streams."""

    def __init__(self, edges: EdgeColumns, context: StreamExecutionEnvironment = None,
                 timeExtractor: AscendingTimestampExtractor = None):
        self.context = context or StreamExecutionEnvironment.getExecutionEnvironment()
        self.edges = edges
        if timeExtractor is not None:   # :90-94 event time
            self.edges = EdgeColumns(edges.src, edges.dst, edges.val,
                                     np.asarray(timeExtractor.extractAscendingTimestamp(edges), dtype=np.int64))

    def getEdges(self) -> EdgeColumns:
        return self.edges

    def getContext(self) -> StreamExecutionEnvironment:
        return self.context

    def mapEdges(self, mapper) -> "SimpleEdgeStream":
        """mapEdges (SimpleEdgeStream.java:221-226) for the value-dropping mapper of WindowTriangles
        (RemoveEdgeValue -> NullValue): mapper(values) returns the new value column or None."""
        e = self.edges
        return SimpleEdgeStream(EdgeColumns(e.src, e.dst, mapper(e.val), e.ts), self.context)

    def reverse(self) -> "SimpleEdgeStream":
        """:332-341 Edge.reverse() = (f1, f0, f2)."""
        e = self.edges
        return SimpleEdgeStream(EdgeColumns(e.dst, e.src, e.val, e.ts), self.context)

    def undirected(self) -> "SimpleEdgeStream":
        """:354-365 emits e then e.reverse() for every edge."""
        e = self.edges
        n = len(e)
        if _is_torch(e.src):
            import torch

            src = torch.stack([e.src, e.dst], 1).reshape(-1)
            dst = torch.stack([e.dst, e.src], 1).reshape(-1)
            val = None if e.val is None else torch.repeat_interleave(e.val, 2)
        else:
            src = np.empty(2 * n, np.int64); src[0::2] = e.src; src[1::2] = e.dst
            dst = np.empty(2 * n, np.int64); dst[0::2] = e.dst; dst[1::2] = e.src
            val = None if e.val is None else np.repeat(np.asarray(e.val), 2)
        ts = None if e.ts is None else np.repeat(np.asarray(e.ts), 2)
        return SimpleEdgeStream(EdgeColumns(src, dst, val, ts), self.context)

    def aggregate(self, graphAggregation, vertexMapper=None) -> "DataStream":
        """One argument: GraphStream.aggregate (SimpleEdgeStream.java:104-106), e.g.
        ConnectedComponents(mergeWindowTime).

        Two arguments, aggregate(edgeMapper, vertexMapper) (:493-498: flatMap -> keyBy(0) -> map): a running value
        per vertex, one record (vertex, value) per record the edge mapper emits, in arrival order.  An
        EdgeValueSeparator with RunningSum / RunningMin / RunningMax / RunningCount runs on the device through one
        fresh state in env.getMicroBatch()-sized batches (the result does not depend on that size); any other
        pair is user code, called record by record on the host: edgeMapper.flatMap(edge, out) (or
        edgeMapper(edge, out)) with edge = (source, target, value) and out a Collector, then vertexMapper.map(record)
        (or vertexMapper(record)) on each collected record."""
        if vertexMapper is None:
            return graphAggregation.run(self)
        edgeMapper = graphAggregation
        if isinstance(edgeMapper, EdgeValueSeparator) and isinstance(vertexMapper, _BuiltinRunning):
            return self._device_aggregate(edgeMapper, vertexMapper, "keyed", False)
        vmap = getattr(vertexMapper, "map", vertexMapper)
        return DataStream([WindowOutput(0, 0, ("records", [vmap(r) for r in self._host_records(edgeMapper)]))])

    def globalAggregate(self, edgeMapper, vertexMapper, collectUpdates: bool) -> "DataStream":
        """:509-539 -> the same at parallelism 1 with one value for the whole stream (bare values); with
        collectUpdates only the values that differ (Java equals) from the one before them.  An EdgeValueSeparator
        with GlobalRunningSum / Min / Max / Count runs on the device; any other pair on the host:
        vertexMapper.flatMap(record, out) (or vertexMapper(record, out)) collects the values."""
        if isinstance(edgeMapper, EdgeValueSeparator) and isinstance(vertexMapper, _BuiltinGlobalRunning):
            return self._device_aggregate(edgeMapper, vertexMapper, "global", collectUpdates)
        vflat = getattr(vertexMapper, "flatMap", vertexMapper)
        out = Collector()
        for r in self._host_records(edgeMapper):
            vflat(r, out)
        values = out.records
        if collectUpdates:   # GlobalAggregateMapper :525-539
            kept, prev = [], None
            for v in values:
                if not java_equals(v, prev):
                    prev = v
                    kept.append(v)
            values = kept
        return DataStream([WindowOutput(0, 0, ("records", values))])

    def _host_records(self, edgeMapper):
        """The records a user edge mapper collects, edge by edge in arrival order."""
        e = self.edges
        eflat = getattr(edgeMapper, "flatMap", edgeMapper)
        src, dst, val = _to_np(e.src), _to_np(e.dst), _to_np(e.val)
        out = Collector()
        for i in range(len(src)):
            eflat((src[i].item(), dst[i].item(), None if val is None else val[i].item()), out)
        return out.records

    def _device_aggregate(self, edgeMapper, vertexMapper, mode: str, collect_updates: bool) -> "DataStream":
        e = self.edges
        n = len(e)
        count = vertexMapper.op == L.GS_OP_COUNT
        if e.val is None and not count:
            raise ValueError("aggregate: the stream has no edge values")
        mb = self.context.getMicroBatch() or max(n, 1)
        out = DataStream()
        with self.context.engine.aggregate_state(vertexMapper.op, _gs_dtype(e.val), mode) as state:
            for a in range(0, n, mb):
                src, dst, val = e.src[a:a + mb], e.dst[a:a + mb], None if e.val is None else e.val[a:a + mb]
                if mode == "keyed":
                    cols = state.edges(src, dst, val, edgeMapper.direction)
                else:
                    vals = state.global_(src, dst, val, edgeMapper.direction, collect_updates)[1]
                    cols = ("records", [x.item() for x in _to_np(vals)])
                out.windows.append(WindowOutput(0, 0, cols))
        return out

    # -- the continuous operators: one device state per call, fed in micro-batches (env.setMicroBatch) ----
    # Records come out in the reference's order at parallelism 1 whatever env.getParallelism() says (at
    # parallelism P the reference emits the same multiset: keyBy keeps each vertex's records in order).
    def _micro_batches(self):
        e = self.edges
        n = len(e)
        mb = self.context.getMicroBatch() or max(n, 1)
        for a in range(0, n, mb):
            yield e.src[a:a + mb], e.dst[a:a + mb]

    def _degree_stream(self, direction: EdgeDirection) -> "DataStream":
        out = DataStream()
        with self.context.engine.continuous() as state:
            for src, dst in self._micro_batches():
                out.windows.append(WindowOutput(0, 0, state.degrees(src, dst, direction)))
        return out

    def getDegrees(self) -> "DataStream":
        """:416-420 -> Vertex<K, Long>(vertex, degree so far) per endpoint of every edge, source first."""
        return self._degree_stream(EdgeDirection.ALL)

    def getInDegrees(self) -> "DataStream":
        """:428-431 -> (target, in-degree so far) per edge."""
        return self._degree_stream(EdgeDirection.IN)

    def getOutDegrees(self) -> "DataStream":
        """:439-442 -> (source, out-degree so far) per edge."""
        return self._degree_stream(EdgeDirection.OUT)

    def _vertex_stream(self, column: int) -> "DataStream":
        out = DataStream()
        with self.context.engine.continuous() as state:
            for src, dst in self._micro_batches():
                cols = state.vertices(src, dst)
                out.windows.append(WindowOutput(0, 0, (cols[0],) if column == 0 else
                                                ("records", [int(x) for x in _to_np(cols[1])])))
        return out

    def getVertices(self) -> "DataStream":
        """:119-125 -> Vertex<K, NullValue>: each vertex once, at its first appearance; records (vertex,)."""
        return self._vertex_stream(0)

    def numberOfVertices(self) -> "DataStream":
        """:370-387 -> the number of distinct vertices so far, emitted whenever it changes (bare longs)."""
        return self._vertex_stream(1)

    def numberOfEdges(self) -> "DataStream":
        """:392-408 -> the number of edges so far, duplicates included, one per edge (bare longs): the state's
        record counter running over the stream, no kernel."""
        out, seen = DataStream(), 0
        for src, _ in self._micro_batches():
            out.windows.append(WindowOutput(0, 0, ("records", list(range(seen + 1, seen + len(src) + 1)))))
            seen += len(src)
        return out

    def distinct(self, per_vertex: bool = True) -> "SimpleEdgeStream":
        """:305-327 -> the stream without its repeated edges: each edge at its first arrival, unchanged (value
        and timestamp), in arrival order.  The stream goes through one fresh device state in
        env.getMicroBatch()-sized batches; the result does not depend on that size.

        per_vertex=True: an edge is a repeat iff its (source, target) pair came before -- the Javadoc's "a
        neighborhood set for each vertex" and the reading TestDistinct pins.  per_vertex=False: iff its target
        came before, whatever its source -- the literal DistinctEdgeMapper, which keeps ONE set of targets per
        operator instance, at parallelism 1.

        env.getParallelism() does not change the result.  Per vertex it cannot: keyBy(0) sends all edges of a
        source to one subtask.  The literal mapper at parallelism P depends on which sources share a subtask,
        i.e. on Flink's key -> subtask hash, which is not part of this package: a caller who wants that holds
        P states (Engine.distinct("instance")) and routes by source."""
        e = self.edges
        n = len(e)
        mb = self.context.getMicroBatch() or max(n, 1)
        src, dst, val, idx = [], [], [], []
        with self.context.engine.distinct("keyed" if per_vertex else "instance") as state:
            for a in range(0, n, mb):
                s, d, v, i = state.edges(e.src[a:a + mb], e.dst[a:a + mb], None if e.val is None else e.val[a:a + mb])
                src.append(s); dst.append(d); val.append(v); idx.append(_to_np(i).astype(np.int64) + a)
        if _is_torch(e.src):
            import torch

            cat = torch.cat
        else:
            cat = np.concatenate
        if not src:
            return SimpleEdgeStream(EdgeColumns(e.src[:0], e.dst[:0], None if e.val is None else e.val[:0],
                                                None if e.ts is None else e.ts[:0]), self.context)
        ts = None if e.ts is None else np.asarray(e.ts)[np.concatenate(idx)]
        return SimpleEdgeStream(EdgeColumns(cat(src), cat(dst), None if e.val is None else cat(val), ts), self.context)

    def slice(self, size: Time, direction: EdgeDirection = EdgeDirection.OUT) -> "GraphWindowStream":
        """:139-171 tumbling windows keyed by the neighbour-key vertex."""
        if not isinstance(direction, EdgeDirection) and direction not in (0, 1, 2):
            raise ValueError("Illegal edge direction")   # IllegalArgumentException :168-169
        return GraphWindowStream(self, size.toMilliseconds(), EdgeDirection(direction))

    # tumbling windows of this stream: [(start, end, columns of that window in arrival order)]
    def _windows(self, size_ms: int, with_index: bool = False):
        """with_index: each window also carries its records' positions in the stream (arrival order)."""
        e = self.edges
        if e.ts is None:
            return [(0, size_ms, e, np.arange(len(e)))] if with_index else [(0, size_ms, e)]
        ts = np.asarray(_to_np(e.ts), dtype=np.int64)
        start = ts - np.fmod(ts, size_ms)
        order = np.argsort(start, kind="stable")
        starts, first = np.unique(start[order], return_index=True)
        bounds = list(first) + [len(order)]
        out = []
        for i, s in enumerate(starts):
            idx = order[bounds[i]:bounds[i + 1]]
            contiguous = len(idx) == 0 or (idx[-1] - idx[0] + 1 == len(idx) and np.all(np.diff(idx) == 1))
            if contiguous and len(idx):
                sl = slice(int(idx[0]), int(idx[-1]) + 1)
                cols = EdgeColumns(e.src[sl], e.dst[sl], None if e.val is None else e.val[sl], ts[sl])
            else:
                cols = EdgeColumns(_take(e.src, idx), _take(e.dst, idx), _take(e.val, idx), ts[idx])
            out.append((int(s), int(s) + size_ms, cols, idx) if with_index else (int(s), int(s) + size_ms, cols))
        return out


class GraphWindowStream:
    """streaming/GraphWindowStream.java:47-183."""

    def __init__(self, stream: SimpleEdgeStream, size_ms: int, direction: EdgeDirection):
        self.stream = stream
        self.size_ms = size_ms
        self.direction = direction

    @property
    def engine(self) -> Engine:
        return self.stream.context.engine

    def _each(self):
        return self.stream._windows(self.size_ms)

    # -- routing: the per-window loop below, or every window in one call ------------------------------------
    def _plan(self, kind: str, op: int) -> SlicePlan:
        e, env = self.stream.edges, self.stream.context
        n = len(e)
        windows = 1
        if e.ts is not None and n:
            windows = window_span(e.ts.min().item() if _is_torch(e.ts) else np.min(e.ts),
                                  e.ts.max().item() if _is_torch(e.ts) else np.max(e.ts), self.size_ms)
        dtype = L.GS_NONE if kind == "degree_max" or op == L.GS_OP_COUNT else _gs_dtype(e.val)
        plan = plan_slice(env.getSliceBatching(), kind, op, dtype, e.ts is not None and n > 0,
                          Engine._records(n, self.direction), windows)
        env.last_slice_plan = plan
        return plan

    def _batched(self, plan: SlicePlan, call) -> DataStream:
        """call(windows_hint) -> (window_start, row_begin, *row columns); None when the engine refuses the key."""
        env = self.stream.context
        try:
            ws, rb, *cols = call(plan.windows)
        except GsError as err:
            if err.status != L.GS_EUNSUPPORTED:
                raise
            env.slice_counts["refused"] += 1
            return None
        env.slice_counts["batched"] += 1
        ws, rb = _to_np(ws), _to_np(rb)
        out = DataStream()
        for w in range(len(ws)):
            lo, hi = int(rb[w]), int(rb[w + 1])
            out.windows.append(WindowOutput(int(ws[w]), int(ws[w]) + self.size_ms, tuple(c[lo:hi] for c in cols)))
        return out

    def reduceOnEdges(self, reduceFunction: EdgesReduce) -> DataStream:
        """:101-104 -> Tuple2<K, EV>(vertex, reduced value) per vertex and window."""
        builtin = isinstance(reduceFunction, _BuiltinReduce)
        plan = self._plan("reduce" if builtin else "user", reduceFunction.op if builtin else -1)
        if plan.batched:
            e = self.stream.edges
            if reduceFunction.op != L.GS_OP_COUNT and e.val is None:
                raise ValueError("reduceOnEdges needs edge values")
            out = self._batched(plan, lambda hint: self.engine.slice_reduce(
                e.src, e.dst, e.val, e.ts, self.size_ms, self.direction, reduceFunction.op, windows_hint=hint))
            if out is not None:
                return out
        self.stream.context.slice_counts["loop"] += 1
        out = DataStream()
        for s, t, w in self._each():
            if len(w) == 0:
                continue
            if isinstance(reduceFunction, _BuiltinReduce):
                if reduceFunction.op != L.GS_OP_COUNT and w.val is None:
                    raise ValueError("reduceOnEdges needs edge values")
                k, v = self.engine.reduce(w.src, w.dst, w.val, self.direction, reduceFunction.op)
                out.windows.append(WindowOutput(s, t, (k, v)))
            else:
                recs = []
                for key, nbrs, vals in self._groups(w):
                    acc = vals[0]
                    for x in vals[1:]:
                        acc = reduceFunction.reduceEdges(acc, x)   # EdgesReduceFunction.reduce :116-120
                    recs.append((key, acc))
                out.windows.append(WindowOutput(s, t, ("records", recs)))
        return out

    def foldNeighbors(self, initialValue, foldFunction: EdgesFold) -> DataStream:
        """:62-64 -> one accumulator per vertex and window, folded from a copy of initialValue."""
        degmax = isinstance(foldFunction, DegreeMaxNeighborFold)
        builtin = isinstance(foldFunction, _BuiltinFold)
        plan = self._plan("degree_max" if degmax else "fold" if builtin else "user", foldFunction.op if builtin else -1)
        if plan.batched:
            e = self.stream.edges
            if degmax:
                init_max = int(initialValue[2]) if len(initialValue) > 2 else -(1 << 63)

                def call(hint):
                    ws, rb, k, d, m = self.engine.slice_fold_degree_max(e.src, e.dst, e.ts, self.size_ms, self.direction,
                                                                        init_max, windows_hint=hint)
                    if int(initialValue[1]) != 0:
                        d = d + int(initialValue[1])
                    return ws, rb, k, d, m
            else:
                if foldFunction.op != L.GS_OP_COUNT and e.val is None:
                    raise ValueError("foldNeighbors needs edge values")

                def call(hint):
                    return self.engine.slice_reduce(e.src, e.dst, e.val, e.ts, self.size_ms, self.direction,
                                                    foldFunction.op, initialValue[1], windows_hint=hint)
            out = self._batched(plan, call)
            if out is not None:
                return out
        self.stream.context.slice_counts["loop"] += 1
        out = DataStream()
        for s, t, w in self._each():
            if len(w) == 0:
                continue
            if isinstance(foldFunction, DegreeMaxNeighborFold):
                init_max = int(initialValue[2]) if len(initialValue) > 2 else -(1 << 63)
                k, d, m = self.engine.fold_degree_max(w.src, w.dst, self.direction, init_max)
                if int(initialValue[1]) != 0:
                    d = d + int(initialValue[1])
                out.windows.append(WindowOutput(s, t, (k, d, m)))
            elif isinstance(foldFunction, _BuiltinFold):
                if foldFunction.op != L.GS_OP_COUNT and w.val is None:
                    raise ValueError("foldNeighbors needs edge values")
                k, v = self.engine.fold(w.src, w.dst, w.val, self.direction, foldFunction.op, initialValue[1])
                out.windows.append(WindowOutput(s, t, (k, v)))
            else:
                recs = []
                for key, nbrs, vals in self._groups(w):
                    acc = copy.deepcopy(initialValue)
                    for nb, x in zip(nbrs, vals if vals is not None else [None] * len(nbrs)):
                        acc = foldFunction.foldEdges(acc, key, nb, x)   # EdgesFoldFunction.fold :78-80
                    recs.append(acc)
                out.windows.append(WindowOutput(s, t, ("records", recs)))
        return out

    def applyOnNeighbors(self, applyFunction: EdgesApply) -> DataStream:
        """:130-131 -> 0..n records per vertex from its (neighbour, value) list in arrival order."""
        from .triangles import GenerateCandidateEdges

        out = DataStream()
        for s, t, w in self._each():
            if len(w) == 0:
                continue
            if isinstance(applyFunction, GenerateCandidateEdges) and self.direction == EdgeDirection.ALL:
                a, b, f = self.engine.candidates(w.src, w.dst)
                out.windows.append(WindowOutput(s, t, (a, b, f)))
                continue
            col = Collector()
            for key, nbrs, vals in self._groups(w):
                vv = vals if vals is not None else [None] * len(nbrs)
                applyFunction.applyOnEdges(key, [(nb, x) for nb, x in zip(nbrs, vv)], col)   # :144-175
            out.windows.append(WindowOutput(s, t, ("records", col.records)))
        return out

    # GPU grouping for host-side user functions: (key, neighbours, values) in arrival order
    def _groups(self, w: EdgeColumns):
        keys, offs, nbrs, vals = self.engine.csr(w.src, w.dst, w.val, self.direction)
        keys, offs, nbrs = _to_np(keys), _to_np(offs), _to_np(nbrs)
        vals = _to_np(vals)
        for u in range(len(keys)):
            lo, hi = int(offs[u]), int(offs[u + 1])
            yield (int(keys[u]), [int(x) for x in nbrs[lo:hi]],
                   None if vals is None else [x.item() for x in vals[lo:hi]])
