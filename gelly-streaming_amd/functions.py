"""The reference's user-function interfaces and the built-ins the engine runs on the GPU.

  EdgesReduce  <- streaming/EdgesReduce.java:31-44   reduceEdges(firstEdgeValue, secondEdgeValue)
  EdgesFold    <- streaming/EdgesFold.java:33-48     foldEdges(accum, vertexID, neighborID, edgeValue)
  EdgesApply   <- streaming/EdgesApply.java:35-48    applyOnEdges(vertexID, neighbors, out)

Dispatch rule: an instance of a *built-in* class below is executed by
libgellyhip.so (sort + segmented reduce on the GPU).  Any other subclass is user code: the GPU still
groups the window (gs_window_csr, arrival order kept) and the user function is then called per
vertex on the host exactly as Flink's window function would call it.

The same rule holds for SimpleEdgeStream.aggregate(edgeMapper, vertexMapper) and globalAggregate: an
EdgeValueSeparator with one of the Running* / GlobalRunning* mappers below runs on the device (gs_agg_edges /
gs_agg_global); any other pair is user code and runs record by record on the host, in arrival order.
"""
from __future__ import annotations

from . import _lib as L


class EdgesReduce:
    """Interface: combine two edge values of one vertex into one (GraphWindowStream.java:101-121)."""

    def reduceEdges(self, firstEdgeValue, secondEdgeValue):
        raise NotImplementedError


class EdgesFold:
    """Interface: fold one neighbour edge into the accumulator (GraphWindowStream.java:62-87)."""

    def foldEdges(self, accum, vertexID, neighborID, edgeValue):
        raise NotImplementedError


class EdgesApply:
    """Interface: compute 0..n outputs from a vertex neighbourhood (GraphWindowStream.java:130-175)."""

    def applyOnEdges(self, vertexID, neighbors, out):
        raise NotImplementedError


class Collector:
    """org.apache.flink.util.Collector: out.collect(record)."""

    def __init__(self):
        self.records = []

    def collect(self, record):
        self.records.append(tuple(record) if isinstance(record, (list, tuple)) else record)


# ---- built-in reducers (GPU) ----------------------------------------------------------------------
class _BuiltinReduce(EdgesReduce):
    op: int = -1


class SumReduce(_BuiltinReduce):
    """reduceEdges(a, b) = a + b  (Integer/Long wrap, Float/Double IEEE) — TestSlice.java:242-249."""
    op = L.GS_OP_SUM

    def reduceEdges(self, a, b):
        return a + b


class MinReduce(_BuiltinReduce):
    """reduceEdges(a, b) = Math.min(a, b)."""
    op = L.GS_OP_MIN

    def reduceEdges(self, a, b):
        return min(a, b)


class MaxReduce(_BuiltinReduce):
    """reduceEdges(a, b) = Math.max(a, b)."""
    op = L.GS_OP_MAX

    def reduceEdges(self, a, b):
        return max(a, b)


class CountReduce(_BuiltinReduce):
    """Number of edge records of the vertex in the window (Long)."""
    op = L.GS_OP_COUNT


# ---- built-in folds (GPU) -------------------------------------------------------------------------
class _BuiltinFold(EdgesFold):
    op: int = -1


class SumValuesFold(_BuiltinFold):
    """acc.f0 = vertexID; acc.f1 += edgeValue, from init (k, v0) -> (vertex, v0 + sum).  TestSlice.java:233-240."""
    op = L.GS_OP_SUM

    def foldEdges(self, accum, vertexID, neighborID, edgeValue):
        return (vertexID, accum[1] + edgeValue)


class MinValuesFold(_BuiltinFold):
    op = L.GS_OP_MIN

    def foldEdges(self, accum, vertexID, neighborID, edgeValue):
        return (vertexID, min(accum[1], edgeValue))


class MaxValuesFold(_BuiltinFold):
    op = L.GS_OP_MAX

    def foldEdges(self, accum, vertexID, neighborID, edgeValue):
        return (vertexID, max(accum[1], edgeValue))


class CountFold(_BuiltinFold):
    """acc = (vertex, acc.f1 + 1)."""
    op = L.GS_OP_COUNT

    def foldEdges(self, accum, vertexID, neighborID, edgeValue):
        return (vertexID, accum[1] + 1)


class DegreeMaxNeighborFold(_BuiltinFold):
    """acc = (vertex, degree + 1, max(maxNeighbor, neighborID)) from init (k, 0, m0) (BASELINE config C3)."""
    op = -2

    def foldEdges(self, accum, vertexID, neighborID, edgeValue):
        return (vertexID, accum[1] + 1, max(accum[2], neighborID))


# ---- aggregate / globalAggregate (SimpleEdgeStream.java:493-539) ------------------------------------------
class EdgeValueSeparator:
    """The built-in edge mapper: DegreeTypeSeparator (SimpleEdgeStream.java:444-463) carrying the edge's value where
    that class puts 1L -- (source, value) if collectOut, then (target, value) if collectIn."""

    def __init__(self, collectIn: bool, collectOut: bool):
        if not (collectIn or collectOut):
            raise ValueError("EdgeValueSeparator: collectIn or collectOut")
        self.collectIn, self.collectOut = bool(collectIn), bool(collectOut)

    @property
    def direction(self) -> int:
        """The EdgeDirection value the engine takes: IN 0, OUT 1, ALL 2."""
        return 2 if self.collectIn and self.collectOut else (0 if self.collectIn else 1)

    def flatMap(self, edge, out):
        if self.collectOut:
            out.collect((edge[0], edge[2]))
        if self.collectIn:
            out.collect((edge[1], edge[2]))


def java_combine(op: int, a, b):
    """a (+) b for numpy scalars of one dtype as gs_window_reduce combines: integer SUM wraps at its width,
    MIN / MAX are Math.min / Math.max (NaN wins, -0.0 < +0.0)."""
    import numpy as np

    if op == L.GS_OP_SUM:
        with np.errstate(over="ignore", invalid="ignore"):
            return a + b
    if np.issubdtype(type(a), np.floating):
        if a != a:
            return a
        if b != b:
            return b
        if a == 0 and b == 0:
            neg = np.signbit(a) or np.signbit(b) if op == L.GS_OP_MIN else np.signbit(a) and np.signbit(b)
            return type(a)(-0.0 if neg else 0.0)
    return (a if a <= b else b) if op == L.GS_OP_MIN else (a if a >= b else b)


class _BuiltinRunning:
    """A vertex mapper the device runs: map((vertex, value)) -> (vertex, accumulator so far), a HashMap<K, VV>
    combined with `op`; a vertex's first value is its accumulator unchanged."""
    op: int = -1

    def __init__(self):
        self.acc = {}

    def map(self, record):
        k, v = record
        v = 1 if self.op == L.GS_OP_COUNT else v
        self.acc[k] = v if k not in self.acc else java_combine(L.GS_OP_SUM if self.op == L.GS_OP_COUNT else self.op,
                                                               self.acc[k], v)
        return (k, self.acc[k])


class RunningSum(_BuiltinRunning):
    """The sum of the vertex's values so far (the weighted degree)."""
    op = L.GS_OP_SUM


class RunningMin(_BuiltinRunning):
    op = L.GS_OP_MIN


class RunningMax(_BuiltinRunning):
    op = L.GS_OP_MAX


class RunningCount(_BuiltinRunning):
    """The number of the vertex's records so far (Long): DegreeMapFunction (SimpleEdgeStream.java:465-482)."""
    op = L.GS_OP_COUNT


class _BuiltinGlobalRunning:
    """A globalAggregate vertex mapper the device runs: flatMap((vertex, value), out) collects the combine of
    every record value of the stream so far."""
    op: int = -1
    _none = object()

    def __init__(self):
        self.acc = self._none

    def flatMap(self, record, out):
        v = 1 if self.op == L.GS_OP_COUNT else record[1]
        self.acc = v if self.acc is self._none else java_combine(
            L.GS_OP_SUM if self.op == L.GS_OP_COUNT else self.op, self.acc, v)
        out.collect(self.acc)


class GlobalRunningSum(_BuiltinGlobalRunning):
    op = L.GS_OP_SUM


class GlobalRunningMin(_BuiltinGlobalRunning):
    op = L.GS_OP_MIN


class GlobalRunningMax(_BuiltinGlobalRunning):
    op = L.GS_OP_MAX


class GlobalRunningCount(_BuiltinGlobalRunning):
    """The number of records so far (Long)."""
    op = L.GS_OP_COUNT


def java_equals(a, b) -> bool:
    """Long.equals / Double.equals on numpy or Python scalars: floats compare by their bits with every NaN as
    one, so 0.0 and -0.0 differ; anything else compares with ==."""
    import numpy as np

    if isinstance(a, (float, np.floating)) and isinstance(b, (float, np.floating)):
        if a != a or b != b:
            return a != a and b != b
        return a == b and np.signbit(a) == np.signbit(b)
    return a is not None and b is not None and bool(a == b)


def is_builtin(f) -> bool:
    return isinstance(f, (_BuiltinReduce, _BuiltinFold))
