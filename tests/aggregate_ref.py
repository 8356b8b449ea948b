"""Plain-Python restatement of SimpleEdgeStream.aggregate / globalAggregate (SimpleEdgeStream.java:493-539) with
the built-in mappers, at parallelism 1: a dict (one value) updated record by record, in Java arithmetic --
integer sums wrap at their width, float sums are numpy.float32 / float64 stepwise sums in arrival order,
MIN / MAX are Math.min / Math.max.  Nothing here sorts or groups: it shares no method with the engine."""
import numpy as np

IN, OUT, ALL = 0, 1, 2
SUM, MIN, MAX, COUNT = 0, 1, 2, 3
NP = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


def expand(src, dst, val, direction):
    """The edge mapper: DegreeTypeSeparator's order (:444-463) with the edge's value where it puts 1L."""
    for i in range(len(src)):
        v = None if val is None else val[i]
        if direction in (OUT, ALL):
            yield int(src[i]), v
        if direction in (IN, ALL):
            yield int(dst[i]), v


def math_min(a, b):
    """Math.min: NaN if either is NaN; -0.0 < +0.0."""
    if a != a:
        return a
    if b != b:
        return b
    if a == 0 and b == 0 and isinstance(a, np.floating):
        return a if np.signbit(a) else b
    return a if a <= b else b


def math_max(a, b):
    if a != a:
        return a
    if b != b:
        return b
    if a == 0 and b == 0 and isinstance(a, np.floating):
        return b if np.signbit(a) else a
    return a if a >= b else b


def combine(op, a, b):
    """a (+) b on numpy scalars of one dtype (COUNT: int64 ones)."""
    if op in (SUM, COUNT):
        with np.errstate(over="ignore", invalid="ignore"):
            return a + b          # numpy integer scalars wrap at their width; floats round once per step
    return math_min(a, b) if op == MIN else math_max(a, b)


class KeyedState:
    """One vertex mapper with a HashMap<K, VV>: vertex -> accumulator, over any number of batches."""

    def __init__(self, op, dtype):
        self.op, self.np = op, (np.int64 if op == COUNT else NP[dtype] if isinstance(dtype, str) else dtype)
        self.acc = {}
        self.records = 0

    def _value(self, v):
        return np.int64(1) if self.op == COUNT else self.np(v)

    def edges(self, src, dst, val, direction):
        out = []
        for k, v in expand(src, dst, val, direction):
            x = self._value(v)
            self.acc[k] = x if k not in self.acc else combine(self.op, self.acc[k], x)
            out.append((k, self.acc[k]))
        self.records += len(out)
        return out

    def export(self):
        return sorted(self.acc.items())


def java_equals(a, b):
    """Long.equals / Double.equals / Float.equals: the bits after NaN canonicalisation (0.0 != -0.0)."""
    if b is None:
        return False
    if isinstance(a, np.floating):
        if a != a or b != b:
            return bool(a != a and b != b)
        return a.tobytes() == b.tobytes()
    return bool(a == b)


class GlobalState:
    """The global vertex mapper (one accumulator) followed, with collect_updates, by GlobalAggregateMapper
    (:525-539), whose previousValue is always the latest running value."""

    def __init__(self, op, dtype):
        self.op, self.np = op, (np.int64 if op == COUNT else NP[dtype] if isinstance(dtype, str) else dtype)
        self.acc = None
        self.records = 0

    def run(self, src, dst, val, direction, collect_updates):
        """[(vertex, value)] of the records kept"""
        out = []
        for k, v in expand(src, dst, val, direction):
            x = np.int64(1) if self.op == COUNT else self.np(v)
            prev = self.acc
            self.acc = x if prev is None else combine(self.op, prev, x)
            self.records += 1
            if not collect_updates or not java_equals(self.acc, prev):
                out.append((k, self.acc))
        return out


def aggregate(edges, op, dtype, direction):
    """SimpleEdgeStream.aggregate over (src, dst, value) tuples"""
    s, d, v = [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges]
    return KeyedState(op, dtype).edges(s, d, v, direction)


def global_aggregate(edges, op, dtype, direction, collect_updates):
    """SimpleEdgeStream.globalAggregate: the bare values"""
    s, d, v = [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges]
    return [x for _, x in GlobalState(op, dtype).run(s, d, v, direction, collect_updates)]
