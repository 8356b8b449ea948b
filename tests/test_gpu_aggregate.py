"""GPU: SimpleEdgeStream.aggregate / globalAggregate with the built-in mappers (gs_agg_*) against the
record-by-record restatement of tests/aggregate_ref.py, in the reference's parallelism-1 order.  The state lives on
the device across calls, so most tests cut one stream into batches in several ways and demand the same output.
Values are compared with valcheck.assert_values: bit for bit for integers, COUNT, MIN / MAX and float sums whose
partial sums are all exact; a general float SUM within valcheck.FLOAT_RTOL."""
import ctypes
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import aggregate_ref as ref
import continuous_ref as cref
import valcheck

pytestmark = pytest.mark.gpu
FIX = json.loads((Path(__file__).parent / "golden" / "continuous_fixtures.json").read_text())
IN, OUT, ALL = 0, 1, 2
SUM, MIN, MAX, COUNT = 0, 1, 2, 3
GS = {"i32": 0, "i64": 1, "f32": 2, "f64": 3}
NP = ref.NP
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SCAN_TILE = 2048   # gs_aggregate.hip's AG_TILE: a power of two <= 16384, so TILE_LENGTHS brackets it


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).cuda() if dev and a is not None else a


def _cuts(n, sizes):
    out, a, i = [], 0, 0
    while a < n:
        b = min(n, a + sizes[min(i, len(sizes) - 1)])
        out.append((a, b))
        a, i = b, i + 1
    return out


def _feed(state, s, d, v, cuts, direction, dev=False, collect=None):
    """the stream through `state` in the given batches: the concatenated (vertices, values)"""
    ks, xs = [], []
    for a, b in cuts:
        cols = (_dev(s[a:b], dev), _dev(d[a:b], dev), None if v is None else _dev(v[a:b], dev))
        k, x = state.edges(*cols, direction) if collect is None else state.global_(*cols, direction, collect)
        ks.append(_np(k).copy())
        xs.append(_np(x).copy())
    return np.concatenate(ks), np.concatenate(xs)


def _split(rows, npdt):
    return np.array([k for k, _ in rows], dtype=np.int64), np.array([x for _, x in rows], dtype=npdt)


def _acc(op, dtype):
    return np.int64 if op == COUNT else NP[dtype]


def _check(got, want, op, dtype, exact=False):
    assert np.array_equal(got[0], want[0]), "vertex column"
    valcheck.assert_values(got[1], want[1], _acc(op, dtype), op, exact=exact)


def _export(state, device=False):
    k, x = state.export(device=device)
    return _np(k).copy(), _np(x).copy()


@functools.lru_cache(maxsize=None)
def _graph(name):
    import __graft_entry__ as ge
    rng = np.random.default_rng(0xA66)
    if name == "rmat":
        s, d = ge.load_oracle().gen_rmat(14, 60_000, 0x5EEDC0)
    elif name == "cut":
        s, d = ge.load_oracle().gen_rmat(14, 6_000, 0x5EEDC1)
    elif name == "growth":
        s, d = rng.integers(0, 30_000, 50_000), rng.integers(0, 30_000, 50_000)
    elif name == "short":      # no vertex has more than 64 records (OUT)
        s, d = rng.permutation(np.repeat(np.arange(1_500), 40)), rng.integers(0, 1_500, 60_000)
    s, d = np.ascontiguousarray(s, dtype=np.int64), np.ascontiguousarray(d, dtype=np.int64)
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


@functools.lru_cache(maxsize=None)
def _values(n, op, dtype, kind="default"):
    """edge values whose float sums are exact (f32: k / 8, k < 64) or in [1, 2) (f64)"""
    rng = np.random.default_rng(0xA660 + 4 * op + GS[dtype])
    if kind == "positive":
        v = rng.uniform(0.5, 2.0, n)
    elif dtype in ("i32", "i64"):
        v = rng.integers(-1000, 1000, n)
    elif op == SUM and dtype == "f32":
        v = rng.integers(0, 64, n) / 8.0
    elif op == SUM:
        v = rng.uniform(1.0, 2.0, n)
    else:
        v = rng.normal(0.0, 100.0, n)
    v = v.astype(NP[dtype])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want(name, op, dtype, direction, kind="default"):
    """the restatement over the whole stream, computed once: records and the final table"""
    s, d = _graph(name)
    v = _values(len(s), op, dtype, kind)
    st = ref.KeyedState(op, dtype)
    rows = st.edges(s.tolist(), d.tolist(), v, direction)
    return _split(rows, _acc(op, dtype)), _split(st.export(), _acc(op, dtype))


def _exact(op, dtype):
    return not (op == SUM and dtype == "f64")


# ---- through the API ------------------------------------------------------------------------------------
class _WeightedDegree:
    """a user vertex mapper (host path): (vertex, sum so far) with a plain dict"""

    def __init__(self):
        self.acc = {}

    def map(self, r):
        self.acc[r[0]] = self.acc.get(r[0], 0) + r[1]
        return (r[0], self.acc[r[0]])


@pytest.mark.parametrize("micro_batch", [None, 3])
def test_fixtures_through_the_api(pkg, engine, micro_batch):
    env = pkg.StreamExecutionEnvironment.getExecutionEnvironment()
    env.setMicroBatch(micro_batch)
    E = FIX["edges"]
    try:
        for dtype in ("i64", "f64", "i32", "f32"):
            g = pkg.SimpleEdgeStream(env.fromCollection(E, value_dtype=NP[dtype]), env)
            for cin, cout, direction in ((True, True, ALL), (True, False, IN), (False, True, OUT)):
                sep = pkg.EdgeValueSeparator(cin, cout)
                for cls, gcls, op in ((pkg.RunningSum, pkg.GlobalRunningSum, SUM), (pkg.RunningMin, pkg.GlobalRunningMin, MIN),
                                      (pkg.RunningMax, pkg.GlobalRunningMax, MAX), (pkg.RunningCount, pkg.GlobalRunningCount, COUNT)):
                    want = [(k, x.item()) for k, x in ref.aggregate(E, op, dtype, direction)]
                    assert g.aggregate(sep, cls()).collect() == want, (dtype, direction, op)
                    for upd in (False, True):
                        want = [x.item() for x in ref.global_aggregate(E, op, dtype, direction, upd)]
                        assert g.globalAggregate(sep, gcls(), upd).collect() == want, (dtype, direction, op, upd)
        g = pkg.SimpleEdgeStream(env.fromCollection(E), env)
        # COUNT is getDegrees; a global COUNT with collectUpdates is numberOfEdges
        assert g.aggregate(pkg.EdgeValueSeparator(True, True), pkg.RunningCount()).collect() == g.getDegrees().collect()
        assert cref.lines(g.globalAggregate(pkg.EdgeValueSeparator(False, True), pkg.GlobalRunningCount(), True).collect()) \
            == sorted(FIX["numberOfEdges"])
        # a user-defined pair runs on the host, record by record
        got = g.aggregate(lambda e, out: (out.collect((e[0], e[2])), out.collect((e[1], e[2]))), _WeightedDegree()).collect()
        assert got == [(k, x.item()) for k, x in ref.aggregate(E, SUM, "i64", ALL)]
        got = g.globalAggregate(pkg.EdgeValueSeparator(True, True), lambda r, out: out.collect(r[1] // 20), True).collect()
        assert got == [0, 1, 2]
        # the one-argument aggregate is still GraphStream.aggregate
        class _Agg:
            def run(self, stream):
                return "ran"
        assert g.aggregate(_Agg()) == "ran"
    finally:
        env.setMicroBatch(None)


# ---- R-MAT scale 14, 60 000 edges ----------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("direction", [IN, OUT, ALL])
@pytest.mark.parametrize("dtype", ["i32", "i64", "f32", "f64"])
@pytest.mark.parametrize("op", [SUM, MIN, MAX, COUNT])
def test_rmat_matches_the_restatement(engine, op, dtype, direction, dev):
    s, d = _graph("rmat")
    v = _values(len(s), op, dtype)
    want, final = _want("rmat", op, dtype, direction)
    with engine.aggregate_state(op, GS[dtype]) as st:
        got = _feed(st, s, d, v, [(0, len(s))], direction, dev)
        _check(got, want, op, dtype, exact=_exact(op, dtype))
        assert st.size() == (len(final[0]), (2 if direction == ALL else 1) * len(s))
        _check(_export(st, device=dev), final, op, dtype, exact=_exact(op, dtype))


def test_f32_sum_within_tolerance_where_runs_are_short(engine):
    """no vertex has more than 64 records and the values are positive: the scan's association and the arrival-order
    fold differ by at most 2 * 63 * 2^-24 = 7.5e-6 relative, inside FLOAT_RTOL = 1e-5"""
    s, d = _graph("short")
    assert np.bincount(s).max() <= 64
    want, final = _want("short", SUM, "f32", OUT, "positive")
    v = _values(len(s), SUM, "f32", "positive")
    with engine.aggregate_state(SUM, GS["f32"]) as st:
        got = _feed(st, s, d, v, _cuts(len(s), [25_000]), OUT, True)
        rel = np.max(np.abs(got[1].astype(np.float64) - want[1]) / want[1])
        print(f"f32 SUM, runs <= 64: worst relative difference {rel:.3g}")
        _check(got, want, SUM, "f32")
        _check(_export(st), final, SUM, "f32")


def test_count_reproduces_cont_degrees(engine):
    s, d = _graph("rmat")
    for direction in (IN, OUT, ALL):
        with engine.aggregate_state(COUNT, None) as st, engine.continuous() as ct:
            for a, b in _cuts(len(s), [33_333]):
                cs, cd = _dev(s[a:b], True), _dev(d[a:b], True)
                k, x = st.edges(cs, cd, None, direction)
                ck, cx = ct.degrees(cs, cd, direction)
                assert torch.equal(k, ck) and torch.equal(x, cx)
            assert st.size() == ct.size()
            ex, cex = _export(st), ct.export()
            assert np.array_equal(ex[0], cex[0]) and np.array_equal(ex[1], cex[1])


# ---- the output does not depend on where the stream is cut -------------------------------------------
def _random_cut(n):
    rng = np.random.default_rng(0xC07)
    return _cuts(n, rng.integers(1, 900, 64).tolist())


CUT_CLASSES = [(SUM, "i64"), (MIN, "i32"), (MAX, "f64"), (SUM, "f32"), (COUNT, "i64")]


@pytest.mark.parametrize("cls", CUT_CLASSES, ids=lambda c: f"op{c[0]}-{c[1]}")
@pytest.mark.parametrize("cut", ["whole", "1", "7", "4096", "4097", "random"])
def test_batch_cut_independence(engine, cut, cls):
    op, dtype = cls
    s, d = _graph("cut")
    n = len(s)
    v = _values(n, op, dtype)
    cuts = _cuts(n, [n]) if cut == "whole" else _random_cut(n) if cut == "random" else _cuts(n, [int(cut)])
    assert cuts[-1][1] == n and (cut == "whole" or len(cuts) > 1)
    want, final = _want("cut", op, dtype, ALL)
    with engine.aggregate_state(op, GS[dtype]) as st:
        _check(_feed(st, s, d, v, cuts, ALL, dev=True), want, op, dtype, exact=True)
        ex = _export(st)
        _check(ex, final, op, dtype, exact=True)
        assert st.size() == (len(final[0]), 2 * n)
    # the global value of the same stream, updates only
    g = ref.GlobalState(op, dtype)
    gw = _split(g.run(s.tolist(), d.tolist(), v, ALL, True), _acc(op, dtype))
    with engine.aggregate_state(op, GS[dtype], mode="global") as st:
        _check(_feed(st, s, d, v, cuts, ALL, dev=True, collect=True), gw, op, dtype, exact=True)
        assert st.size() == (1, 2 * n)
        ek, ex = _export(st)
        assert len(ek) == 1 and ex.tobytes() == _acc(op, dtype)(g.acc).tobytes()


# ---- runs that end at, before and after a scan tile's edge ------------------------------------------
TILE_LENGTHS = sorted({1, 2, 70_000} | {(1 << k) + o for k in range(6, 15) for o in (-1, 0, 1)})
assert SCAN_TILE in TILE_LENGTHS and SCAN_TILE - 1 in TILE_LENGTHS and SCAN_TILE + 1 in TILE_LENGTHS


def _record_stream(seq, rng, pairs):
    """edges whose records, in arrival order, are the vertices of seq (pairs: under ALL, two records per edge; an odd
    sequence gets one more record of vertex 99, which sorts last)"""
    if pairs:
        seq = seq + [99] * (len(seq) % 2)
        s, d = np.array(seq[0::2], dtype=np.int64), np.array(seq[1::2], dtype=np.int64)
    else:
        s, d = np.array(seq, dtype=np.int64), np.zeros(len(seq), dtype=np.int64)
    return s, d, rng.integers(-1000, 1000, len(s)).astype(np.int64)


@pytest.mark.parametrize("L", TILE_LENGTHS)
def test_runs_around_the_tile_edges(engine, L):
    rng = np.random.default_rng(L)
    one = [10] * L
    two = [20] + [10] * (L // 2) + [20] + [10] * (L - L // 2) + [20]   # B's run starts at sorted position L
    for seq in (one, two):
        for direction in (OUT, ALL):
            s, d, v = _record_stream(list(seq), rng, direction == ALL)
            want = _split(ref.KeyedState(SUM, "i64").edges(s.tolist(), d.tolist(), v, direction), np.int64)
            with engine.aggregate_state(SUM, GS["i64"]) as st:
                _check(_feed(st, s, d, v, [(0, len(s))], direction, True), want, SUM, "i64")
            gwant = _split(ref.GlobalState(SUM, "i64").run(s.tolist(), d.tolist(), v, direction, False), np.int64)
            with engine.aggregate_state(SUM, GS["i64"], mode="global") as st:
                _check(_feed(st, s, d, v, [(0, len(s))], direction, True, collect=False), gwant, SUM, "i64")


# ---- special values --------------------------------------------------------------------------------------
SPECIALS = [
    (MIN, "f64", [5.0, float("nan"), 1.0, 2.0]), (MAX, "f32", [5.0, float("nan"), 9.0, 2.0]),   # NaN, then a smaller / larger value
    (SUM, "f64", [float("inf"), 1.0, float("-inf"), 1.0]), (SUM, "f32", [float("inf"), float("-inf"), 3.0]),
    (SUM, "f32", [-0.0, -0.0, 0.0, -0.0]), (SUM, "f64", [-0.0, -0.0]),                          # a first -0.0 stays -0.0
    (MIN, "f64", [0.0, -0.0, 0.0]), (MAX, "f32", [-0.0, 0.0, -0.0]),
    (SUM, "i64", [I64_MAX, 1, I64_MIN, -1]), (SUM, "i64", [I64_MIN, I64_MIN]),                  # wrap at 64 bits
    (SUM, "i32", [2**31 - 1, 1, -2**31, -1]), (MIN, "i32", [-2**31, 2**31 - 1]), (MAX, "i64", [I64_MIN, I64_MAX, 0]),
]


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", range(len(SPECIALS)))
def test_special_values(engine, case, dev):
    op, dtype, vals = SPECIALS[case]
    n = len(vals)
    # vertex 7 takes the values in order; vertex 8 takes them too, interleaved and cut after the first
    s = np.array([7, 8] * n, dtype=np.int64)
    d = np.full(2 * n, 3, dtype=np.int64)
    v = np.repeat(np.array(vals, dtype=NP[dtype]), 2)
    for cuts in ([(0, 2 * n)], [(0, 2), (2, 2 * n)]):
        model = ref.KeyedState(op, dtype)
        want = _split(model.edges(s.tolist(), d.tolist(), v, OUT), NP[dtype])
        with engine.aggregate_state(op, GS[dtype]) as st:
            _check(_feed(st, s, d, v, cuts, OUT, dev), want, op, dtype, exact=True)
            _check(_export(st, dev), _split(model.export(), NP[dtype]), op, dtype, exact=True)
        for upd in (False, True):
            gw = _split(ref.GlobalState(op, dtype).run(s[::2].tolist(), d[::2].tolist(), v[::2], OUT, upd), NP[dtype])
            gcuts = [(0, n)] if len(cuts) == 1 else [(0, 1), (1, n)]
            with engine.aggregate_state(op, GS[dtype], mode="global") as st:
                _check(_feed(st, s[::2], d[::2], v[::2], gcuts, OUT, dev, collect=upd), gw, op, dtype, exact=True)


# ---- id extremes: every int64 is a legal id, the empty-slot value included ---------------------------
EXTREMES = [I64_MIN, I64_MAX, -1, 0, 1]


def _extreme_stream():
    other = [17, -17, 1 << 40, -(1 << 40), 3]
    s, d = [], []
    for rep in range(2):
        for e, o in zip(EXTREMES, other):
            s += [e, o + rep, e]
            d += [o + rep, e, e]
    return np.array(s, dtype=np.int64), np.array(d, dtype=np.int64)


@pytest.mark.parametrize("direction", [IN, OUT, ALL])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_id_extremes_across_two_batches(engine, direction, dev):
    s, d = _extreme_stream()
    v = np.arange(1, len(s) + 1, dtype=np.int64) * 1000
    for op in (SUM, MIN, COUNT):
        model = ref.KeyedState(op, "i64")
        want = _split(model.edges(s.tolist(), d.tolist(), v, direction), np.int64)
        with engine.aggregate_state(op, GS["i64"]) as st:
            _check(_feed(st, s, d, v, _cuts(len(s), [len(s) // 2]), direction, dev), want, op, "i64")
            ex = _export(st, device=dev)
            _check(ex, _split(model.export(), np.int64), op, "i64")
            assert ex[0][0] == I64_MIN and ex[0][-1] == I64_MAX and -1 in ex[0].tolist()


def test_compact_batch_then_wide_batch_share_vertices(engine):
    rng = np.random.default_rng(0xC0DE)
    s1, d1 = rng.integers(0, 3_000, 4_000), rng.integers(0, 3_000, 4_000)
    w = rng.integers(0, 3_000, 4_000) * 7_919_000_003 - (1 << 61)
    s2 = np.where(rng.random(4_000) < 0.5, w, rng.integers(0, 3_000, 4_000))
    d2 = np.where(rng.random(4_000) < 0.5, rng.permutation(w), rng.integers(0, 3_000, 4_000))
    s, d = np.concatenate([s1, s2]).astype(np.int64), np.concatenate([d1, d2]).astype(np.int64)
    assert int(np.max(s1)) < 1 << 32 and int(np.min(s2)) < -(1 << 32) and len(set(s1.tolist()) & set(s2.tolist())) > 100
    v = rng.normal(0, 10, len(s))
    model = ref.KeyedState(MAX, "f64")
    want = _split(model.edges(s.tolist(), d.tolist(), v, ALL), np.float64)
    with engine.aggregate_state(MAX, GS["f64"]) as st:
        _check(_feed(st, s, d, v, [(0, 4_000), (4_000, 8_000)], ALL, True), want, MAX, "f64")
        _check(_export(st), _split(model.export(), np.float64), MAX, "f64")


# ---- table growth -------------------------------------------------------------------------------------
def test_table_growth_keeps_every_accumulator(engine):
    s, d = _graph("growth")
    n = len(s)
    v = _values(n, SUM, "i64")
    model = ref.KeyedState(SUM, "i64")
    with engine.aggregate_state(SUM, GS["i64"], reserve_vertices=16) as st:
        slots0, _ = st.capacity()
        for a, b in _cuts(n, [n // 5]):
            want = _split(model.edges(s[a:b].tolist(), d[a:b].tolist(), v[a:b], ALL), np.int64)
            _check(_feed(st, s[a:b], d[a:b], v[a:b], [(0, b - a)], ALL, True), want, SUM, "i64")
            assert st.size() == (len(model.acc), model.records)
        slots, growths = st.capacity()
        assert growths >= 3 and slots > slots0 and 2 * len(model.acc) <= slots
        _check(_export(st), _split(model.export(), np.int64), SUM, "i64")


def test_empty_batch_and_single_edge(engine):
    e = np.empty(0, dtype=np.int64)
    with engine.aggregate_state(SUM, GS["i64"]) as st:
        for dev in (False, True):
            k, x = st.edges(_dev(e, dev), _dev(e, dev), _dev(e, dev), ALL)
            assert len(k) == 0 and len(x) == 0
        assert st.size() == (0, 0) and len(_export(st)[0]) == 0
        one = (np.array([9], dtype=np.int64), np.array([4], dtype=np.int64), np.array([5], dtype=np.int64))
        k, x = st.edges(*one, ALL)
        assert k.tolist() == [9, 4] and x.tolist() == [5, 5]
        k, x = st.edges(*(_dev(c, True) for c in one), ALL)
        assert k.tolist() == [9, 4] and x.tolist() == [10, 10] and st.size() == (2, 4)
        assert [c.tolist() for c in _export(st)] == [[4, 9], [10, 10]]
    with engine.aggregate_state(MAX, GS["f32"], mode="global") as st:
        k, x = st.global_(e, e, np.empty(0, dtype=np.float32), ALL, True)
        assert len(k) == 0 and st.size() == (0, 0) and len(_export(st)[0]) == 0 and st.capacity() == (0, 0)
        k, x = st.global_(np.array([9]), np.array([4]), np.array([2.5], dtype=np.float32), ALL, True)
        assert k.tolist() == [9] and x.tolist() == [2.5] and x.dtype == np.float32 and st.size() == (1, 2)


# ---- checkpoints ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("cls", [(SUM, "i64"), (MIN, "f32"), (COUNT, "i64")], ids=lambda c: f"op{c[0]}-{c[1]}")
def test_export_load_round_trip_continues_identically(engine, cls, dev):
    op, dtype = cls
    s, d = _graph("cut")
    v = _values(len(s), op, dtype)
    h = len(s) // 2
    want, final = _want("cut", op, dtype, ALL)
    with engine.aggregate_state(op, GS[dtype]) as a, engine.aggregate_state(op, GS[dtype]) as b:
        first = _feed(a, s, d, v, [(0, h)], ALL, dev)
        keys, accs = a.export(device=dev)
        b.load(keys, accs, a.size()[1])
        assert b.size() == a.size()
        _check(_export(b), _export(a), op, dtype, exact=True)
        ra, rb = _feed(a, s, d, v, [(h, len(s))], ALL, dev), _feed(b, s, d, v, [(h, len(s))], ALL, dev)
        _check((np.concatenate([first[0], ra[0]]), np.concatenate([first[1], ra[1]])), want, op, dtype, exact=True)
        _check(rb, ra, op, dtype, exact=True)
        _check(_export(b), final, op, dtype, exact=True)
        with pytest.raises(Exception) as ei:      # a state that has seen records takes no checkpoint
            b.load(keys, accs, 5 * len(keys))
        assert ei.value.status == -1
        _check(_export(b), final, op, dtype, exact=True)
        with engine.aggregate_state(op, GS[dtype]) as c:
            with pytest.raises(Exception) as ei:  # a vertex twice: refused, and the state is empty again
                c.load(np.array([1, 2, 1], dtype=np.int64), np.array([1, 2, 3], dtype=_acc(op, dtype)), 3)
            assert ei.value.status == -1 and c.size() == (0, 0) and len(_export(c)[0]) == 0
            c.load(keys, accs, a.size()[1])
            _check(_feed(c, s, d, v, [(h, len(s))], ALL, dev), ra, op, dtype, exact=True)
    # a global state: one row, the key is ignored
    g = ref.GlobalState(op, dtype)
    g.run(s[:h].tolist(), d[:h].tolist(), v[:h], OUT, True)
    gw = _split(g.run(s[h:].tolist(), d[h:].tolist(), v[h:], OUT, True), _acc(op, dtype))
    with engine.aggregate_state(op, GS[dtype], mode="global") as a, engine.aggregate_state(op, GS[dtype], mode="global") as b:
        _feed(a, s, d, v, [(0, h)], OUT, dev, collect=True)
        keys, accs = a.export(device=dev)
        assert len(keys) == 1
        b.load(keys + 77, accs, h)
        assert b.size() == (1, h)
        _check(_feed(b, s, d, v, [(h, len(s))], OUT, dev, collect=True), gw, op, dtype, exact=True)
        with pytest.raises(Exception) as ei:
            b.load(keys, accs, h)
        assert ei.value.status == -1


# ---- global mode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_global_running_max_emits_the_record_highs(engine, dev):
    rng = np.random.default_rng(0x6A)
    n = 20_000
    v = rng.integers(0, 300, n).astype(np.int64)       # repeated maxima: long plateaus
    v[5_000:5_004] = 1_000                               # a plateau of equal highs ...
    s, d = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64) + n
    for direction, cuts in ((OUT, [(0, n)]), (ALL, [(0, n)]), (ALL, [(0, 5_002), (5_002, n)]), (OUT, _cuts(n, [4_097]))):
        for upd in (True, False):
            gw = _split(ref.GlobalState(MAX, "i64").run(s.tolist(), d.tolist(), v, direction, upd), np.int64)
            with engine.aggregate_state(MAX, GS["i64"], mode="global") as st:
                got = _feed(st, s, d, v, cuts, direction, dev, collect=upd)
                _check(got, gw, MAX, "i64")
                R = n * (2 if direction == ALL else 1)
                assert st.size() == (1, R)
                if upd:     # the record highs, each once -- a cut inside the plateau emits nothing twice
                    assert np.all(np.diff(got[1]) > 0) and got[1].tolist().count(1_000) == 1 and len(got[1]) < 40
                else:
                    assert len(got[1]) == R
    # keys may be NULL in this mode
    from gelly_streaming_amd import _lib as L
    with engine.aggregate_state(MAX, GS["i64"], mode="global") as st:
        x = np.empty(n, dtype=np.int64)
        n_out = ctypes.c_uint64(0)
        b = L.GsEdgeBatch(s.ctypes.data, d.ctypes.data, v.ctypes.data, n, L.GS_I64, L.GS_MEM_HOST, 0)
        vo = L.GsVertexOut(None, x.ctypes.data, n, ctypes.pointer(n_out), L.GS_MEM_HOST, 0)
        assert st._L.gs_agg_global(engine.ctx, st.handle, ctypes.byref(b), OUT, 1, ctypes.byref(vo)) == 0
        gw = _split(ref.GlobalState(MAX, "i64").run(s.tolist(), d.tolist(), v, OUT, True), np.int64)
        assert x[:n_out.value].tolist() == gw[1].tolist()


# ---- failed calls -----------------------------------------------------------------------------------------
def test_failed_calls_leave_the_state_alone(pkg, engine):
    from gelly_streaming_amd import _lib as L
    s, d = _graph("cut")
    v = _values(len(s), SUM, "i64")
    h = 2_000
    lib = pkg.load_library()
    for mode in ("keyed", "global"):
        model = ref.KeyedState(SUM, "i64") if mode == "keyed" else ref.GlobalState(SUM, "i64")
        run = (lambda a, b: model.edges(s[a:b].tolist(), d[a:b].tolist(), v[a:b], ALL)) if mode == "keyed" else \
              (lambda a, b: model.run(s[a:b].tolist(), d[a:b].tolist(), v[a:b], ALL, False))
        feed = lambda st, a, b: _feed(st, s, d, v, [(a, b)], ALL, True, collect=None if mode == "keyed" else False)
        good = lib.gs_agg_edges if mode == "keyed" else (lambda c, t, b, dr, o: lib.gs_agg_global(c, t, b, dr, 0, o))
        other = (lambda c, t, b, dr, o: lib.gs_agg_global(c, t, b, dr, 0, o)) if mode == "keyed" else lib.gs_agg_edges
        with engine.aggregate_state(SUM, GS["i64"], mode=mode) as st:
            _check(feed(st, 0, h), _split(run(0, h), np.int64), SUM, "i64")
            size, ex = st.size(), _export(st)

            def untouched():
                e2 = _export(st)
                return st.size() == size and np.array_equal(e2[0], ex[0]) and np.array_equal(e2[1], ex[1])

            cs, cd, cv = _dev(s[h:], True), _dev(d[h:], True), _dev(v[h:], True)
            R = 2 * len(cs)
            k, x = torch.empty(R, dtype=torch.int64, device="cuda"), torch.empty(R, dtype=torch.int64, device="cuda")
            b = L.GsEdgeBatch(cs.data_ptr(), cd.data_ptr(), cv.data_ptr(), len(cs), L.GS_I64, L.GS_MEM_DEVICE, 0)
            n_out = ctypes.c_uint64(0)
            short = L.GsVertexOut(k.data_ptr(), x.data_ptr(), R - 1, ctypes.pointer(n_out), L.GS_MEM_DEVICE, 0)
            full = L.GsVertexOut(k.data_ptr(), x.data_ptr(), R, ctypes.pointer(n_out), L.GS_MEM_DEVICE, 0)
            assert good(engine.ctx, st.handle, ctypes.byref(b), ALL, ctypes.byref(short)) == L.GS_ECAPACITY
            assert n_out.value == R and untouched()
            for bad in (3, -1):
                assert good(engine.ctx, st.handle, ctypes.byref(b), bad, ctypes.byref(full)) == L.GS_EINVAL and untouched()
            cf = cv.to(torch.float64)
            bf = L.GsEdgeBatch(cs.data_ptr(), cd.data_ptr(), cf.data_ptr(), len(cs), L.GS_F64, L.GS_MEM_DEVICE, 0)
            assert good(engine.ctx, st.handle, ctypes.byref(bf), ALL, ctypes.byref(full)) == L.GS_EINVAL and untouched()
            assert other(engine.ctx, st.handle, ctypes.byref(b), ALL, ctypes.byref(full)) == L.GS_EINVAL and untouched()
            # the same batch with enough room: the right answer, as if nothing had happened
            _check(feed(st, h, len(s)), _split(run(h, len(s)), np.int64), SUM, "i64")
            assert st.size()[1] == 2 * len(s)
    # create refuses what the header rules out
    for args in ((2, SUM, L.GS_I64), (0, 4, L.GS_I64), (0, SUM, L.GS_NONE), (0, SUM, 5)):
        hnd = ctypes.c_void_p()
        assert lib.gs_agg_create(engine.ctx, *args, 0, ctypes.byref(hnd)) == L.GS_EINVAL and not hnd.value


# ---- neighbours on one engine ---------------------------------------------------------------------------
def test_neighbours_on_one_engine_do_not_disturb_each_other(engine):
    from gelly_streaming_amd import _lib as L
    s, d = _graph("cut")
    v = _values(len(s), SUM, "i64")
    cs, cd, cv = _dev(s, True), _dev(d, True), _dev(v, True)
    cuts = _cuts(len(s), [2_500])

    def others(ct, ds, a, b):
        rk, rv = engine.reduce(cs[a:b], cd[a:b], cv[a:b], ALL, L.GS_OP_SUM)
        ck, cx = ct.degrees(cs[a:b], cd[a:b], ALL)
        de = ds.edges(cs[a:b], cd[a:b], cv[a:b])
        return [_np(t).copy() for t in (rk, rv, ck, cx, *de)]

    with engine.continuous() as ct, engine.distinct() as ds:
        alone = [others(ct, ds, a, b) for a, b in cuts]
    want, final = _want("cut", SUM, "i64", ALL)
    ks, xs = [], []
    with engine.continuous() as ct, engine.distinct() as ds, engine.aggregate_state(SUM, GS["i64"]) as st:
        for i, (a, b) in enumerate(cuts):       # before, between and after the aggregate's batches
            got = others(ct, ds, a, b)
            assert all(np.array_equal(g, w) for g, w in zip(got, alone[i]))
            k, x = st.edges(cs[a:b], cd[a:b], cv[a:b], ALL)
            ks.append(_np(k).copy())
            xs.append(_np(x).copy())
        got = others(ct, ds, 0, 1_000)
        with engine.continuous() as ct2, engine.distinct() as ds2:
            assert all(np.array_equal(g, w) for g, w in zip(got[:2], others(ct2, ds2, 0, 1_000)[:2]))
        _check((np.concatenate(ks), np.concatenate(xs)), want, SUM, "i64")
        _check(_export(st), final, SUM, "i64")
