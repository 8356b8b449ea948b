"""GPU: SimpleEdgeStream.distinct() (gs_distinct_*) against the record-by-record restatement of
tests/distinct_ref.py: exact, and in arrival order.  The edge set lives on the device across calls, so most
tests cut one stream into batches in several ways and demand the same output."""
import ctypes
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import continuous_ref
import distinct_ref as ref

pytestmark = pytest.mark.gpu
FIX = json.loads((Path(__file__).parent / "golden" / "distinct_fixtures.json").read_text())
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MODES = [ref.KEYED, ref.INSTANCE]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()


def _cuts(n, sizes):
    """[(a, b)] covering [0, n): batches of the given sizes, the last size repeating"""
    out, a, i = [], 0, 0
    while a < n:
        b = min(n, a + sizes[min(i, len(sizes) - 1)])
        out.append((a, b))
        a, i = b, i + 1
    return out


def _feed(state, src, dst, cuts, val=None, dev=False, out=None):
    """the stream through `state` in the given batches: the emitted (src, dst, position in the stream) rows,
    and the emitted values' bits"""
    rows, bits = [], []
    for a, b in cuts:
        s, d, v = src[a:b], dst[a:b], None if val is None else val[a:b]
        if dev:
            s, d, v = _dev(s), _dev(d), _dev(v)
        os_, od, ov, oi = state.edges(s, d, v, out=out)
        rows.extend(zip(_np(os_).tolist(), _np(od).tolist(), (_np(oi).astype(np.int64) + a).tolist()))
        if ov is not None:
            bits.extend(_np(ov).view(f"u{_np(ov).dtype.itemsize}").tolist())
    return rows, bits


def _want(src, dst, mode):
    """the restatement over the whole stream as (src, dst, position in the stream) rows"""
    return [(s, d, i) for s, d, _, i in ref.DistinctState(mode).edges(src.tolist(), dst.tolist())]


@functools.lru_cache(maxsize=None)
def _graph(name):
    import __graft_entry__ as ge
    rng = np.random.default_rng(0xD157)
    if name == "rmat":        # 2^20 possible pairs under R-MAT skew: many repeats
        s, d = ge.load_oracle().gen_rmat(10, 40_000, 0x5EEDD1)
    elif name == "growth":
        s, d = rng.integers(0, 30_000, 50_000), rng.integers(0, 30_000, 50_000)
    elif name == "hot":       # one hot pair, a fresh edge every 1 000 positions
        s, d = np.full(70_000, 5), np.full(70_000, 9)
        at = np.arange(0, 70_000, 1000)
        s[at], d[at] = 1_000 + at, 2_000 + at
    s, d = np.ascontiguousarray(s, dtype=np.int64), np.ascontiguousarray(d, dtype=np.int64)
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


@functools.lru_cache(maxsize=None)
def _want_graph(name, mode):
    return _want(*_graph(name), mode)


# ---- the reference's own test, through the API ------------------------------------------------------------
@pytest.mark.parametrize("micro_batch", [None, 3, 1])
@pytest.mark.parametrize("per_vertex", [True, False])
def test_reference_fixture_through_the_api(pkg, engine, per_vertex, micro_batch):
    doubled = [tuple(e) for e in FIX["edges"]] * 2
    env = pkg.StreamExecutionEnvironment.getExecutionEnvironment()
    env.setMicroBatch(micro_batch)
    try:
        g = pkg.SimpleEdgeStream(env.fromCollection(doubled), env)
        e = g.distinct(per_vertex=per_vertex).getEdges()
    finally:
        env.setMicroBatch(None)
    got = list(zip(_np(e.src).tolist(), _np(e.dst).tolist(), _np(e.val).tolist()))
    assert ref.lines(got) == sorted(FIX["distinct" if per_vertex else "instance"])   # the reference's comparison
    assert got == ref.distinct(doubled, ref.KEYED if per_vertex else ref.INSTANCE)     # and arrival order


# ---- batch cuts: R-MAT scale 10, 40 000 edges ------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["host", "device", "device_out"])
@pytest.mark.parametrize("mode", MODES)
def test_output_does_not_depend_on_the_batch_cut(engine, mode, mem):
    s, d = _graph("rmat")
    want = _want_graph("rmat", mode)
    assert 10 * len(want) < 7 * len(s)        # the stream does repeat itself: over 30 % of its edges
    out = None
    if mem == "device_out":
        out = (torch.empty(len(s), dtype=torch.int64, device="cuda"), torch.empty(len(s), dtype=torch.int64, device="cuda"),
               None, torch.empty(len(s), dtype=torch.int64, device="cuda"))
    for sizes in ([len(s)], [4096], [7, 64, 1000]):
        with engine.distinct(mode) as st:
            got, _ = _feed(st, s, d, _cuts(len(s), sizes), dev=mem != "host", out=out)
            assert got == want, sizes
            assert st.size() == (len(want), len(s))


@pytest.mark.parametrize("mode", MODES)
def test_batches_of_one_and_a_second_run(engine, mode):
    s, d = _graph("rmat")
    s, d = s[:600], d[:600]
    want = _want(s, d, mode)
    with engine.distinct(mode) as st:
        assert _feed(st, s, d, _cuts(600, [1]))[0] == want
    runs = []
    for _ in range(2):
        with engine.distinct(mode) as st:
            runs.append(_feed(st, *_graph("rmat"), _cuts(40_000, [4096]), dev=True)[0])
    assert runs[0] == runs[1] == _want_graph("rmat", mode)


# ---- the winner among equal keys of one batch is the smallest arrival index ----------------------------------
def test_first_arrival_wins_inside_one_batch(engine):
    rng = np.random.default_rng(0xF1257)
    pair = rng.permutation(np.repeat(np.arange(64), 1000))
    s, d = (pair // 8 + 100).astype(np.int64), (pair % 8 - 4).astype(np.int64)
    val = np.arange(len(pair), dtype=np.int64)
    first = sorted(int(np.flatnonzero(pair == p)[0]) for p in range(64))
    for dev in (False, True):
        with engine.distinct() as st:
            os_, od, ov, oi = st.edges(*((_dev(s), _dev(d), _dev(val)) if dev else (s, d, val)))
            assert _np(oi).tolist() == first and _np(ov).tolist() == first
            assert _np(os_).tolist() == s[first].tolist() and _np(od).tolist() == d[first].tolist()
            # the same pairs again, now in the log: nothing is emitted
            os_, od, ov, oi = st.edges(s[::-1].copy(), d[::-1].copy(), val) if not dev else st.edges(_dev(s), _dev(d), _dev(val))
            assert len(os_) == len(od) == len(ov) == len(oi) == 0
            assert st.size() == (64, 2 * len(pair))


@pytest.mark.parametrize("sizes", [[70_000], [10_000]])
@pytest.mark.parametrize("mode", MODES)
def test_one_hot_key(engine, mode, sizes):
    s, d = _graph("hot")
    with engine.distinct(mode) as st:
        got, _ = _feed(st, s, d, _cuts(len(s), sizes), dev=True)
    assert got == _want_graph("hot", mode) and len(got) == 71


def test_id_extremes(engine):
    ids = [I64_MIN, -1, 0, 1, 1 << 32, (1 << 32) + 1, I64_MAX]
    pairs = [(a, b) for a in ids for b in ids] * 2
    order = np.random.default_rng(0xE87).permutation(len(pairs))
    s = np.array([pairs[i][0] for i in order], dtype=np.int64)
    d = np.array([pairs[i][1] for i in order], dtype=np.int64)
    want = _want(s, d, ref.KEYED)
    assert len(want) == 49 and sorted((a, b) for a, b, _ in want) == sorted(set(pairs))
    for dev in (False, True):
        for sizes in ([len(s)], [5]):
            with engine.distinct() as st:
                got, _ = _feed(st, s, d, _cuts(len(s), sizes), dev=dev)
                assert got == want
                assert list(zip(*(x.tolist() for x in st.export()))) == [(a, b) for a, b, _ in want]
    got = {(a, b) for a, b, _ in got}
    assert (-1, -1) in got and (1, 1 << 32) in got and (1 << 32, 1) in got and ((1 << 32) + 1, 1) in got
    with engine.distinct("instance") as st:
        got, _ = _feed(st, s, d, _cuts(len(s), [len(s)]))
        assert got == _want(s, d, ref.INSTANCE) and len(got) == 7


# ---- values travel bit for bit -----------------------------------------------------------------------------
def _values(kind, n):
    rng = np.random.default_rng(0x7A1)
    if kind == "i32":
        return rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    if kind == "i64":
        return rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    if kind == "f32":
        bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        bits[:4] = [0x7FC12345, 0x80000000, 0x7F800000, 0xFFA00001]   # a NaN with a payload, -0.0, inf, a signalling NaN
        return bits.view(np.float32)
    bits = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    bits[:3] = [0x7FF8000000ABCDEF, 0x8000000000000000, 0x7FF0000000000000]
    return bits.view(np.float64)


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("kind", ["i32", "i64", "f32", "f64", "none"])
def test_values_are_the_first_arrivals_bit_for_bit(engine, kind, dev):
    s, d = _graph("rmat")
    s, d = s[:5000], d[:5000]
    val = None if kind == "none" else _values(kind, len(s))
    want = _want(s, d, ref.KEYED)
    with engine.distinct() as st:
        got, bits = _feed(st, s, d, _cuts(len(s), [1500]), val=val, dev=dev)
    assert got == want
    if val is None:
        assert bits == []
    else:
        assert bits == val.view(f"u{val.dtype.itemsize}")[[i for _, _, i in want]].tolist()


def test_a_value_column_asked_of_a_batch_without_values(pkg, engine):
    from gelly_streaming_amd import _lib
    s, d = np.array([1, 2], dtype=np.int64), np.array([3, 4], dtype=np.int64)
    buf = np.zeros(2, dtype=np.int64)
    n_out = ctypes.c_uint64(0)
    with engine.distinct() as st:
        b = _lib.GsEdgeBatch(s.ctypes.data, d.ctypes.data, None, 2, _lib.GS_NONE, _lib.GS_MEM_HOST, 0)
        eo = _lib.GsEdgeOut(None, None, buf.ctypes.data, None, 2, ctypes.pointer(n_out), _lib.GS_MEM_HOST, 0)
        assert engine._L.gs_distinct_edges(engine.ctx, st.handle, ctypes.byref(b), ctypes.byref(eo)) == _lib.GS_EINVAL
        assert st.size() == (0, 0)


# ---- growth ------------------------------------------------------------------------------------------------
def test_growth_matches_a_reserved_state(engine):
    s, d = _graph("growth")
    cuts = _cuts(len(s), [777])
    want = _want_graph("growth", ref.KEYED)
    outs = {}
    for name, reserve in (("growing", 0), ("reserved", len(s) + 777)):
        with engine.distinct(reserve_edges=reserve) as st:
            rows = []
            for a, b in cuts:
                rows.extend(_feed(st, s, d, [(a, b)])[0])
                assert st.size()[0] <= st.capacity()[0] // 2
            outs[name] = (rows, st.capacity()[1], st.size())
    assert outs["growing"][0] == outs["reserved"][0] == want
    assert outs["growing"][1] > 0 and outs["reserved"][1] == 0
    assert outs["growing"][2] == outs["reserved"][2] == (len(want), len(s))


# ---- a failing call leaves the state alone ------------------------------------------------------------------
def test_failure_leaves_the_state_alone(pkg, engine):
    from gelly_streaming_amd import _lib
    L = engine._L
    s, d = _graph("rmat")
    with engine.distinct() as st:
        first, _ = _feed(st, s, d, [(0, 3000)])
        size, log = st.size(), [x.tolist() for x in st.export()]
        bs, bd = np.ascontiguousarray(s[3000:5000]), np.ascontiguousarray(d[3000:5000])
        n = len(bs)
        os_, od, oi = (np.zeros(n, dtype=np.int64) for _ in range(3))
        n_out = ctypes.c_uint64(0)

        def call(handle=st.handle, capacity=n, np_out=ctypes.pointer(n_out), dtype=_lib.GS_NONE, ctx=engine.ctx):
            b = _lib.GsEdgeBatch(bs.ctypes.data, bd.ctypes.data, None, n, dtype, _lib.GS_MEM_HOST, 0)
            eo = _lib.GsEdgeOut(os_.ctypes.data, od.ctypes.data, None, oi.ctypes.data, capacity, np_out, _lib.GS_MEM_HOST, 0)
            return L.gs_distinct_edges(ctx, handle, ctypes.byref(b), ctypes.byref(eo))

        def unchanged():
            return st.size() == size and [x.tolist() for x in st.export()] == log

        assert call(capacity=n - 1) == _lib.GS_ECAPACITY and n_out.value == n and unchanged()
        assert call(np_out=None) == _lib.GS_EINVAL and unchanged()
        assert call(dtype=17) == _lib.GS_EINVAL and unchanged()
        if pkg.Engine.device_count() > 1:
            with pkg.Engine(1) as other, other.distinct() as foreign:
                assert call(handle=foreign.handle) == _lib.GS_EINVAL and foreign.size() == (0, 0)
            assert unchanged()
        # the same batch with room
        assert call() == _lib.GS_OK
        k = n_out.value
        got = first + list(zip(os_[:k].tolist(), od[:k].tolist(), (oi[:k] + 3000).tolist()))
        assert got == _want(s[:5000], d[:5000], ref.KEYED)
        # all four columns NULL: the state is updated and the count reported
        b = _lib.GsEdgeBatch(bs.ctypes.data, bd.ctypes.data, None, n, _lib.GS_NONE, _lib.GS_MEM_HOST, 0)
        eo = _lib.GsEdgeOut(None, None, None, None, 0, ctypes.pointer(n_out), _lib.GS_MEM_HOST, 0)
        assert L.gs_distinct_edges(engine.ctx, st.handle, ctypes.byref(b), ctypes.byref(eo)) == _lib.GS_OK
        assert n_out.value == 0 and st.size() == (len(got), 7000)


# ---- checkpoint ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_checkpoint_and_restore(pkg, engine, mode, device):
    from gelly_streaming_amd import _lib
    s, d = _graph("rmat")
    half = len(s) // 2
    want = _want_graph("rmat", mode)
    with engine.distinct(mode) as st:
        a, _ = _feed(st, s, d, _cuts(half, [4096]))
        es, ed = st.export(device=device)
        assert list(zip(_np(es).tolist(), _np(ed).tolist())) == [r[:2] for r in a]      # the output stream so far
        with engine.distinct(mode) as fresh:
            fresh.load(es, ed)
            assert fresh.size() == (len(a), len(a))
            b = _feed(fresh, s[half:], d[half:], _cuts(len(s) - half, [4096]))[0]
            assert a + [(x, y, i + half) for x, y, i in b] == want
            assert [x.tolist() for x in fresh.export()] == [[r[0] for r in want], [r[1] for r in want]]
            with pytest.raises(pkg.GsError) as err:      # not empty any more
                fresh.load(es, ed)
            assert err.value.status == _lib.GS_EINVAL and fresh.size()[0] == len(want)
        # rows in another order, each of them three times: taken once
        with engine.distinct(mode) as again:
            rs, rd = np.tile(_np(es)[::-1], 3), np.tile(_np(ed)[::-1], 3)
            again.load(rs, rd)
            assert again.size() == (len(a), len(a))
            b = _feed(again, s[half:], d[half:], _cuts(len(s) - half, [4096]))[0]
            assert [(x, y, i + half) for x, y, i in b] == want[len(a):]


# ---- composition with the other operators -------------------------------------------------------------------
def test_distinct_then_degrees(pkg, engine):
    s, d = _graph("rmat")
    s, d = s[:6000], d[:6000]
    env = pkg.StreamExecutionEnvironment.getExecutionEnvironment()
    env.setMicroBatch(1000)
    try:
        got = pkg.SimpleEdgeStream(pkg.EdgeColumns(s, d), env).distinct().getDegrees().collect()
    finally:
        env.setMicroBatch(None)
    edges = ref.distinct(list(zip(s.tolist(), d.tolist())))
    assert got == continuous_ref.get_degrees(edges, continuous_ref.ALL)


def test_distinct_then_windows(pkg, engine, oracle):
    """repeats across and inside windows: each edge counts once, in the window of its first arrival"""
    rng = np.random.default_rng(0x3D6E)
    n = 3000
    s, d = rng.integers(0, 40, n), rng.integers(0, 40, n)
    val = rng.integers(-1000, 1000, n)
    ts = np.sort(rng.integers(0, 2000, n))            # five windows of 400 ms
    edges = list(zip(s.tolist(), d.tolist(), val.tolist(), ts.tolist()))
    kept = ref.distinct(edges)
    assert 5 * len(kept) < 4 * n and len({t // 400 for *_, t in kept}) == 5
    env = pkg.StreamExecutionEnvironment.getExecutionEnvironment()
    env.setMicroBatch(700)
    try:
        dist = pkg.SimpleEdgeStream(env.fromCollection(edges), env).distinct()
    finally:
        env.setMicroBatch(None)
    e = dist.getEdges()
    assert list(zip(_np(e.src).tolist(), _np(e.dst).tolist(), _np(e.val).tolist(), _np(e.ts).tolist())) == kept
    pipeline = lambda g: g.slice(pkg.Time.milliseconds(400), pkg.EdgeDirection.ALL).reduceOnEdges(pkg.SumReduce())
    got = pipeline(dist).collectWithTimestamps()
    assert got == pipeline(pkg.SimpleEdgeStream(env.fromCollection(kept), env)).collectWithTimestamps()
    want = []
    for w in range(5):
        rows = [r for r in kept if r[3] // 400 == w]
        k, v = oracle.window_reduce(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]),
                                    np.array([r[2] for r in rows]), oracle.DIR_ALL, oracle.OP_SUM)
        want.extend(((int(a), int(b)), 400 * (w + 1) - 1) for a, b in zip(k, v))
    assert got == want
