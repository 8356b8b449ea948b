"""GPU: gs_slice_reduce / gs_slice_fold_degree_max -- every tumbling window of a batch in one call.

The rows must be the per-window entry points' outputs concatenated in window order: each case compares the call with
tests/slice_ref.sliced (oracle.split_windows + the per-window oracle functions), integers, COUNT and float MIN / MAX
bit for bit, float SUM through valcheck.  Shapes: SORT_TILE is 8192 records, the reduce-by-key tile 4096, the window
scan's tile 2048; 20 000 - 70 000 records reach every tile boundary."""
import ctypes
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import op_matrix as M
import slice_ref as S
from valcheck import assert_values

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
IN, OUT, ALL = 0, 1, 2
SUM, MIN, MAX, COUNT = 0, 1, 2, 3
GS_EINVAL, GS_ECAPACITY, GS_EUNSUPPORTED = -1, -2, -6
DTYPES = {"i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}
N, SIZE = 30_000, 1000


def _oracle():
    import __graft_entry__ as ge
    return ge.load_oracle()


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).cuda()   # (a copy: the shared columns are read-only)


# ---- the shared stream: R-MAT s12, 30 000 edges, timestamps out of order over about 50 windows ------------------
@functools.lru_cache(maxsize=None)
def _stream():
    src, dst = _oracle().gen_rmat(12, N, 0x51CE)
    rng = np.random.default_rng(0x51CE)
    ts = rng.integers(-20_000, 30_000, N).astype(np.int64)   # windows -20 .. 29, window 0 twice as long
    for a in (src, dst, ts):
        a.setflags(write=False)
    return src, dst, ts


@functools.lru_cache(maxsize=None)
def _values(name):
    rng = np.random.default_rng(len(name) * 7 + ord(name[1]))
    dt = DTYPES[name]
    if name[0] == "i":
        info = np.iinfo(dt)
        v = rng.integers(-1000, 1000, N).astype(dt)
        v[rng.integers(0, N, 40)] = info.max
        v[rng.integers(0, N, 40)] = info.min
    else:
        # finite floats are integers in [-8, 8), as in test_gpu_special_values.py: every summation order is exact
        # (|sum| < 2^24), so the 1e-5 rule is not at the mercy of a cancelling sum's condition number
        v = rng.integers(-8, 8, N).astype(dt)
        for i, x in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0)):   # planted specials, some sharing a group
            v[rng.integers(0, N, 30)] = x
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want_reduce(direction, op, name, init=None):
    src, dst, ts = _stream()
    orc = _oracle()
    if init is None:
        return S.sliced(orc.window_reduce, src, dst, _values(name), ts, SIZE, direction, op)
    return S.sliced(orc.window_fold, src, dst, _values(name), ts, SIZE, direction, op, init)


def _check(got, want, dtype=np.int64, op=COUNT):
    ws, rb, k, *vals = [_np(x) for x in got]
    assert ws.dtype == np.int64 and np.array_equal(ws, want[0]), (ws[:5], want[0][:5])
    assert np.array_equal(rb.astype(np.uint64), want[1])
    assert k.dtype == np.int64 and np.array_equal(k, want[2])
    assert len(vals) == len(want) - 3
    for g, w in zip(vals, want[3:]):
        assert_values(g, w, dtype, op)


# ---- 1. every direction x op x dtype, host and device columns ---------------------------------------------------
@pytest.mark.parametrize("name", list(DTYPES))
@pytest.mark.parametrize("direction", [IN, OUT, ALL])
def test_every_op_and_dtype(engine, direction, name):
    src, dst, ts = _stream()
    val = _values(name)
    host, dev = (src, dst, val, ts), tuple(_dev(x) for x in (src, dst, val, ts))
    assert 45 <= len(_want_reduce(direction, COUNT, "i64")[0]) <= 50
    for op in (SUM, MIN, MAX) + ((COUNT,) if name == "i64" else ()):
        want = _want_reduce(direction, op, "i64" if op == COUNT else name)
        for s, d, v, t in (host, dev):
            _check(engine.slice_reduce(s, d, v, t, SIZE, direction, op), want, DTYPES[name], op)
    # mixed: device columns with host timestamps
    _check(engine.slice_reduce(dev[0], dev[1], dev[2], ts, SIZE, direction, MIN), _want_reduce(direction, MIN, name),
           DTYPES[name], MIN)


@pytest.mark.parametrize("direction", [IN, OUT, ALL])
def test_fold_with_init_and_degree_fold(engine, direction):
    src, dst, ts = _stream()
    for name, op, init in (("i64", SUM, 1 << 40), ("i32", MAX, 7), ("f64", MIN, -3.5), ("f32", SUM, 0.25),
                           ("i64", COUNT, 5)):
        val = _values(name)
        want = _want_reduce(direction, op, name, init)
        _check(engine.slice_reduce(src, dst, val, ts, SIZE, direction, op, init), want, DTYPES[name], op)
        _check(engine.slice_reduce(_dev(src), _dev(dst), _dev(val), _dev(ts), SIZE, direction, op, init), want,
               DTYPES[name], op)
    for init_max in (I64_MIN, 2000):
        want = S.sliced(_oracle().window_fold_degree_max, src, dst, None, ts, SIZE, direction, init_max)
        _check(engine.slice_fold_degree_max(src, dst, ts, SIZE, direction, init_max), want)
        _check(engine.slice_fold_degree_max(_dev(src), _dev(dst), _dev(ts), SIZE, direction, init_max), want)


# ---- 2. one window: Engine.reduce on the same columns ------------------------------------------------------------
@pytest.mark.parametrize("direction", [IN, OUT, ALL])
def test_one_window_is_engine_reduce(engine, direction):
    src, dst, _ = _stream()
    ts = np.random.default_rng(2).integers(5000, 6000, N)
    for name, op in (("i64", SUM), ("f32", MAX), ("i32", MIN)):
        val = _values(name)
        k, v = engine.reduce(src, dst, val, direction, op)
        ws, rb, gk, gv = engine.slice_reduce(src, dst, val, ts, SIZE, direction, op)
        assert ws.tolist() == [5000] and rb.tolist() == [0, len(k)]
        assert np.array_equal(gk, k)
        assert_values(gv, v, DTYPES[name], op)
    k, d, m = engine.fold_degree_max(src, dst, direction, 100)
    ws, rb, gk, gd, gm = engine.slice_fold_degree_max(src, dst, ts, SIZE, direction, 100)
    assert ws.tolist() == [5000] and rb.tolist() == [0, len(k)]
    assert np.array_equal(gk, k) and np.array_equal(gd, d) and np.array_equal(gm, m)


# ---- 3. the extremes of the window count -------------------------------------------------------------------------
def test_every_record_its_own_window(engine):
    n = 10_000
    src, dst = _oracle().gen_rmat(12, n, 77)
    val = np.arange(n, dtype=np.int64) * 3 - 5
    ts = np.random.default_rng(3).permutation(n).astype(np.int64) * 10 + 3   # one record per 10 ms window
    order = np.argsort(ts)
    ws, rb, k, v = engine.slice_reduce(src, dst, val, ts, 10, OUT, SUM)
    assert len(ws) == n and np.array_equal(ws, ts[order] - 3)
    assert np.array_equal(rb, np.arange(n + 1, dtype=np.uint64))
    assert np.array_equal(k, src[order]) and np.array_equal(v, val[order])
    # ALL: two rows per window (one for a self-loop), device columns
    want = S.sliced(_oracle().window_reduce, src, dst, val, ts, 10, ALL, SUM)
    _check(engine.slice_reduce(_dev(src), _dev(dst), _dev(val), _dev(ts), 10, ALL, SUM), want)
    assert len(want[0]) == n


def test_two_windows(engine):
    src, dst, _ = _stream()
    ts = np.random.default_rng(4).integers(0, 2, N).astype(np.int64) * SIZE + 999
    for name, op in (("i64", SUM), ("f64", SUM)):
        want = S.sliced(_oracle().window_reduce, src, dst, _values(name), ts, SIZE, ALL, op)
        assert want[0].tolist() == [0, 1000]
        _check(engine.slice_reduce(src, dst, _values(name), ts, SIZE, ALL, op), want, DTYPES[name], op)


# ---- 4. a hub: one vertex owns all 30 000 records of one window --------------------------------------------------
@pytest.mark.parametrize("before", [8192, 5000], ids=["boundary_on_record_8192", "boundary_inside_a_tile"])
def test_hub_window(engine, before):
    """`before` records of an earlier window, then the hub's 30 000: sorted, the window boundary falls on record
    `before` -- exactly on the sort tile's edge, or inside a tile."""
    rng = np.random.default_rng(before)
    n = before + N
    src = np.concatenate([rng.integers(0, 3000, before), np.full(N, 1234)]).astype(np.int64)
    dst = rng.integers(0, 3000, n).astype(np.int64)
    ts = np.concatenate([np.full(before, 1500), np.full(N, 2500)]).astype(np.int64)
    p = rng.permutation(n)
    src, dst, ts = src[p], dst[p], ts[p]
    orc = _oracle()
    for name, op in (("i64", SUM), ("f32", MIN), ("f64", SUM)):
        val = np.resize(_values(name), n)
        want = S.sliced(orc.window_reduce, src, dst, val, ts, SIZE, OUT, op)
        assert want[0].tolist() == [1000, 2000] and want[1][2] - want[1][1] == 1
        _check(engine.slice_reduce(src, dst, val, ts, SIZE, OUT, op), want, DTYPES[name], op)
    want = S.sliced(orc.window_fold_degree_max, src, dst, None, ts, SIZE, OUT, I64_MIN)
    _check(engine.slice_fold_degree_max(_dev(src), _dev(dst), _dev(ts), SIZE, OUT, I64_MIN), want)
    want = S.sliced(orc.window_reduce, src, dst, np.zeros(n, np.int64), ts, SIZE, OUT, COUNT)
    _check(engine.slice_reduce(src, dst, None, ts, SIZE, OUT, COUNT), want)


# ---- 5. timestamps -----------------------------------------------------------------------------------------------
def test_negative_timestamps_and_exact_multiples(engine):
    rng = np.random.default_rng(5)
    n = 20_000
    src, dst = _oracle().gen_rmat(10, n, 5)
    val = rng.integers(-99, 99, n).astype(np.int64)
    ts = rng.integers(-6000, 6000, n).astype(np.int64)
    ts[rng.integers(0, n, 3000)] = rng.integers(-6, 7, 3000) * SIZE       # exact multiples of the size, both signs
    ts[:6] = [-1000, -999, -1, 0, 999, 1000]
    want = S.sliced(_oracle().window_reduce, src, dst, val, ts, SIZE, IN, SUM)
    assert np.array_equal(want[0], np.unique(_oracle().window_start(ts, SIZE))) and 0 in want[0] and len(want[0]) == 13
    _check(engine.slice_reduce(src, dst, val, ts, SIZE, IN, SUM), want)
    _check(engine.slice_reduce(_dev(src), _dev(dst), _dev(val), _dev(ts), SIZE, IN, SUM), want)


def test_int64_extreme_timestamps(engine):
    size = 1 << 62
    ts = np.array([I64_MIN + 1, I64_MAX, 0, -1, 1, size, -size, size - 1, 1 - size, I64_MAX - 1], dtype=np.int64)
    src = np.array([1, 1, 2, 2, 3, 1, 1, 3, 2, 1], dtype=np.int64)
    dst = np.arange(10, dtype=np.int64)
    val = np.arange(10, dtype=np.int64) + 100
    want = S.sliced(_oracle().window_reduce, src, dst, val, ts, size, OUT, SUM)
    assert want[0].tolist() == [-size, 0, size]
    _check(engine.slice_reduce(src, dst, val, ts, size, OUT, SUM), want)
    want = S.sliced(_oracle().window_fold_degree_max, src, dst, None, ts, size, ALL, 4)
    _check(engine.slice_fold_degree_max(src, dst, ts, size, ALL, 4), want)


# ---- 6. negative and wide vertex ids -----------------------------------------------------------------------------
def test_full_int64_vertex_range_in_one_window(engine):
    rng = np.random.default_rng(6)
    n = 20_000
    src = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    src[:4] = [I64_MIN, I64_MAX, -1, 0]
    src[100:3000] = src[rng.integers(0, 50, 2900)]    # repeats
    dst = rng.integers(-50, 50, n).astype(np.int64)
    val = rng.integers(-9, 9, n).astype(np.int64)
    ts = rng.integers(-999, 1000, n).astype(np.int64)   # the window that straddles zero
    want = S.sliced(_oracle().window_reduce, src, dst, val, ts, SIZE, OUT, SUM)
    assert want[0].tolist() == [0] and want[2][0] == I64_MIN and want[2][-1] == I64_MAX
    _check(engine.slice_reduce(src, dst, val, ts, SIZE, OUT, SUM), want)
    # negative ids, several windows
    ts2 = rng.integers(0, 5000, n).astype(np.int64)
    src2 = rng.integers(-(1 << 50), -(1 << 50) + 4000, n).astype(np.int64)
    want = S.sliced(_oracle().window_reduce, src2, dst, val, ts2, SIZE, ALL, MAX)
    _check(engine.slice_reduce(src2, dst, val, ts2, SIZE, ALL, MAX), want)


# ---- raw calls: capacities, refusals ------------------------------------------------------------------------------
SENTINEL = 0x5A


def _raw(pkg, engine, src, dst, val, ts, size, direction, op, cap_w, cap_r):
    """gs_slice_reduce into host buffers pre-filled with SENTINEL bytes: (status, n_windows, n_rows, buffers)"""
    L = pkg._lib
    b, keep, _ = engine._batch(src, dst, val)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    odt = np.int64 if op == COUNT or val is None else val.dtype
    bufs = [np.full(max(cap_w, 1), SENTINEL, np.uint8).repeat(8).view(np.int64),
            np.full(cap_w + 1, SENTINEL, np.uint8).repeat(8).view(np.uint64),
            np.full(max(cap_r, 1), SENTINEL, np.uint8).repeat(8).view(np.int64),
            np.full(max(cap_r, 1) * np.dtype(odt).itemsize, SENTINEL, np.uint8).view(odt)]
    nw, nr = ctypes.c_uint64(12345), ctypes.c_uint64(12345)
    out = L.GsSlicedOut(*(ctypes.c_void_p(x.ctypes.data) for x in bufs), None, cap_w, cap_r, ctypes.pointer(nw),
                        ctypes.pointer(nr), L.GS_MEM_HOST, 0)
    st = engine._L.gs_slice_reduce(engine.ctx, ctypes.byref(b), ctypes.c_void_p(ts.ctypes.data), L.GS_MEM_HOST, size,
                                   direction, op, None, ctypes.byref(out))
    return st, nw.value, nr.value, bufs


def _untouched(bufs):
    return all(np.all(x.view(np.uint8) == SENTINEL) for x in bufs)


# ---- 7. the width boundary ---------------------------------------------------------------------------------------
def test_width_boundary(pkg, engine):
    ts = np.array([0, ((1 << 24) - 1) * SIZE], dtype=np.int64)
    dst = np.array([5, 6], dtype=np.int64)
    val = np.array([10, 20], dtype=np.int64)
    fits = np.array([0, (1 << 40) - 1], dtype=np.int64)      # 24 window bits + 40 vertex bits
    wide = np.array([0, 1 << 40], dtype=np.int64)            # ... + 41
    assert S.geometry(fits, dst, ts, SIZE, OUT).wbits + S.geometry(fits, dst, ts, SIZE, OUT).vbits == 64
    want = S.sliced(_oracle().window_reduce, fits, dst, val, ts, SIZE, OUT, SUM)
    _check(engine.slice_reduce(fits, dst, val, ts, SIZE, OUT, SUM), want)
    st, nw, nr, bufs = _raw(pkg, engine, wide, dst, val, ts, SIZE, OUT, SUM, 4, 4)
    assert st == GS_EUNSUPPORTED and _untouched(bufs) and (nw, nr) == (12345, 12345)
    msg = engine._L.gs_last_error(engine.ctx).decode()
    assert "24" in msg and "41" in msg, msg
    # under IN the wide column keys nothing: accepted; and the next call on the ctx is correct
    _check(engine.slice_reduce(wide, dst, val, ts, SIZE, IN, SUM), S.sliced(_oracle().window_reduce, wide, dst, val, ts, SIZE, IN, SUM))
    _check(engine.slice_reduce(fits, dst, val, ts, SIZE, OUT, SUM), want)
    with pytest.raises(pkg.GsError) as e:
        engine.slice_reduce(wide, dst, val, ts, SIZE, OUT, SUM)
    assert e.value.status == GS_EUNSUPPORTED
    # the same stream through the API: the batched call is refused, the loop's records come back
    recs = {}
    for mode in (True, False):
        env = pkg.StreamExecutionEnvironment()
        env._engine = engine
        env.setSliceBatching(mode)
        stream = pkg.SimpleEdgeStream(pkg.EdgeColumns(wide, dst, val, ts), env)
        recs[mode] = stream.slice(pkg.Time.milliseconds(SIZE), pkg.EdgeDirection.OUT).reduceOnEdges(pkg.SumReduce())
        assert env.slice_counts == ({"batched": 0, "loop": 1, "refused": 1} if mode else
                                    {"batched": 0, "loop": 1, "refused": 0})
    assert recs[True].collectWithTimestamps() == recs[False].collectWithTimestamps() == \
        [((0, 10), 999), ((1 << 40, 20), ((1 << 24) - 1) * SIZE + 999)]


# ---- 8. capacities and arguments ---------------------------------------------------------------------------------
def test_capacity_and_arguments(pkg, engine):
    src, dst, ts = (x[:20_000] for x in _stream())
    val = _values("i64")[:20_000]
    want = S.sliced(_oracle().window_reduce, src, dst, val, ts, SIZE, OUT, SUM)
    W, U = len(want[0]), len(want[2])
    for cap_w, cap_r in ((W, U - 1), (W - 1, U), (1, 1), (0, 0)):
        st, nw, nr, bufs = _raw(pkg, engine, src, dst, val, ts, SIZE, OUT, SUM, cap_w, cap_r)
        assert st == GS_ECAPACITY and (nw, nr) == (W, U), (cap_w, cap_r, st, nw, nr)
        st, nw, nr, bufs = _raw(pkg, engine, src, dst, val, ts, SIZE, OUT, SUM, nw, nr)   # the retry, exactly sized
        assert st == 0 and (nw, nr) == (W, U)
        _check(bufs, want)
    # the engine method retries by itself when its first guess of the windows is short
    _check(engine.slice_reduce(src, dst, val, ts, SIZE, OUT, SUM, windows_hint=3), want)
    # arguments
    for size in (0, -1000):
        st, nw, nr, bufs = _raw(pkg, engine, src, dst, val, ts, size, OUT, SUM, W, U)
        assert st == GS_EINVAL and _untouched(bufs)
    st, *_ = _raw(pkg, engine, src, dst, val, ts, SIZE, 7, SUM, W, U)
    assert st == GS_EINVAL
    st, *_ = _raw(pkg, engine, src, dst, None, ts, SIZE, OUT, SUM, W, U)   # SUM without values
    assert st == GS_EINVAL
    # an empty batch: zero windows, row_begin[0] == 0
    e = np.zeros(0, np.int64)
    st, nw, nr, bufs = _raw(pkg, engine, e, e, e, e, SIZE, OUT, SUM, 4, 4)
    assert st == 0 and (nw, nr) == (0, 0) and bufs[1][0] == 0
    ws, rb, k, v = engine.slice_reduce(_dev(e), _dev(e), _dev(e), _dev(e), SIZE, ALL, SUM)
    assert len(ws) == 0 and rb.tolist() == [0] and len(k) == 0 and len(v) == 0
    _check(engine.slice_reduce(src, dst, val, ts, SIZE, OUT, SUM), want)


# ---- 9. the struct against the C compiler ------------------------------------------------------------------------
def test_sliced_out_layout_matches_header(pkg, tmp_path):
    t = pkg._lib.GsSlicedOut
    lines, want = ['printf("%zu\\n", sizeof(gs_sliced_out));'], [ctypes.sizeof(t)]
    for f, _ in t._fields_:
        lines.append(f'printf("%zu\\n", offsetof(gs_sliced_out, {f}));')
        want.append(getattr(t, f).offset)
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gelly_hip.h\"\nint main(){" + "".join(lines) + "}"
    tmp = tmp_path
    (tmp / "sliced_sz.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp / "sliced_sz.c"), "-o", str(tmp / "sliced_sz")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp / "sliced_sz")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want and len(want) == 12


# ---- 10. the ctx rule: nothing carried between calls -------------------------------------------------------------
@pytest.fixture(scope="module")
def own_engine(pkg):
    eng = pkg.Engine(0)
    yield eng
    eng.close()


CATALOGUE = ("reduce_i64_a", "reduce_i64_wide", "csr_all_f64", "tri_b18", "cc_two_phase", "distinct_keyed")


@pytest.mark.parametrize("name", CATALOGUE)
def test_between_other_entry_points(own_engine, name):
    assert name in M.VARIANTS
    src, dst, ts = _stream()
    val = _values("i64")

    def sliced_call():
        _check(own_engine.slice_reduce(src, dst, val, ts, SIZE, ALL, SUM), _want_reduce(ALL, SUM, "i64"))
        want = S.sliced(_oracle().window_fold_degree_max, src[:9000], dst[:9000], None, ts[:9000], SIZE, IN, 9)
        _check(own_engine.slice_fold_degree_max(_dev(src[:9000]), _dev(dst[:9000]), _dev(ts[:9000]), SIZE, IN, 9), want)

    # the variant, the sliced calls, the variant again; then the other order
    M.run_sequence(own_engine, [name], label=f"{name} before the sliced call")
    sliced_call()
    M.run_sequence(own_engine, [name], label=f"{name} after the sliced call")
    sliced_call()
    M.run_sequence(own_engine, [name], M._host, label=f"{name} after the sliced call, again")
    sliced_call()


# ---- 11. the Python API ------------------------------------------------------------------------------------------
def _api(pkg, engine, mode, cols, direction, run):
    env = pkg.StreamExecutionEnvironment()
    env._engine = engine
    env.setSliceBatching(mode)
    stream = pkg.SimpleEdgeStream(pkg.EdgeColumns(*cols), env)
    return run(stream.slice(pkg.Time.milliseconds(SIZE), pkg.EdgeDirection(direction))), env


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_api_batched_equals_loop(pkg, engine, device):
    src, dst, ts = (x[:12_000] for x in _stream())
    put = _dev if device else (lambda x: x)
    runs = {
        "reduce i64 SUM": ("i64", ALL, lambda w: w.reduceOnEdges(pkg.SumReduce())),
        "reduce i32 MIN": ("i32", OUT, lambda w: w.reduceOnEdges(pkg.MinReduce())),
        "reduce COUNT": ("i64", IN, lambda w: w.reduceOnEdges(pkg.CountReduce())),
        "fold i64 MAX": ("i64", OUT, lambda w: w.foldNeighbors((0, -5), pkg.MaxValuesFold())),
        "fold COUNT": ("i64", ALL, lambda w: w.foldNeighbors((0, 3), pkg.CountFold())),
        "degree fold": ("i64", ALL, lambda w: w.foldNeighbors((0, 2, 1500), pkg.DegreeMaxNeighborFold())),
        "reduce f32 MAX": ("f32", IN, lambda w: w.reduceOnEdges(pkg.MaxReduce())),
    }
    for what, (name, direction, run) in runs.items():
        cols = (put(src), put(dst), put(_values(name)[:12_000]), put(ts) if device else ts)
        a, env_a = _api(pkg, engine, True, cols, direction, run)
        b, env_b = _api(pkg, engine, False, cols, direction, run)
        assert env_a.slice_counts == {"batched": 1, "loop": 0, "refused": 0} and env_a.last_slice_plan.batched, what
        assert env_b.slice_counts == {"batched": 0, "loop": 1, "refused": 0} and not env_b.last_slice_plan.batched
        assert len(a.windows) == len(b.windows) > 40
        assert [(w.start, w.end, w.max_timestamp) for w in a.windows] == [(w.start, w.end, w.max_timestamp) for w in b.windows]
        ra, rb = a.collectWithTimestamps(), b.collectWithTimestamps()
        if name == "f32":   # NaN != NaN: compare the columns through valcheck
            for wa, wb in zip(a.windows, b.windows):
                assert np.array_equal(_np(wa.columns[0]), _np(wb.columns[0]))
                assert_values(_np(wa.columns[1]), _np(wb.columns[1]), np.float32, MAX)
        else:
            assert ra == rb and a.collect() == b.collect(), what


def test_api_float_sum(pkg, engine):
    src, dst, ts = (x[:12_000] for x in _stream())
    cols = (src, dst, _values("f64")[:12_000], ts)
    run = lambda w: w.reduceOnEdges(pkg.SumReduce())   # noqa: E731
    a, env_a = _api(pkg, engine, True, cols, OUT, run)
    b, env_b = _api(pkg, engine, False, cols, OUT, run)
    c, env_c = _api(pkg, engine, "auto", cols, OUT, run)
    assert env_a.last_slice_plan.batched and env_a.slice_counts["batched"] == 1
    # "auto" leaves a float SUM to the loop, whatever the crossover
    assert not env_c.last_slice_plan.batched and "float SUM" in env_c.last_slice_plan.reason
    assert env_c.slice_counts == {"batched": 0, "loop": 1, "refused": 0}
    assert len(a.windows) == len(b.windows) == len(c.windows)
    for wa, wb, wc in zip(a.windows, b.windows, c.windows):
        assert (wa.start, wa.end) == (wb.start, wb.end) == (wc.start, wc.end)
        assert np.array_equal(wa.columns[0], wb.columns[0]) and np.array_equal(wc.columns[0], wb.columns[0])
        assert_values(wa.columns[1], wb.columns[1], np.float64, SUM)
        assert_values(wc.columns[1], wb.columns[1], np.float64, SUM)
