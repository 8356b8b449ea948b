"""GPU: reduce / fold / fold_degree_max in the configuration bench.py times -- GS_FLAG_ASYNC_OUTPUT (the
Engine's default) at a timing level below GS_TIMING_STAGES, where a window returns on the read-back block
the emit kernel's first block writes into pinned host memory (bucket_wait) while the other blocks still
write the outputs, and the same tensor objects window after window (Engine._fold's cached arguments).

Every test makes its own engine ("lean": GS_TIMING_OFF / GS_TIMING_DOMINANT); gs_last_readback says which
read-back each window took.  The reference is the CPU oracle (integers bit-exact, float sums within
FLOAT_RTOL); where noted also an engine with async_outputs=False at the default timing -- the synchronous
read-back the rest of the suite runs."""
import numpy as np
import pytest
import torch

from test_gpu_bucket import BUCKET, SPANS, VALUE_MIXES, _check, _dev, _window

pytestmark = pytest.mark.gpu

I64_MIN = np.iinfo(np.int64).min
LEVELS = pytest.mark.parametrize("level", [0, 1], ids=["off", "dominant"])   # GS_TIMING_OFF, GS_TIMING_DOMINANT

_REF = {}   # references and windows computed once, shared by the timing levels of a case (never modified)


def _once(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _lean(pkg, level, **kw):
    L = pkg._lib
    assert (L.GS_TIMING_OFF, L.GS_TIMING_DOMINANT) == (0, 1)
    e = pkg.Engine(0, **kw)
    e.set_timing(level)
    return e


def _is_early(pkg, e):
    L = pkg._lib
    return e.last_readback() in (L.GS_READBACK_EARLY, L.GS_READBACK_EARLY_TIMEOUT)


def _check_deg(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)


# ---- a. shapes x ops x directions on the early path -----------------------------------------------------
@LEVELS
@pytest.mark.parametrize("shape", list(SPANS))
@pytest.mark.parametrize("direction", [0, 1, 2])
@pytest.mark.parametrize("dtype,op", [(np.int64, 0), (np.int32, 1), (np.int64, 2), (np.float64, 0), (np.float32, 0),
                                      (np.int64, 3)])
def test_early_reduce_shapes(pkg, oracle, level, shape, direction, dtype, op):
    def make():
        rng = np.random.default_rng(hash((shape, direction, op)) & 0xFFFF)
        n = 60000
        s, d = _window(rng, n, SPANS[shape])
        v = oracle.gen_values(n, 11 + op, oracle.DT_OF_NP[np.dtype(dtype)])
        return s, d, v, oracle.window_reduce(s, d, v, direction, op)

    s, d, v, (rk, rv) = _once(("a", shape, direction, np.dtype(dtype).name, op), make)
    with _lean(pkg, level) as e:
        gk, gv = e.reduce(*_dev(s, d, v), direction, op)
        assert e.stage_times().path in BUCKET
        assert _is_early(pkg, e)
        _check(gk, gv, rk, rv, dtype, op)


@LEVELS
def test_early_readback_is_reached(pkg, oracle, level):
    """Of 8 warmed windows at least one returns on the pinned block itself (a loaded machine may push single
    windows past the 2 ms spin, so no single window is required to)."""
    rng = np.random.default_rng(808)
    n = 60000
    s, d = _window(rng, n, 1 << 19)
    v = oracle.gen_values(n, 3, oracle.DT_I64)
    rk, rv = oracle.window_reduce(s, d, v, 2, 0)
    cols = _dev(s, d, v)
    with _lean(pkg, level) as e:
        for _ in range(2):
            e.reduce(*cols, 2, 0)
        e.synchronize()
        how = []
        for _ in range(8):
            gk, gv = e.reduce(*cols, 2, 0)
            how.append(e.last_readback())
            _check(gk, gv, rk, rv, np.int64, 0)
        assert set(how) <= {pkg._lib.GS_READBACK_EARLY, pkg._lib.GS_READBACK_EARLY_TIMEOUT}, how
        assert pkg._lib.GS_READBACK_EARLY in how, how


@LEVELS
@pytest.mark.parametrize("dtype,op,init", [(np.int64, 0, -77), (np.int64, 1, 5), (np.int64, 2, 40000),
                                           (np.int32, 0, 2**31 - 5), (np.float64, 0, 0.25), (np.int64, 3, 1000)])
def test_early_fold_init(pkg, oracle, level, dtype, op, init):
    def make():
        rng = np.random.default_rng(op + 100)
        n = 50000
        s, d = _window(rng, n, 1 << 21)
        v = oracle.gen_values(n, 4, oracle.DT_OF_NP[np.dtype(dtype)])
        return s, d, v, oracle.window_fold(s, d, v, 0, op, init)

    s, d, v, (rk, rv) = _once(("a.fold", np.dtype(dtype).name, op), make)
    with _lean(pkg, level) as e:
        gk, gv = e.fold(*_dev(s, d, v), 0, op, init)
        assert e.stage_times().path in BUCKET
        assert _is_early(pkg, e)
        _check(gk, gv, rk, rv, dtype, op)


@LEVELS
@pytest.mark.parametrize("span", [1 << 10, 1 << 17, 1 << 24])
def test_early_degree_max(pkg, oracle, level, span):
    def make():
        rng = np.random.default_rng(span % 97)
        s, d = _window(rng, 80000, span, hub_frac=0.3)
        return s, d, {(direction, im): oracle.window_fold_degree_max(s, d, direction, im)
                      for direction in (0, 1, 2) for im in (I64_MIN, span // 2)}

    s, d, want = _once(("a.deg", span), make)
    with _lean(pkg, level) as e:
        for (direction, init_max), w in want.items():
            got = e.fold_degree_max(*_dev(s, d), direction, init_max)
            assert e.stage_times().path in BUCKET
            assert _is_early(pkg, e)
            _check_deg(got, w)


# ---- b. host decisions taken from the early block -------------------------------------------------------
class _Pair:
    """A lean engine and the synchronous one (async_outputs=False, default timing) run window by window."""

    def __init__(self, pkg, level):
        self.pkg = pkg
        self.e = _lean(pkg, level)
        self.s = pkg.Engine(0, async_outputs=False)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()
        self.s.close()

    def reduce(self, s, d, v, direction, op, dtype, want, bucket=True):
        """One window on both engines -> (lean stage times, synchronous stage times)."""
        gk, gv = self.e.reduce(*_dev(s, d, v), direction, op)
        t = self.e.stage_times()
        early = _is_early(self.pkg, self.e)
        xk, xv = self.s.reduce(*_dev(s, d, v), direction, op)
        ts = self.s.stage_times()
        assert self.s.last_readback() == self.pkg._lib.GS_READBACK_STREAM
        _check(gk, gv, *want, dtype, op)
        flt = np.issubdtype(np.dtype(dtype), np.floating)
        assert torch.equal(gk, xk) and (flt or torch.equal(gv, xv))   # float sums: LDS-atomic order
        if bucket:
            assert early
        return t, ts

    def degree(self, s, d, direction, init_max, want):
        got = self.e.fold_degree_max(*_dev(s, d), direction, init_max)
        t = self.e.stage_times()
        assert _is_early(self.pkg, self.e)
        ref = self.s.fold_degree_max(*_dev(s, d), direction, init_max)
        _check_deg(got, want)
        for g, x in zip(got, ref):
            assert torch.equal(g, x)
        return t, self.s.stage_times()


def _prediction_windows(oracle):
    out = []
    rng = np.random.default_rng(17)
    for span, off in ((1 << 24, 0), (1 << 16, 0), (1 << 16, 0), (1 << 24, 0), (1 << 20, -(1 << 33)),
                      (1 << 24, 1 << 40), (1 << 24, 0)):
        s, d = _window(rng, 30011, span, off)
        v = oracle.gen_values(30011, 5, oracle.DT_I64)
        out.append((s, d, v, 1, oracle.window_reduce(s, d, v, 1, 0)))
    return out


@LEVELS
def test_early_prediction_shrinks_and_grows(pkg, oracle, level):
    """A missed base / bucket-count prediction read from the early block reruns the window."""
    with _Pair(pkg, level) as p:
        for s, d, v, direction, want in _once("b.pred", lambda: _prediction_windows(oracle)):
            t, ts = p.reduce(s, d, v, direction, 0, np.int64, want)
            assert t.path in BUCKET and ts.path in BUCKET


@LEVELS
@pytest.mark.parametrize("offset", [-(1 << 40), -5000, 123_456_789_012, (1 << 62)])
def test_early_base_prediction(pkg, oracle, level, offset):
    def make():
        out = []
        rng = np.random.default_rng(abs(offset) % 1000)
        for span in (1 << 12, 1 << 20, 1 << 20):
            s, d = _window(rng, 40000, span, offset)
            v = oracle.gen_values(40000, 9, oracle.DT_I64)
            out.append((s, d, v, oracle.window_reduce(s, d, v, 2, 0)))
        return out

    with _Pair(pkg, level) as p:
        for s, d, v, want in _once(("b.base", offset), make):
            t, ts = p.reduce(s, d, v, 2, 0, np.int64, want)
            assert t.path in BUCKET and ts.path in BUCKET


@LEVELS
@pytest.mark.parametrize("dtype", [np.int64, np.int32])
@pytest.mark.parametrize("op", [0, 1, 2])
def test_early_packing_feedback(pkg, oracle, level, dtype, op):
    """The escape count of the early block turns packing off for the following windows."""
    n = 200_003

    def make():
        rng = np.random.default_rng(1000 + op)
        s, d = _window(rng, n, 1 << 22, hub_frac=0.02)
        out = []
        for mix in ("narrow", "sparse_wide", "boundary", "all_wide", "narrow"):
            v = VALUE_MIXES[mix](rng, n).astype(dtype)
            out.append((mix, v, oracle.window_reduce(s, d, v, 1, op)))
        return s, d, out

    s, d, wins = _once(("b.pack", np.dtype(dtype).name, op), make)
    with _Pair(pkg, level) as p:
        for w, (mix, v, want) in enumerate(wins):
            tp, ts = p.reduce(s, d, v, 1, op, dtype, want)
            assert (tp.path, tp.packed, tp.escapes) == (ts.path, ts.packed, ts.escapes), mix
            if mix == "narrow" and w == 0:
                assert tp.packed and tp.escapes == 0
            if mix == "sparse_wide":
                assert tp.packed and 0 < tp.escapes < n // 8
            if mix == "boundary":   # about half the values escape: the following windows store 8-byte values
                assert tp.packed and tp.escapes > n // 8
            if mix == "all_wide" or w == 4:
                assert not tp.packed


@LEVELS
def test_early_packed_sum_wraps_to_zero(pkg, oracle, level):
    """test_packed_integer_sum_wraps_to_zero's hub window: a 32-bit sum back at 0 is still emitted (through
    the histogram, then through the speculative partition)."""
    def make():
        rng = np.random.default_rng(99)
        n_hub, n_rest = 1 << 17, 70_000
        out = []
        for w in range(2):
            s = np.concatenate([np.full(n_hub, 4242, np.int64), rng.integers(5000, 1 << 20, n_rest)])
            d = rng.integers(0, 1 << 20, n_hub + n_rest).astype(np.int64)
            v = np.concatenate([np.full(n_hub, 32768), rng.integers(0, 0xFFFF, n_rest)]).astype(np.int32)
            perm = rng.permutation(len(s))
            s, d, v = s[perm], d[perm], v[perm]
            rk, rv = oracle.window_reduce(s, d, v, 1, 0)
            assert rv[np.searchsorted(rk, 4242)] == 0
            out.append((s, d, v, (rk, rv)))
        return out

    with _Pair(pkg, level) as p:
        for w, (s, d, v, want) in enumerate(_once("b.wrap", make)):
            t, ts = p.reduce(s, d, v, 1, 0, np.int32, want)
            assert t.path == 2 and t.packed and t.speculative == ts.speculative


@LEVELS
@pytest.mark.parametrize("op", [0, 1, 2])
def test_early_packed_presence(pkg, oracle, level, op):
    """test_packed_presence_of_zero_and_escaped_only_vertices' window (histogram, then speculative)."""
    def make():
        rng = np.random.default_rng(555 + op)
        n = 200_000
        out = []
        for w in range(2):
            s, d = _window(rng, n, 1 << 16)
            v = rng.integers(1, 0xFFFF, n).astype(np.int64)
            zero_v = rng.choice(1 << 16, 300, replace=False)
            for j, x in enumerate(zero_v):   # vertices whose every record is 0 (first 150) or escaped
                v[s == x] = 0 if j < 150 else -(1 << 40) - j
            v[rng.random(n) < 0.0005] = 0
            v[rng.random(n) < 0.0005] = 1 << 33
            out.append((s, d, v, oracle.window_reduce(s, d, v, 1, op)))
        return out

    with _Pair(pkg, level) as p:
        for w, (s, d, v, want) in enumerate(_once(("b.presence", op), make)):
            t, ts = p.reduce(s, d, v, 1, op, np.int64, want)
            assert t.path == 2 and t.packed and t.speculative == w == ts.speculative


def _speculative_windows(oracle, direction, dtype, op):
    """test_speculative_partition's sequence: (s, d, v, expected stage_times().speculative, reference)."""
    rng = np.random.default_rng(4242 + 10 * direction + op)
    n = 300_001
    flt = np.issubdtype(np.dtype(dtype), np.floating)

    def win(m, span=1 << 22):
        s, d = _window(rng, m, span, hub_frac=0.1)
        v = rng.integers(0, 0xFFFF, m)
        v[rng.random(m) < 0.001] = -(1 << 40) if dtype == np.int64 else -(1 << 30)   # escapes
        return s, d, (rng.random(m) * 100 if flt else v).astype(dtype)

    seq = [(win(n), 0)]                                # first window: histogram (nothing to predict from)
    seq += [(win(n), 1) for _ in range(4)]
    seq.append((win(n * 3 // 2), 1))                   # regions scale with the record count
    s, d, v = win(n)
    (s if direction != 0 else d)[: n // 2] = 12345     # half the records in bucket 0: regions overflow
    if direction == 2:
        d[: n // 2] = 12345
    seq.append(((s, d, v), 2))
    seq += [(win(n), 0) for _ in range(8)]             # skip = 8
    seq.append((win(n), 1))
    s, d, v = win(n)
    s[n // 3] = d[n // 3] = (1 << 23) + 5              # outside the predicted bucket count
    seq.append(((s, d, v), 2))
    return [(s, d, v, expect, oracle.window_reduce(s, d, v, direction, op)) for (s, d, v), expect in seq]


@LEVELS
@pytest.mark.parametrize("direction,dtype,op", [(1, np.int64, 0), (2, np.int64, 2), (1, np.float64, 0),
                                                (0, np.int64, 3)])
def test_early_speculative_partition(pkg, oracle, level, direction, dtype, op):
    """Hits, the overflow miss, the 8 windows that do not speculate after it, and the out-of-range key: the
    speculative partition's hit / miss word comes back in the early block."""
    flt = np.issubdtype(np.dtype(dtype), np.floating)
    packed = not flt and op != 3
    seq = _once(("b.spec", direction, np.dtype(dtype).name, op), lambda: _speculative_windows(oracle, direction, dtype, op))
    with _Pair(pkg, level) as p:
        for w, (s, d, v, expect, want) in enumerate(seq):
            t, ts = p.reduce(s, d, v, direction, op, dtype, want)
            assert t.path == 2 and t.packed == packed, w
            assert t.speculative == expect and ts.speculative == expect, (w, t.speculative, ts.speculative, expect)


@LEVELS
@pytest.mark.parametrize("op", [0, 3])
def test_early_multi_item_hub(pkg, oracle, level, op):
    """test_bucket_multi_item_hub's window: the item count of the early block (partials > buckets)."""
    def make():
        rng = np.random.default_rng(21 + op)
        n = 700_000
        s, d = _window(rng, n, 1 << 20, hub_frac=0.6)
        v = oracle.gen_values(n, 3, oracle.DT_I64)
        return s, d, v, {direction: oracle.window_reduce(s, d, v, direction, op) for direction in (1, 2)}

    s, d, v, want = _once(("b.hub", op), make)
    buckets = (1 << 20) >> (15 if op == 3 else 14)
    with _Pair(pkg, level) as p:
        for direction in (1, 2):
            t, ts = p.reduce(s, d, v, direction, op, np.int64, want[direction])
            assert t.path in BUCKET and t.partials > buckets
            assert t.partials == ts.partials


@LEVELS
def test_early_sort_fallback_and_back(pkg, oracle, level):
    """A vertex range over the bucket path's (known from the early block) takes the sort path; the next
    window of the engine is back on the bucket path, early."""
    def make():
        rng = np.random.default_rng(3)
        out = []
        for span in (1 << 30, 1 << 20):
            s, d = _window(rng, 30000, span)
            v = oracle.gen_values(30000, 2, oracle.DT_I64)
            out.append((s, d, v, oracle.window_reduce(s, d, v, 1, 0)))
        return out

    wide, narrow = _once("b.sort", make)
    with _Pair(pkg, level) as p:
        t, ts = p.reduce(*wide[:3], 1, 0, np.int64, wide[3], bucket=False)
        assert t.path == 0 and ts.path == 0
        t, ts = p.reduce(*narrow[:3], 1, 0, np.int64, narrow[3])
        assert t.path in BUCKET and ts.path in BUCKET


@LEVELS
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_early_degree_max_far_neighbours(pkg, oracle, level, direction):
    """The 32-bit neighbour policy's wide retry, after an early emit already wrote into the caller's outputs."""
    def make():
        rng = np.random.default_rng(31 + direction)
        n = 90000
        s = rng.integers(0, 1 << 20, n).astype(np.int64)
        d = rng.integers(0, 1 << 20, n).astype(np.int64)
        d[::7] += 1 << 40
        return s, d, {im: oracle.window_fold_degree_max(s, d, direction, im) for im in (I64_MIN, 1 << 41)}

    s, d, want = _once(("b.far", direction), make)
    with _Pair(pkg, level) as p:
        for init_max, w in want.items():
            p.degree(s, d, direction, init_max, w)


@LEVELS
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_early_speculative_degree_max(pkg, oracle, level, direction):
    def make():
        rng = np.random.default_rng(77 + direction)
        n = 250_001
        out = []
        for w in range(6):
            s, d = _window(rng, n, 1 << 21, hub_frac=0.05)
            if w == 4:
                d[::1000] += 1 << 40   # far neighbours (keys stay in range for OUT)
            out.append((s, d, oracle.window_fold_degree_max(s, d, direction, I64_MIN)))
        return out

    with _Pair(pkg, level) as p:
        spec, spec_s = [], []
        for s, d, want in _once(("b.specdeg", direction), make):
            t, ts = p.degree(s, d, direction, I64_MIN, want)
            spec.append(t.speculative)
            spec_s.append(ts.speculative)
        assert spec[1] == spec[2] == spec[3] == 1, spec
        assert spec == spec_s, (spec, spec_s)


# ---- c. windows back to back with no host synchronisation between them ----------------------------------
GROWING = (40_000, 60_000, 100_000, 150_000, 220_000, 300_000)   # ensure() reallocates workspace as n grows


def _growing_windows(oracle):
    rng = np.random.default_rng(0xC0DE)
    out = []
    for n in GROWING:
        s, d = _window(rng, n, 1 << 22, hub_frac=0.02)
        v = oracle.gen_values(n, 7, oracle.DT_I64)
        out.append((s, d, v, oracle.window_reduce(s, d, v, 2, 0), oracle.window_fold_degree_max(s, d, 2, -5)))
    return out


@LEVELS
@pytest.mark.parametrize("shared", [False, True], ids=["own_out", "shared_out"])
def test_back_to_back_reduce(pkg, oracle, level, shared):
    """Six windows enqueued with nothing read in between: each call returns while its emit may still run and
    the next grows the workspace.  own_out: every window's rows are checked afterwards; shared_out: the last
    window's, and the earlier windows' trimmed views are the same buffer (the documented reuse)."""
    wins = _once("c", lambda: _growing_windows(oracle))
    cols = [_dev(s, d, v) for s, d, v, _, _ in wins]
    cap = 2 * GROWING[-1]
    mk = lambda n: (torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"))
    one = mk(cap)
    outs = [one if shared else mk(2 * n) for n in GROWING]
    torch.cuda.synchronize()
    with _lean(pkg, level) as e:
        got, how = [], []
        for c, o in zip(cols, outs):
            got.append(e.reduce(*c, 2, 0, out=o))
            how.append(e.last_readback())
        # nothing was read or waited for until here
        assert pkg._lib.GS_READBACK_STREAM not in how, how
        if shared:
            assert all(gk.data_ptr() == one[0].data_ptr() and gv.data_ptr() == one[1].data_ptr() for gk, gv in got)
            _check(*got[-1], *wins[-1][3], np.int64, 0)
        else:
            for (gk, gv), w in zip(got, wins):
                _check(gk, gv, *w[3], np.int64, 0)


@LEVELS
@pytest.mark.parametrize("shared", [False, True], ids=["own_out", "shared_out"])
def test_back_to_back_degree_max(pkg, oracle, level, shared):
    wins = _once("c", lambda: _growing_windows(oracle))
    cols = [_dev(s, d) for s, d, _, _, _ in wins]
    mk = lambda n: tuple(torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(3))
    one = mk(2 * GROWING[-1])
    outs = [one if shared else mk(2 * n) for n in GROWING]
    torch.cuda.synchronize()
    with _lean(pkg, level) as e:
        got, how = [], []
        for c, o in zip(cols, outs):
            got.append(e.fold_degree_max(*c, 2, -5, out=o))
            how.append(e.last_readback())
        assert pkg._lib.GS_READBACK_STREAM not in how, how
        if shared:
            assert all(g.data_ptr() == b.data_ptr() for r in got for g, b in zip(r, one))
            _check_deg(got[-1], wins[-1][4])
        else:
            for r, w in zip(got, wins):
                _check_deg(r, w[4])


# ---- d. the stream contract of GS_FLAG_ASYNC_OUTPUT -----------------------------------------------------
def _contract_window(oracle):
    rng = np.random.default_rng(0xD)
    n = 120_000
    s, d = _window(rng, n, 1 << 21, hub_frac=0.05)
    v = oracle.gen_values(n, 13, oracle.DT_I64)
    return s, d, v, oracle.window_reduce(s, d, v, 2, 0)


@LEVELS
def test_read_on_another_stream_after_synchronize(pkg, oracle, level):
    """"A caller that reads them on that stream -- or after gs_synchronize -- needs no wait": after
    Engine.synchronize() another stream reads complete rows."""
    s, d, v, (rk, rv) = _once("d", lambda: _contract_window(oracle))
    cols = _dev(s, d, v)
    out = (torch.empty(2 * len(s), dtype=torch.int64, device="cuda"), torch.empty(2 * len(s), dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _lean(pkg, level) as e:
        gk, gv = e.reduce(*cols, 2, 0, out=out)
        assert _is_early(pkg, e)
        e.synchronize()
        with torch.cuda.stream(side):
            ck, cv = gk.clone(), gv.clone()
        side.synchronize()
        _check(ck, cv, rk, rv, np.int64, 0)


@LEVELS
def test_window_on_a_torch_side_stream(pkg, oracle, level):
    """use_torch_stream() inside torch.cuda.stream(s1): the window runs on s1 and a read on s1 sees its rows."""
    s, d, v, (rk, rv) = _once("d", lambda: _contract_window(oracle))
    s1 = torch.cuda.Stream()
    with _lean(pkg, level) as e:
        try:
            with torch.cuda.stream(s1):
                e.use_torch_stream()
                cols = _dev(s, d, v)
                gk, gv = e.reduce(*cols, 2, 0)
                assert _is_early(pkg, e)
                ck, cv = gk.clone(), gv.clone()   # on s1, ordered after the emit
                s1.synchronize()
        finally:
            torch.cuda.synchronize()
            e.use_torch_stream()   # back on the default stream
        _check(ck, cv, rk, rv, np.int64, 0)
        gk, gv = e.reduce(*cols, 2, 0)
        _check(gk, gv, rk, rv, np.int64, 0)


# ---- e. the 2 ms fallback of bucket_wait, made deterministic by stream order ----------------------------
PRELUDE_MS = 20.0   # 10x bucket_wait's 2 ms of spinning: covers the host's time before it starts to spin


@LEVELS
@pytest.mark.parametrize("kind", ["reduce", "degree_max"])
def test_spin_timeout_waits_for_the_stream(pkg, oracle, level, kind):
    """A window enqueued behind >= 20 ms of other work on the engine's stream: the read-back block cannot
    arrive within the 2 ms spin, bucket_wait falls back to hipStreamSynchronize and finds it; the next
    window's sequence word is still in step."""
    L = pkg._lib

    def make():
        rng = np.random.default_rng(0xE)
        n = 100_000
        s, d = _window(rng, n, 1 << 21, hub_frac=0.05)
        v = oracle.gen_values(n, 17, oracle.DT_I64)
        return s, d, v, oracle.window_reduce(s, d, v, 2, 0), oracle.window_fold_degree_max(s, d, 2, I64_MIN)

    s, d, v, want_r, want_d = _once("e", make)
    S, D, V = _dev(s, d, v)
    with _lean(pkg, level) as e:
        if kind == "reduce":
            out = tuple(torch.empty(2 * len(s), dtype=torch.int64, device="cuda") for _ in range(2))
            run = lambda: e.reduce(S, D, V, 2, 0, out=out)
            check = lambda got: _check(*got, *want_r, np.int64, 0)
        else:
            out = tuple(torch.empty(2 * len(s), dtype=torch.int64, device="cuda") for _ in range(3))
            run = lambda: e.fold_degree_max(S, D, 2, I64_MIN, out=out)
            check = lambda got: _check_deg(got, want_d)
        for _ in range(2):   # warm: no allocation between the window's launches and its spin
            check(run())
        # the prelude: sorts of 2^24 elements on the engine's (torch's current) stream
        x = torch.randint(0, 1 << 60, (1 << 24,), dtype=torch.int64, device="cuda")
        buf = (torch.empty_like(x), torch.empty_like(x))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.sort(x, out=buf)
        ev[0].record()
        torch.sort(x, out=buf)
        ev[1].record()
        torch.cuda.synchronize()
        one_ms = ev[0].elapsed_time(ev[1])
        reps = int(1.5 * PRELUDE_MS / max(one_ms, 1e-3)) + 1
        assert reps <= 2000, one_ms
        ev[2].record()
        for _ in range(reps):
            torch.sort(x, out=buf)
        ev[3].record()
        got = run()   # at once, behind the prelude
        how = e.last_readback()
        torch.cuda.synchronize()
        prelude_ms = ev[2].elapsed_time(ev[3])
        print(f"prelude: {reps} sorts of {one_ms:.3f} ms, {prelude_ms:.1f} ms queued; read-back {how}")
        assert prelude_ms >= PRELUDE_MS, (prelude_ms, reps, one_ms)
        assert how == L.GS_READBACK_EARLY_TIMEOUT
        check(got)
        got = run()   # no prelude: the sequence word is in step, the block arrives
        assert _is_early(pkg, e)
        check(got)


# ---- f. where the early path must stay off --------------------------------------------------------------
def _f_window(oracle):
    rng = np.random.default_rng(0xF)
    n = 200_000
    s, d = _window(rng, n, 1 << 21, hub_frac=0.03)
    v = oracle.gen_values(n, 19, oracle.DT_I64)
    return s, d, v


def _f_want(oracle, kind, direction):
    s, d, v = _once("f", lambda: _f_window(oracle))
    if kind == "sum":
        return _once(("f.sum", direction), lambda: oracle.window_reduce(s, d, v, direction, 0))
    return _once(("f.deg", direction), lambda: oracle.window_fold_degree_max(s, d, direction, -5))


@LEVELS
def test_host_columns_wait_for_the_stream(pkg, oracle, level):
    s, d, v = _once("f", lambda: _f_window(oracle))
    with _lean(pkg, level) as e:
        gk, gv = e.reduce(s, d, v, 2, 0)
        assert isinstance(gk, np.ndarray) and e.last_readback() == pkg._lib.GS_READBACK_STREAM
        rk, rv = _f_want(oracle, "sum", 2)
        assert np.array_equal(gk, rk) and np.array_equal(gv, rv)
        got = e.fold_degree_max(s, d, 1, -5)
        assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
        for g, w in zip(got, _f_want(oracle, "deg", 1)):
            assert np.array_equal(g, w)


@LEVELS
@pytest.mark.parametrize("direction", [1, 2])
def test_chunked_windows_wait_for_the_stream(pkg, oracle, level, direction):
    s, d, v = _once("f", lambda: _f_window(oracle))
    S, D, V = _dev(s, d, v)
    with _lean(pkg, level) as e:
        e.set_max_window_records(50_000)
        gk, gv = e.reduce(S, D, V, direction, 0)
        assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
        _check(gk, gv, *_f_want(oracle, "sum", direction), np.int64, 0)
        got = e.fold_degree_max(S, D, direction, -5)
        assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
        _check_deg(got, _f_want(oracle, "deg", direction))
        e.set_max_window_records(0)
        gk, gv = e.reduce(S, D, V, direction, 0)
        assert _is_early(pkg, e)
        _check(gk, gv, *_f_want(oracle, "sum", direction), np.int64, 0)
        got = e.fold_degree_max(S, D, direction, -5)
        assert _is_early(pkg, e)
        _check_deg(got, _f_want(oracle, "deg", direction))


@LEVELS
def test_exchange_windows_wait_for_the_stream(pkg, oracle, level):
    """gs_window_reduce_dist / _fold_degree_max_dist (the owner-grouped emit, the exchange, the merge) are
    unchanged by the flag; a plain window of the same engine afterwards is early again."""
    s, d, v = _once("f", lambda: _f_window(oracle))
    S, D, V = _dev(s, d, v)
    with _lean(pkg, level, flags=pkg._lib.GS_FLAG_TEST_FORCE_EXCHANGE) as e:
        e.comm_init(1, 0, pkg.Engine.comm_unique_id())
        try:
            for _ in range(2):   # the second window's local step speculates (its read-back rides on the exchange)
                gk, gv = e.reduce_dist(S, D, V, 1, 0)
                assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
                _check(gk, gv, *_f_want(oracle, "sum", 1), np.int64, 0)
            got = e.fold_degree_max_dist(S, D, 2, -5)
            assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
            _check_deg(got, _f_want(oracle, "deg", 2))
            gk, gv = e.reduce(S, D, V, 1, 0)
            assert _is_early(pkg, e)
            _check(gk, gv, *_f_want(oracle, "sum", 1), np.int64, 0)
        finally:
            e.comm_destroy()


def test_partials_and_merge_wait_for_the_stream(pkg, oracle):
    """The halves bench.py runs around torch.distributed's all-to-all, at GS_TIMING_OFF: the partials grouped
    by owner and each owner's merge; the owners' rows together are the window's."""
    s, d, v = _once("f", lambda: _f_window(oracle))
    S, D, V = _dev(s, d, v)
    with _lean(pkg, pkg._lib.GS_TIMING_OFF) as e:
        keys, vals, counts = e.reduce_partials(S, D, V, 2, 0, 3)
        assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
        assert len(counts) == 3 and sum(counts) == keys.numel()
        mk, mv, at = [], [], 0
        for c in counts:
            k, x = e.merge_partials(keys[at:at + c], vals[at:at + c], 0)
            assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
            assert bool((k[1:] > k[:-1]).all())
            mk.append(k)
            mv.append(x)
            at += c
        mk, mv = torch.cat(mk), torch.cat(mv)
        order = torch.argsort(mk)
        _check(mk[order], mv[order], *_f_want(oracle, "sum", 2), np.int64, 0)


@LEVELS
def test_sync_engine_at_lean_timing(pkg, oracle, level):
    """async_outputs=False at a lean timing level: every window waits for the stream."""
    s, d, v = _once("f", lambda: _f_window(oracle))
    S, D, V = _dev(s, d, v)
    with _lean(pkg, level, async_outputs=False) as e:
        for _ in range(2):
            gk, gv = e.reduce(S, D, V, 2, 0)
            assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
            _check(gk, gv, *_f_want(oracle, "sum", 2), np.int64, 0)
        got = e.fold_degree_max(S, D, 1, -5)
        assert e.last_readback() == pkg._lib.GS_READBACK_STREAM
        _check_deg(got, _f_want(oracle, "deg", 1))


# ---- g. the cached-argument fast path of Engine._fold ---------------------------------------------------
G_N = 50_000


def _g_windows(oracle):
    """Nine windows of one length: different spans (U differs) and values."""
    rng = np.random.default_rng(0x6)
    out = []
    for i, span in enumerate((1 << 12, 1 << 16, 1 << 20, 1 << 22, 1 << 14, 1 << 18, 1 << 21, 1 << 13, 1 << 19)):
        s, d = _window(rng, G_N, span, offset=1000 * i)
        v = oracle.gen_values(G_N, 30 + i, oracle.DT_I64)
        out.append((s, d, v, oracle.window_reduce(s, d, v, 2, 0)))
    assert len({len(w[3][0]) for w in out[:3]}) == 3
    return out


def _g_out(n=2 * G_N):
    return (torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"))


@LEVELS
def test_cached_args_refilled_in_place(pkg, oracle, level):
    """The same src / dst / val / out objects, refilled with copy_: each result is the current contents'."""
    wins = _once("g", lambda: _g_windows(oracle))
    with _lean(pkg, level) as e:
        S, D, V = _dev(*wins[0][:3])
        out = _g_out()
        for rnd in range(2):
            for s, d, v, (rk, rv) in wins[:3]:
                for t, a in zip((S, D, V), _dev(s, d, v)):
                    t.copy_(a)
                gk, gv = e.reduce(S, D, V, 2, 0, out=out)
                assert _is_early(pkg, e) and len(e._args) == 1
                assert gk.data_ptr() == out[0].data_ptr() and gk.numel() == len(rk)
                _check(gk, gv, rk, rv, np.int64, 0)


@LEVELS
def test_cached_args_eviction(pkg, oracle, level):
    """Nine input sets (one more than Engine._ARGS_KEEP) cycled twice through one out= pair: entries are
    evicted and rebuilt."""
    wins = _once("g", lambda: _g_windows(oracle))
    cols = [_dev(s, d, v) for s, d, v, _ in wins]
    with _lean(pkg, level) as e:
        assert len(cols) == e._ARGS_KEEP + 1
        out = _g_out()
        for rnd in range(2):
            for c, w in zip(cols, wins):
                gk, gv = e.reduce(*c, 2, 0, out=out)
                assert _is_early(pkg, e) and len(e._args) <= e._ARGS_KEEP
                _check(gk, gv, *w[3], np.int64, 0)


@LEVELS
def test_cached_args_see_a_shorter_column(pkg, oracle, level):
    """dst.resize_(n // 2) keeps the storage and data_ptr (nothing can fault); a cache hit must still refuse
    columns of different lengths, as the first call does."""
    s, d, v, (rk, rv) = _once("g", lambda: _g_windows(oracle))[2]
    with _lean(pkg, level) as e:
        S, D, V = _dev(s, d, v)
        out = _g_out()
        for _ in range(2):   # the second call is a hit
            _check(*e.reduce(S, D, V, 2, 0, out=out), rk, rv, np.int64, 0)
        ptr = D.data_ptr()
        D.resize_(G_N // 2)
        assert D.data_ptr() == ptr and D.numel() == G_N // 2
        with pytest.raises(ValueError):
            e.reduce(S, D, V, 2, 0, out=out)
        D.resize_(G_N)
        _check(*e.reduce(S, D, V, 2, 0, out=out), rk, rv, np.int64, 0)
        V.resize_(G_N // 2)
        with pytest.raises(ValueError):
            e.reduce(S, D, V, 2, 0, out=out)
        V.resize_(G_N)
        _check(*e.reduce(S, D, V, 2, 0, out=out), rk, rv, np.int64, 0)


@LEVELS
def test_cached_args_new_out_pair(pkg, oracle, level):
    """After a hit, another out= pair of another length >= R: the rows are right and in the new buffers."""
    s, d, v, (rk, rv) = _once("g", lambda: _g_windows(oracle))[3]
    with _lean(pkg, level) as e:
        cols = _dev(s, d, v)
        a, b = _g_out(), _g_out(2 * G_N + 4096)
        for _ in range(2):
            e.reduce(*cols, 2, 0, out=a)
        e.synchronize()
        b[0].fill_(-1)
        b[1].fill_(-1)
        gk, gv = e.reduce(*cols, 2, 0, out=b)
        assert _is_early(pkg, e)
        assert gk.data_ptr() == b[0].data_ptr() and gv.data_ptr() == b[1].data_ptr()
        _check(gk, gv, rk, rv, np.int64, 0)
        _check(a[0][:len(rk)], a[1][:len(rk)], rk, rv, np.int64, 0)   # the first pair keeps its window's rows


@LEVELS
def test_cached_args_count_and_sum_apart(pkg, oracle, level):
    """COUNT ignores val: the same columns and out= pair under SUM and COUNT are two entries."""
    s, d, v, (rk, rv) = _once("g", lambda: _g_windows(oracle))[1]
    ck, cv = _once("g.count", lambda: oracle.window_reduce(s, d, v, 2, 3))
    with _lean(pkg, level) as e:
        cols = _dev(s, d, v)
        out = _g_out()
        for _ in range(2):
            _check(*e.reduce(*cols, 2, 0, out=out), rk, rv, np.int64, 0)
            _check(*e.reduce(*cols, 2, 3, out=out), ck, cv, np.int64, 3)
        assert len(e._args) == 2
