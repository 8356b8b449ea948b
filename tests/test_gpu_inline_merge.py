"""GPU: multi-item buckets merged inside k_bk_accum (the last item of a bucket of 2 .. GS_BK_INLINE_K items
adds the other items' slabs into its LDS table) and the merge launches a speculative window skips when its
predecessor had no bucket that needs them.

A bucket is 2^14 consecutive ids (2^15 with 4-byte accumulators) and an item 2^17 records at these sizes, so
shape A's buckets have 1 .. 7 items under OUT and up to 13 under ALL: single-item buckets, inline merges of 2,
3 and 4 slabs, and buckets past the limit that keep k_bk_merge_groups / _slices / k_bk_merge.  Shape B has
A's proportions with every bucket at 2^17 records or fewer: B -> A hits the speculative scatter (the regions
scale with the record count) but needs the merge launches B's window said it would not.

Sequences that depend on what the engine saw before make their own engine."""
import numpy as np
import pytest

from test_gpu_bucket import _check, _dev

pytestmark = pytest.mark.gpu

W = 1 << 14
A_COUNTS = (150_000, 300_000, 524_288, 524_289, 0, 700, 800_000)
B_COUNTS = tuple(c * 131_000 // 800_000 for c in A_COUNTS)
assert max(B_COUNTS) <= 1 << 17

_REF = {}   # windows and references computed once (never modified)


def _once(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _shape(counts, seed):
    """src and dst ids drawn per bucket (dst: the same buckets in another order, so ALL doubles every count);
    values mostly below 2^16 with zeros, negatives and about 1 % above 2^16."""
    rng = np.random.default_rng(seed)
    bucket = np.repeat(np.arange(len(counts)), counts)
    n = len(bucket)
    s = bucket[rng.permutation(n)] * W + rng.integers(0, W, n)
    d = bucket[rng.permutation(n)] * W + rng.integers(0, W, n)
    v = rng.integers(1, 1 << 16, n)
    v[rng.random(n) < 0.01] = 0
    neg = rng.random(n) < 0.01
    v[neg] = -rng.integers(1, 1 << 20, int(neg.sum()))
    wide = rng.random(n) < 0.01
    v[wide] = rng.integers(1 << 16, 1 << 30, int(wide.sum()))
    return s.astype(np.int64), d.astype(np.int64), v.astype(np.int64)


def _a():
    return _once("A", lambda: _shape(A_COUNTS, 0xA))


def _b():
    return _once("B", lambda: _shape(B_COUNTS, 0xB))


def _want(oracle, name, dtype, direction, op):
    s, d, v = _a() if name == "A" else _b()
    return _once((name, np.dtype(dtype).name, direction, op),
                 lambda: oracle.window_reduce(s, d, v.astype(dtype), direction, op))


@pytest.mark.parametrize("direction", [1, 2], ids=["out", "all"])
@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("op", [0, 1, 2], ids=["sum", "min", "max"])
def test_shape_a_three_windows(pkg, oracle, direction, dtype, op):
    """Histogram path, then two speculative windows: each bit-exact."""
    s, d, v = _a()
    rk, rv = _want(oracle, "A", dtype, direction, op)
    cols = _dev(s, d, v.astype(dtype))
    with pkg.Engine(0) as e:
        for w in range(3):
            gk, gv = e.reduce(*cols, direction, op)
            t = e.stage_times()
            assert t.path == 2 and t.speculative == (1 if w else 0), (w, t.path, t.speculative)
            assert t.partials > 7   # multi-item buckets
            _check(gk, gv, rk, rv, dtype, op)


def test_transitions(pkg, oracle):
    """B, B, A, A, B, A twice over on one engine: bit-exact whether the skipped merge launches were predicted
    right (window 1), the window reran (window 2: the scatter hits, the plan finds buckets for the launches
    that were skipped) or the histogram path ran.  Then A, B, B on another engine: merges launched with no
    bucket for them, then skipped."""
    cols = {"A": _dev(*_a()), "B": _dev(*_b())}
    want = {k: _want(oracle, k, np.int64, 1, 0) for k in cols}
    with pkg.Engine(0) as e:
        spec = []
        for name in "BBAABA" * 2:
            gk, gv = e.reduce(*cols[name], 1, 0)
            spec.append(e.stage_times().speculative)
            _check(gk, gv, *want[name], np.int64, 0)
        assert spec[:3] == [0, 1, 2], spec
    with pkg.Engine(0) as e:
        spec = []
        for name in "ABB":
            gk, gv = e.reduce(*cols[name], 1, 0)
            spec.append(e.stage_times().speculative)
            _check(gk, gv, *want[name], np.int64, 0)
        assert spec == [0, 1, 1], spec


def test_planned_multi_item_bucket_stays_empty(pkg, oracle):
    """A bucket planned with two items (140,000 records in the window before: a capacity over 2^17) receives no
    record at all, while the other buckets take its records (+3.5 %, inside the regions' 1/16 slack): the
    window still hits, every item of that bucket is idle and its count stays 0."""
    full = (140_000,) + (400_000,) * 10   # the others: 4 items by capacity in either window (no bucket crosses
    gone = (0,) + (414_000,) * 10         # GS_BK_INLINE_K, which would be a miss of its own)
    assert sum(full) == sum(gone)
    wins = {k: _once(("C", k), lambda c=c, k=k: _shape(c, 0xC0 + k)) for k, c in enumerate((full, gone))}
    want = {k: _once(("C.ref", k), lambda k=k: oracle.window_reduce(*wins[k], 1, 0)) for k in wins}
    assert want[1][0].min() >= W   # nothing in bucket 0
    cols = {k: _dev(*wins[k]) for k in wins}
    with pkg.Engine(0) as e:
        spec = []
        for k in (0, 0, 1, 1):
            gk, gv = e.reduce(*cols[k], 1, 0)
            spec.append(e.stage_times().speculative)
            _check(gk, gv, *want[k], np.int64, 0)
        assert spec == [0, 1, 1, 1], spec


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_float_sums_keep_the_launched_merges(pkg, oracle, dtype):
    s, d, v = _a()
    rk, rv = _want(oracle, "A", dtype, 1, 0)
    cols = _dev(s, d, v.astype(dtype))
    with pkg.Engine(0) as e:
        for w in range(2):
            gk, gv = e.reduce(*cols, 1, 0)
            _check(gk, gv, rk, rv, dtype, 0)   # within 1e-5 relative


def test_degree_max(engine, oracle):
    s, d, _ = _a()
    want = _once("A.deg", lambda: oracle.window_fold_degree_max(s, d, 1, -5))
    S, D = _dev(s, d)
    for w in range(2):
        for g, x in zip(engine.fold_degree_max(S, D, 1, -5), want):
            assert np.array_equal(g.cpu().numpy(), x)


def test_no_spec(pkg, oracle):
    rk, rv = _want(oracle, "A", np.int64, 1, 0)
    cols = _dev(*_a())
    with pkg.Engine(0, no_spec=True) as e:
        for w in range(2):
            gk, gv = e.reduce(*cols, 1, 0)
            assert e.stage_times().speculative == 0
            _check(gk, gv, rk, rv, np.int64, 0)
