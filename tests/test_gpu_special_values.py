"""GPU: float specials (NaN, +-inf, signed zeros, denormals, +-MAX) and integer extremes on every
reduce / fold path, against the CPU oracle.

The other value tests draw floats from oracle.gen_values, i.e. from [0, 1): on such values LDS integer
atomics order floats correctly and fminf agrees with Math.min, so neither "float MIN / MAX refuse the
bucket path" nor java_min / java_max (gs_rbk.hpp: NaN wins, -0.0 < +0.0) was pinned.  Here:

  float MIN / MAX   sort path (path 0 on a default engine): 32-bit, wide (ids to 2^40) and negative keys;
                    foldNeighbors' init; the chunked window; partials + merge
  float SUM         sort path (sort_only engine) and bucket path: one bucket, direct partition, onesweep
                    partition, a speculative second window, a multi-item hub bucket (LDS slabs that hold
                    -0.0, NaN and infinities), foldNeighbors' init; chunked; partials + merge
  integer ops       values equal to the LDS identity of the op (MAX_INT under MIN, MIN_INT under MAX), sums
                    that wrap to exactly 0: packed, unpacked (no_pack) and histogram-only (no_spec) engines

Every float window: a hub vertex (a third of the records: its run crosses several tiles of every
sort-path kernel, so the look-back carry takes its NaN across tiles) with no special / NaN first / NaN
last; ~2% of the other records NaN, +-inf, +-0.0; planted vertices with a literal table of the value
Java's rules give (checked on the oracle's output before any GPU call).  Finite values are integers in
[-8, 8): every summation order is exact in f32 (|sum| < 2^24), so sums are compared bit for bit too,
including the sign of a cancelled zero.  No partial sum overflows: the one documented divergence (f32
SUM accumulates in f64 on the bucket path, so a reference f32 fold that overflows midway to inf can
differ) is out of these inputs on purpose."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from valcheck import assert_values

pytestmark = pytest.mark.gpu

SUM, MIN, MAX = 0, 1, 2
OUT, ALL = 1, 2
BUCKET = (1, 2)
NAN, INF = float("nan"), float("inf")
FLOATS = [np.float32, np.float64]
HUBS = ["none", "first", "last"]


# ---- windows ---------------------------------------------------------------------------------------
def _planted(dtype, op):
    """name -> (values in arrival order, MIN, MAX, SUM by Java's Math.min / Math.max / +).  +-MAX is planted
    for MIN / MAX only: under SUM a sequential f32 fold from an init absorbs the init into MAX (0.25 + MAX
    - MAX = 0), which is the fold's own rounding, not a rule of the op."""
    fi = np.finfo(dtype)
    mx, dn = float(fi.max), float(fi.smallest_subnormal)
    table = {
        "pos_zeros": ([0.0] * 4, 0.0, 0.0, 0.0),
        "neg_zeros": ([-0.0] * 4, -0.0, -0.0, -0.0),
        "pos_then_neg_zero": ([0.0, -0.0], -0.0, 0.0, 0.0),
        "neg_then_pos_zero": ([-0.0, 0.0], -0.0, 0.0, 0.0),
        "neg_inf_and_5": ([-INF, 5.0], -INF, 5.0, -INF),
        "both_infs": ([INF, -INF], -INF, INF, NAN),
        "nan_first": ([NAN, 3.0, -2.0], NAN, NAN, NAN),
        "nan_last": ([3.0, -2.0, NAN], NAN, NAN, NAN),
        "nan_only": ([NAN], NAN, NAN, NAN),
        "denorm_and_zero": ([dn, -dn, 0.0], -dn, dn, 0.0),
        "denorm_multiples": ([dn, 3 * dn, 2 * dn], dn, 3 * dn, 6 * dn),
    }
    if op != SUM:
        table["flt_max"] = ([mx, -mx], -mx, mx, 0.0)
    return table


def _key_of(keys, span):
    if keys == "wide":       # ids up to 2^40: 64-bit sort keys
        return lambda i: np.int64(5) + np.asarray(i, np.int64) * np.int64((1 << 40) // span)
    if keys == "negative":   # the sign bit varies
        return lambda i: np.asarray(i, np.int64) - np.int64(span // 2)
    return lambda i: np.asarray(i, np.int64)


@functools.lru_cache(maxsize=None)
def _window(dtype, op, n, span, keys, hub, seed, hub_frac=1 / 3):
    """src / dst / values of one window for SUM, or for MIN and MAX (which share it).  Index space
    [0, span): the hub at span // 3, the planted vertices and a sink right after it (so they share the
    hub's bucket), every other index ordinary.  Planted records go to the sink (direction ALL: the sink
    takes their specials, the planted vertices only their own values); the hub and the planted vertices
    never appear as a destination."""
    if op == MAX:
        return _window(dtype, MIN, n, span, keys, hub, seed, hub_frac)
    rng = np.random.default_rng(seed)
    table = _planted(dtype, op)
    hub_i = span // 3
    planted_i = {name: hub_i + 1 + j for j, name in enumerate(table)}
    sink_i = hub_i + 1 + len(table)
    ordinary = np.setdiff1d(np.arange(span), [hub_i, sink_i, *planted_i.values()])
    s = ordinary[rng.integers(0, len(ordinary), n)]
    d = ordinary[rng.integers(0, len(ordinary), n)]
    v = rng.integers(-8, 8, n).astype(dtype)
    is_hub = rng.random(n) < hub_frac
    s[is_hub] = hub_i
    special = (rng.random(n) < 0.02) & ~is_hub
    v[special] = rng.choice(np.array([NAN, INF, -INF, 0.0, -0.0], dtype), int(special.sum()))
    pos = rng.permutation(rng.choice(np.flatnonzero(~is_hub), sum(len(t[0]) for t in table.values()), replace=False))
    at = 0
    for name, (vals, *_) in table.items():
        p = np.sort(pos[at:at + len(vals)])   # arrival order = the order listed
        at += len(vals)
        s[p], d[p], v[p] = planted_i[name], sink_i, np.array(vals, dtype)
    hp = np.flatnonzero(is_hub)
    hub_vals = [int(x) for x in v[hp]]
    if hub == "first":
        v[hp[0]] = NAN
    elif hub == "last":
        v[hp[-1]] = NAN
    key = _key_of(keys, span)
    w = SimpleNamespace(s=key(s), d=key(d), v=v, dtype=dtype, hub=hub, hub_id=int(key(hub_i)), hub_vals=hub_vals,
                        hub_records=len(hp), planted={name: int(key(i)) for name, i in planted_i.items()},
                        table=table, want={})
    for a in (w.s, w.d, w.v):
        a.setflags(write=False)
    return w


def _same(a, b):
    """bit for bit, or both NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.isnan(a) and np.isnan(b)) or a.tobytes() == b.tobytes()


def _want(oracle, w, direction, op):
    """The oracle's rows for the window's reduce, computed once.  Before they serve as a reference, on the
    oracle's output alone: at least 75% of the rows are not NaN (so they are compared bit for bit), and the
    hub and every planted vertex hold the value of the literal table."""
    if (direction, op) not in w.want:
        rk, rv = oracle.window_reduce(w.s, w.d, w.v, direction, op)
        share = float(np.mean(~np.isnan(rv)))
        assert share >= 0.75, share
        for name, row in w.table.items():
            i = int(np.searchsorted(rk, w.planted[name]))
            assert rk[i] == w.planted[name]
            assert _same(rv[i], w.dtype(row[1 + {MIN: 0, MAX: 1, SUM: 2}[op]])), (name, op, rv[i])
        i = int(np.searchsorted(rk, w.hub_id))
        hub_want = NAN if w.hub != "none" else {MIN: min, MAX: max, SUM: sum}[op](w.hub_vals)
        assert rk[i] == w.hub_id and _same(rv[i], w.dtype(hub_want)), (w.hub, op, rv[i])
        rk.setflags(write=False)
        rv.setflags(write=False)
        w.want[direction, op] = (rk, rv, share)
    return w.want[direction, op][:2]


def _dev(*arrs):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrs]   # (a copy: the windows are read-only)


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _reduce_matches(eng, oracle, w, direction, op, host=False):
    rk, rv = _want(oracle, w, direction, op)
    gk, gv = eng.reduce(*((w.s, w.d, w.v) if host else _dev(w.s, w.d, w.v)), direction, op)
    t = eng.stage_times()
    assert np.array_equal(_np(gk), rk)
    assert_values(_np(gv), rv, w.dtype, op, exact=True)
    return t


def _fold_matches(eng, oracle, w, direction, op, init):
    _want(oracle, w, direction, op)   # the window's preconditions
    rk, rv = oracle.window_fold(w.s, w.d, w.v, direction, op, init)
    if np.isnan(init):
        assert np.isnan(rv).all()     # Java: NaN + x, Math.min(NaN, x), Math.max(NaN, x) are NaN
    gk, gv = eng.fold(*_dev(w.s, w.d, w.v), direction, op, init)
    t = eng.stage_times()
    assert np.array_equal(_np(gk), rk)
    assert_values(_np(gv), rv, w.dtype, op, exact=True)
    return t


@pytest.fixture(scope="module")
def sort_engine(pkg):
    with pkg.Engine(0, sort_only=True) as e:
        yield e


@pytest.fixture(scope="module")
def onesweep_engine(pkg):
    with pkg.Engine(0, bk_onesweep=True) as e:
        yield e


@pytest.fixture(scope="module")
def chunked(pkg):
    with pkg.Engine(0) as e:
        e.set_max_window_records(20_000)
        yield e


# ---- float MIN / MAX: the sort path ---------------------------------------------------------------------
N_SORT, SPAN_SORT = 60_000, 1 << 12


@pytest.mark.parametrize("hub", HUBS)
@pytest.mark.parametrize("keys", ["k32", "wide", "negative"])
@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("op", [MIN, MAX])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_minmax_sort_path(engine, oracle, dtype, op, direction, keys, hub):
    """A default engine sends float MIN / MAX to the sort path (LDS integer atomics would order negative
    floats, NaN and signed zeros wrongly): java_min / java_max through the fused combine, the look-back
    carry and the merge of straddling partials."""
    w = _window(dtype, op, N_SORT, SPAN_SORT, keys, hub, 11)
    assert w.hub_records > 3 * 4096   # the hub's run crosses RBK_TILE 4096, COMB_TILE 3072, SORT_TILE 8192
    t = _reduce_matches(engine, oracle, w, direction, op)
    assert t.path == 0
    if keys == "wide":
        assert t.key_bytes == 8


@pytest.mark.parametrize("init", [NAN, -0.0, INF, -INF, 0.5])
@pytest.mark.parametrize("op", [MIN, MAX])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_minmax_fold_init(engine, oracle, dtype, op, init):
    w = _window(dtype, op, N_SORT, SPAN_SORT, "k32", "none", 12)
    assert _fold_matches(engine, oracle, w, OUT, op, init).path == 0


# ---- float SUM: the sort path ------------------------------------------------------------------------------
@pytest.mark.parametrize("hub", HUBS)
@pytest.mark.parametrize("keys", ["k32", "wide", "negative"])
@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_sort_path(sort_engine, oracle, dtype, direction, keys, hub):
    w = _window(dtype, SUM, N_SORT, SPAN_SORT, keys, hub, 11)
    assert _reduce_matches(sort_engine, oracle, w, direction, SUM).path == 0


@pytest.mark.parametrize("init", [0.25, -0.0, NAN])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_sort_path_fold_init(sort_engine, oracle, dtype, init):
    w = _window(dtype, SUM, N_SORT, SPAN_SORT, "k32", "none", 12)
    assert _fold_matches(sort_engine, oracle, w, OUT, SUM, init).path == 0


# ---- float SUM: the bucket path ----------------------------------------------------------------------------
# f64 accumulators from the identity -0.0 (BkVal::identity), presence inferred from the accumulator's bits
# (BkVal::present), foldNeighbors' init added as (T)((double)init + a) (BkVal::emit)
BUCKET_SHAPES = {"one_bucket": (1 << 13, False), "direct": (1 << 19, False), "onesweep": (1 << 19, True)}


@pytest.mark.parametrize("hub", HUBS)
@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("shape", list(BUCKET_SHAPES))
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_bucket_path(engine, onesweep_engine, oracle, dtype, shape, direction, hub):
    span, onesweep = BUCKET_SHAPES[shape]
    w = _window(dtype, SUM, 60_000, span, "k32", hub, 13)
    t = _reduce_matches(onesweep_engine if onesweep else engine, oracle, w, direction, SUM)
    assert t.path == (1 if onesweep else 2)


@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_bucket_speculative_window(pkg, oracle, dtype, direction):
    """Two windows of one geometry on one engine: the second takes the speculative partition."""
    with pkg.Engine(0) as e:
        for k, hub in enumerate(("first", "last")):
            w = _window(dtype, SUM, 60_000, 1 << 19, "k32", hub, 20 + k)
            t = _reduce_matches(e, oracle, w, direction, SUM)
            assert t.path == 2 and t.speculative == k


@pytest.mark.parametrize("hub", HUBS)
@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_bucket_multi_item_hub(engine, oracle, dtype, direction, hub):
    """~300,000 records in the hub's bucket: several work items, whose LDS slabs (the hub's partial sums;
    the planted vertices' -0.0, NaN and infinities, which share the bucket) are merged."""
    span = 1 << 20
    w = _window(dtype, SUM, 400_000, span, "k32", hub, 14, hub_frac=0.75)
    assert 280_000 < w.hub_records < 320_000
    t = _reduce_matches(engine, oracle, w, direction, SUM)
    assert t.path in BUCKET and t.partials > span >> 14   # the hub's bucket took several items


@pytest.mark.parametrize("init", [0.25, -0.0, NAN])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_sum_bucket_fold_init(engine, oracle, dtype, init):
    w = _window(dtype, SUM, 60_000, 1 << 19, "k32", "none", 15)
    assert _fold_matches(engine, oracle, w, OUT, SUM, init).path in BUCKET


# ---- the chunked window ----------------------------------------------------------------------------------------
N_CHUNKED = 90_000   # 5 chunks of 20,000 records (OUT), 9 of 10,000 edges (ALL)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("hub", ["first", "last"])
@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("op", [SUM, MIN, MAX])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_chunked(chunked, oracle, dtype, op, direction, hub, host):
    """Each chunk's partials merged into the running partials: a NaN of the first chunk survives every
    merge, one of the last chunk arrives in the last merge; signed zeros and infinities of different
    chunks combine as in one pass."""
    w = _window(dtype, op, N_CHUNKED, SPAN_SORT, "k32", hub, 16)
    _reduce_matches(chunked, oracle, w, direction, op, host=host)


@pytest.mark.parametrize("init", [0.5, NAN])
@pytest.mark.parametrize("op", [SUM, MIN, MAX])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_chunked_fold_init_applied_once(chunked, oracle, dtype, op, init):
    w = _window(dtype, op, N_CHUNKED, SPAN_SORT, "k32", "none", 17)
    _fold_matches(chunked, oracle, w, OUT, op, init)


# ---- partials + merge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", [OUT, ALL])
@pytest.mark.parametrize("op", [SUM, MIN, MAX])
@pytest.mark.parametrize("dtype", FLOATS)
def test_float_partials_then_merge(engine, oracle, dtype, op, direction):
    """The multi-GPU keyBy halves on one GPU: three slices of the window -> partials grouped by 3 owners,
    each owner's rows merged; the owners' rows together are the whole window's."""
    w = _window(dtype, op, N_SORT, SPAN_SORT, "k32", "first", 18)
    rk, rv = _want(oracle, w, direction, op)
    nparts, third = 3, N_SORT // 3
    rows = [[] for _ in range(nparts)]
    for j in range(3):
        sl = slice(j * third, (j + 1) * third)
        k, p, counts = engine.reduce_partials(*_dev(w.s[sl], w.d[sl], w.v[sl]), direction, op, nparts)
        bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        assert bounds[-1] == len(k)
        for o in range(nparts):
            rows[o].append((k[bounds[o]:bounds[o + 1]].clone(), p[bounds[o]:bounds[o + 1]].clone()))
    gk, gv = [], []
    for o in range(nparts):
        mk, mv = engine.merge_partials(torch.cat([r[0] for r in rows[o]]), torch.cat([r[1] for r in rows[o]]), op)
        assert all(engine.owner_of(int(x), nparts) == o for x in _np(mk)[:50])
        gk.append(_np(mk))
        gv.append(_np(mv))
    gk, gv = np.concatenate(gk), np.concatenate(gv)
    order = np.argsort(gk, kind="stable")
    assert np.array_equal(gk[order], rk)
    assert_values(gv[order], rv, dtype, op, exact=True)


# ---- integer extremes on the bucket path ----------------------------------------------------------------------
def _int_planted(dtype, op):
    """name -> (values, the op's result): the LDS identity of the op as a value (BkVal::identity: MAX_INT
    under MIN, MIN_INT under MAX, 0 under SUM), alone and mixed with narrow (packed) values"""
    lo, hi = int(np.iinfo(dtype).min), int(np.iinfo(dtype).max)
    if op == MIN:
        return {"identity_only": ([hi] * 3, hi), "identity_single": ([hi], hi), "identity_and_narrow": ([hi, 7, hi], 7),
                "narrow_then_identity": ([9, hi], 9), "other_extreme": ([lo, 5], lo), "both": ([hi, lo, hi], lo)}
    if op == MAX:
        return {"identity_only": ([lo] * 3, lo), "identity_single": ([lo], lo), "identity_and_narrow": ([lo, 7, lo], 7),
                "narrow_then_identity": ([9, lo], 9), "other_extreme": ([hi, 5], hi), "both": ([lo, hi, lo], hi)}
    return {"min_plus_min": ([lo, lo], 0), "max_plus_1": ([hi, 1], lo), "max_max_2": ([hi, hi, 2], 0),
            "cancel": ([-5, 5], 0), "narrow_cancel": ([3, 4, -7], 0), "zeros": ([0, 0], 0), "zero_single": ([0], 0),
            "min_single": ([lo], lo), "minus_one_plus_one": ([-1, 1], 0)}


@functools.lru_cache(maxsize=None)
def _int_window(dtype, op, seed, n=200_000, span=1 << 20):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    table = _int_planted(dtype, op)
    first = span // 3
    ids = {name: first + j for j, name in enumerate(table)}
    ordinary = np.setdiff1d(np.arange(span), list(ids.values()))
    s = ordinary[rng.integers(0, len(ordinary), n)].astype(np.int64)
    d = ordinary[rng.integers(0, len(ordinary), n)].astype(np.int64)
    v = rng.integers(0, 0xFFFF, n).astype(dtype)                 # narrow: travel packed
    rare = rng.random(n) < 0.002                                  # extremes among common records (escaped)
    v[rare] = rng.choice(np.array([info.min, info.max], dtype), int(rare.sum()))
    pos = rng.permutation(rng.choice(n, sum(len(t[0]) for t in table.values()), replace=False))
    at = 0
    for name, (vals, _) in table.items():
        p = np.sort(pos[at:at + len(vals)])
        at += len(vals)
        s[p], v[p] = ids[name], np.array(vals, dtype)
    for a in (s, d, v):
        a.setflags(write=False)
    return SimpleNamespace(s=s, d=d, v=v, ids=ids, table=table, n=n)


@pytest.mark.parametrize("op", [SUM, MIN, MAX])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_integer_extremes_bucket_path(pkg, oracle, dtype, op):
    """The packed path infers a vertex's presence from an accumulator that left its identity, unless a
    value escaped (BkVal::add_packed, INFER_PRESENCE): vertices seen only through the identity itself, or
    whose sum wraps back to 0, must still be emitted, with the reference's value.  Packed, unpacked and
    histogram-only engines; a second window (speculative on the first two); folds from both extremes."""
    info = np.iinfo(dtype)
    with pkg.Engine(0) as ep, pkg.Engine(0, no_pack=True) as eu, pkg.Engine(0, no_spec=True) as eh:
        for k in range(2):
            w = _int_window(dtype, op, 30 + k)
            rk, rv = oracle.window_reduce(w.s, w.d, w.v, OUT, op)
            for name, (_, want) in w.table.items():   # the oracle holds the literal table
                i = int(np.searchsorted(rk, w.ids[name]))
                assert rk[i] == w.ids[name] and int(rv[i]) == want, (name, rv[i], want)
            got = []
            for e in (ep, eu, eh):
                gk, gv = e.reduce(*_dev(w.s, w.d, w.v), OUT, op)
                assert np.array_equal(_np(gk), rk)
                assert_values(_np(gv), rv, dtype, op)
                got.append((gk, gv, e.stage_times()))
            tp, tu, th = (g[2] for g in got)
            assert tp.path == tu.path == th.path == 2
            assert tp.packed and 0 < tp.escapes < w.n // 8 and not tu.packed
            assert (tp.speculative, tu.speculative, th.speculative) == (k, k, 0)
            for gk, gv, _ in got[1:]:
                assert torch.equal(gk, got[0][0]) and torch.equal(gv, got[0][1])
        for init in (int(info.min), int(info.max)):
            rk, rv = oracle.window_fold(w.s, w.d, w.v, OUT, op, init)
            for e in (ep, eu, eh):
                gk, gv = e.fold(*_dev(w.s, w.d, w.v), OUT, op, init)
                assert e.stage_times().path == 2
                assert np.array_equal(_np(gk), rk)
                assert_values(_np(gv), rv, dtype, op)
