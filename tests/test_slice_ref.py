"""CPU: the model of the batched slice call (tests/slice_ref.py) and the routing rule (stream.plan_slice).

The composite key must order records as (window, vertex, arrival) under a stable sort, round-trip every int64 vertex
and timestamp the 64 bits hold, and refuse exactly from 65 bits on; the model's windows must be the reference's own
TestSlice results when its graph is replayed into three windows."""
import json
from pathlib import Path

import numpy as np
import pytest

import slice_ref as S

FIX = json.loads((Path(__file__).parent / "golden" / "reference_fixtures.json").read_text())
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DIRS = {"IN": 0, "OUT": 1, "ALL": 2}


def test_window_start_is_the_oracles(oracle):
    rng = np.random.default_rng(11)
    ts = np.concatenate([rng.integers(-10**6, 10**6, 2000), rng.integers(I64_MIN, I64_MAX, 2000, dtype=np.int64),
                         np.array([I64_MIN + 1, I64_MAX, -1, 0, 1, -1000, 1000, -999, 999])]).astype(np.int64)
    for size in (1, 7, 1000, 1 << 31, 1 << 62, I64_MAX):
        assert np.array_equal(S.window_start(ts, size), oracle.window_start(ts, size)), size
    # every ts in (-size, size) shares window 0
    assert set(S.window_start(np.arange(-999, 1000), 1000)) == {0}


def _round_trip(src, dst, ts, size, direction):
    g = S.geometry(src, dst, ts, size, direction)
    v, t = S.expand(src, dst, ts, direction)
    keys = S.pack(g, v, t)
    assert S.unpack(g, keys) == list(zip(S.window_start(t, size).tolist(), v.tolist()))
    # a stable sort of the keys is the (window, vertex, arrival) order
    order = sorted(range(len(keys)), key=keys.__getitem__)
    want = np.lexsort((np.arange(len(v)), v, S.window_start(t, size)))
    assert order == want.tolist()
    assert max(keys) < 1 << max(g.wbits + g.vbits, 1)
    return g


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_pack_round_trips_random_columns(direction):
    rng = np.random.default_rng(5 + direction)
    n = 3000
    src = rng.integers(-50_000, 50_000, n)
    dst = rng.integers(-50_000, 50_000, n)
    ts = rng.integers(-40_000, 90_000, n)    # out of order, both signs, the window that straddles zero
    g = _round_trip(src, dst, ts, 1000, direction)
    assert g.vbits == 17 and g.wbits == 8


def test_pack_round_trips_extremes():
    # the full vertex range leaves no window bits: one window
    g = _round_trip([I64_MIN, I64_MAX, 0, -1], [0, 0, 0, 0], [5, 6, 7, 8], 1000, S.DIR_OUT)
    assert (g.wbits, g.vbits) == (0, 64)
    # the full timestamp range in windows of 2^62: starts -2^62 .. 2^62, a span no int64 difference holds
    g = _round_trip([3, 3, 4, 3], [0, 0, 0, 0], [I64_MIN + 1, I64_MAX, 0, -1], 1 << 62, S.DIR_OUT)
    assert (g.start_min, g.wbits, g.vbits) == (-(1 << 62), 2, 1)
    # window size 1 over the full range: 64 window bits, one vertex
    g = _round_trip([9, 9], [1, 2], [I64_MIN + 1, I64_MAX], 1, S.DIR_OUT)
    assert (g.wbits, g.vbits) == (64, 0)
    # ALL: the span covers both columns
    g = _round_trip([0, 1], [I64_MAX, 2], [0, 0], 10, S.DIR_ALL)
    assert g.vbits == 63


def test_the_64_65_bit_boundary():
    size = 1000
    ts = [0, ((1 << 24) - 1) * size]
    g = _round_trip([0, (1 << 40) - 1], [0, 0], ts, size, S.DIR_OUT)
    assert (g.wbits, g.vbits) == (24, 40)
    with pytest.raises(S.Refused, match="24 window bits \\+ 41 vertex bits"):
        S.geometry([0, 1 << 40], [0, 0], ts, size, S.DIR_OUT)
    # the wide column is not a key column under IN: accepted
    assert S.geometry([0, 1 << 40], [0, 0], ts, size, S.DIR_IN).vbits == 0
    # 64 window bits leave room for one vertex only
    assert S.geometry([0, 0], [0, 0], [I64_MIN + 1, I64_MAX], 1, S.DIR_ALL).wbits == 64
    with pytest.raises(S.Refused, match="64 window bits \\+ 1 vertex bits"):
        S.geometry([0, 1], [0, 0], [I64_MIN + 1, I64_MAX], 1, S.DIR_OUT)


# ---- routing ---------------------------------------------------------------------------------------------------
def test_plan_slice_routes(pkg):
    L = pkg._lib
    plan, X = pkg.plan_slice, 1000   # an explicit crossover: the rule, whatever constant was measured
    I64, F32, F64, NONE = L.GS_I64, L.GS_F32, L.GS_F64, L.GS_NONE
    SUM, MIN, MAX, COUNT = L.GS_OP_SUM, L.GS_OP_MIN, L.GS_OP_MAX, L.GS_OP_COUNT

    def auto(kind, op, dt, has_ts=True, records=10_000, windows=100):
        return plan("auto", kind, op, dt, has_ts, records, windows, crossover=X)

    # small windows, bit-stable ops: batched
    for kind, op, dt in (("reduce", SUM, I64), ("reduce", SUM, L.GS_I32), ("reduce", COUNT, NONE), ("reduce", MIN, F32),
                         ("reduce", MAX, F64), ("fold", MIN, F64), ("fold", SUM, I64), ("degree_max", -2, NONE)):
        p = auto(kind, op, dt)
        assert p.batched and p.windows == 100, (kind, op, dt, p)
    # float SUM under "auto" takes the loop, reduce and fold alike; under True it goes batched
    for kind in ("reduce", "fold"):
        for dt in (F32, F64):
            assert not auto(kind, SUM, dt).batched
            assert plan(True, kind, SUM, dt, True, 10_000, 100, crossover=X).batched
    # a single window, no timestamps, user functions, too many records: the loop, under every mode
    for mode in ("auto", True):
        assert not plan(mode, "reduce", SUM, I64, True, 10_000, 1, crossover=X).batched
        assert not plan(mode, "reduce", SUM, I64, False, 10_000, 100, crossover=X).batched
        assert not plan(mode, "user", -1, I64, True, 10_000, 100, crossover=X).batched
        assert not plan(mode, "reduce", SUM, I64, True, 1 << 32, 100, crossover=X).batched
        assert plan(mode, "reduce", SUM, I64, True, (1 << 32) - 1, 1 << 30, crossover=X).batched
    # the crossover: mean records per window strictly below it
    assert auto("reduce", SUM, I64, records=99_999, windows=100).batched
    assert not auto("reduce", SUM, I64, records=100_000, windows=100).batched
    assert plan(True, "reduce", SUM, I64, True, 100_000, 100, crossover=X).batched    # True ignores it
    assert not plan("auto", "reduce", SUM, I64, True, 10, 100, crossover=0).batched   # batched never won: nothing
    # off
    assert not plan(False, "reduce", SUM, I64, True, 10_000, 100, crossover=X).batched
    # the default crossover is the module's constant
    assert plan("auto", "reduce", SUM, I64, True, 200, 100).batched == (2 < pkg.stream.SLICE_CROSSOVER)


def test_window_span_and_setting(pkg):
    assert pkg.window_span(0, 999, 1000) == 1
    assert pkg.window_span(-999, 999, 1000) == 1
    assert pkg.window_span(-1000, 1000, 1000) == 3
    assert pkg.window_span(I64_MIN + 1, I64_MAX, 1 << 62) == 3
    env = pkg.StreamExecutionEnvironment()
    assert env.getSliceBatching() == "auto"
    assert env.setSliceBatching(True).getSliceBatching() is True
    assert env.setSliceBatching(False).getSliceBatching() is False
    assert env.setSliceBatching("auto").getSliceBatching() == "auto"
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError):
            env.setSliceBatching(bad)


# ---- the reference's TestSlice goldens, three windows ----------------------------------------------------------
@pytest.mark.parametrize("case", FIX["slice_cases"], ids=lambda c: c["name"])
def test_testslice_goldens_in_three_windows(oracle, case):
    e = np.array(FIX["slice_graph"]["edges"], dtype=np.int64)
    size, n = FIX["slice_graph"]["window_ms"], len(e)
    # the 7 edges at ts, ts + 1000 and ts + 2000, the three replays interleaved (arrival order kept inside each)
    rep = np.tile(np.arange(3), n)
    src, dst, val = (np.repeat(e[:, c], 3) for c in range(3))
    ts = 17 + 1000 * rep
    direction = DIRS[case["direction"]]
    if case["kind"] == "fold":       # SumEdgeValues from Tuple2(0, 0)
        ws, rb, k, r = S.sliced(oracle.window_fold, src, dst, val, ts, size, direction, oracle.OP_SUM, 0)
    else:                            # SumEdgeValuesReduce; SumEdgeValuesApply: sum > 50 ? big : small
        ws, rb, k, r = S.sliced(oracle.window_reduce, src, dst, val, ts, size, direction, oracle.OP_SUM)
    assert ws.tolist() == [0, 1000, 2000] and len(rb) == 4 and rb[0] == 0 and rb[3] == len(k)
    want = {tuple(x) for x in case["expected"]}
    for w in range(3):
        lo, hi = int(rb[w]), int(rb[w + 1])
        assert np.all(np.diff(k[lo:hi]) > 0)
        if case["kind"] == "apply":
            got = {(str(a), "big" if b > 50 else "small") for a, b in zip(k[lo:hi], r[lo:hi])}
        else:
            got = {(str(a), str(b)) for a, b in zip(k[lo:hi], r[lo:hi])}
        assert got == want, w
