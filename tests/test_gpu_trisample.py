"""GPU: the sampling triangle estimators (gs_trisample_*) against the edge-by-edge restatement of
tests/trisample_ref.py, driven by the same counter-based draws: exact and ordered equality of the emitted
TriangleEstimate records and of the exported sampler rows.  The samplers live on the device across calls, so
most tests cut one stream into batches in several ways and demand the same output."""
import ctypes
import functools
import math
import random

import numpy as np
import pytest
import torch

import trisample_ref as ref

pytestmark = pytest.mark.gpu
MODES = ["broadcast", "incidence"]
TILE = 2048   # GS_TRISAMPLE_TILE: edges per tile of the streaming pass (checked against the library below)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _cuts(n, sizes):
    """[(a, b)] covering [0, n): batches of the given sizes, the last size repeating"""
    out, a, i = [], 0, 0
    while a < n:
        b = min(n, a + sizes[min(i, len(sizes) - 1)])
        out.append((a, b))
        a, i = b, i + 1
    return out


def _at(n, positions):
    """[(a, b)] covering [0, n), cut after the given stream positions"""
    edges = sorted({p for p in positions if 0 < p < n} | {0, n})
    return list(zip(edges, edges[1:]))


def _feed(state, src, dst, cuts, dev=True):
    """the stream through `state` in the given batches: the records it emits"""
    S, D = (torch.tensor(src).cuda(), torch.tensor(dst).cuda()) if dev else (src, dst)
    out = []
    for a, b in cuts:
        k, v = state.edges(S[a:b], D[a:b])
        out.extend(zip(_np(k).tolist(), _np(v).tolist()))
    return out


@functools.lru_cache(maxsize=None)
def _want(mode, S, V, seed, stream, first=0, upto=None):
    """the restatement over the named stream: (records, rows, beta sum, last emitted, trace)"""
    src, dst = _stream(stream)
    st = ref.TriangleSamplerRef(mode, S, V, seed=seed, first_sampler=first, trace=True)
    rec = st.edges(src[:upto], dst[:upto])
    rows = st.rows()
    rows.setflags(write=False)
    return rec, rows, st.beta_sum(), st.previous, tuple(st.trace)


def _check(engine, mode, S, V, seed, stream, cuts, dev=True, first=0):
    src, dst = _stream(stream)
    rec, rows, beta, prev, _ = _want(mode, S, V, seed, stream, first)
    with engine.triangle_sampler(mode, S, V, seed, first_sampler=first) as st:
        got = _feed(st, src, dst, cuts, dev)
        hdr, grows = st.export()
        assert got == rec
        assert np.array_equal(grows, rows)
        assert st.size() == (len(src), beta)
        assert (hdr["edges_seen"], hdr["beta_sum"], hdr["last_emitted"]) == (len(src), beta, prev)


@functools.lru_cache(maxsize=None)
def _stream(name):
    rng = np.random.default_rng(0x7A1)
    if name == "default":      # BroadcastTriangleCount.java:257-264
        k = np.arange(1000)
        s = np.repeat(k, 2)
        d = np.stack([(k + 2) % 1000, (k + 4) % 1000], axis=1).ravel()
    elif name == "k12":
        edges = [(a, b) for a in range(12) for b in range(a + 1, 12)]
        random.Random(12).shuffle(edges)
        s, d = np.array([e[0] for e in edges]), np.array([e[1] for e in edges])
    elif name == "dense30":    # 600 random edges over 30 vertices: wedges close all the time
        s, d = rng.integers(0, 30, 600), rng.integers(0, 30, 600)
    elif name.startswith("len"):   # 40 vertices, a given length
        n = int(name[3:])
        s, d = rng.integers(0, 40, n), rng.integers(0, 40, n)
    elif name == "cut5000":
        s, d = rng.integers(0, 60, 5000), rng.integers(0, 60, 5000)
    elif name == "v5":         # 5 vertices: both orientations, repeats and self-loops of everything
        s, d = rng.integers(0, 5, 400), rng.integers(0, 5, 400)
    elif name == "ids":        # endpoints far outside [0, vertex_count) among a few inside it
        pal = np.array([-1, -5, 0, 1, 2, 3, 4, 5, (1 << 32) + 3, 1 << 40, I64_MIN, I64_MAX, -1, 2, 3], dtype=np.int64)
        s, d = pal[rng.integers(0, len(pal), 900)], pal[rng.integers(0, len(pal), 900)]
    elif name == "rmat":       # 2^17 edges of R-MAT scale 10
        import __graft_entry__ as ge
        s, d = ge.load_oracle().gen_rmat(10, 1 << 17, 0x5EED75)
    s, d = np.ascontiguousarray(s, dtype=np.int64), np.ascontiguousarray(d, dtype=np.int64)
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


def test_tile_constant(pkg):
    from gelly_streaming_amd import _lib
    assert _lib.GS_TRISAMPLE_TILE == TILE == pkg.TriangleSamplerState.TILE


# ---- the reference's own default ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_reference_default_stream(engine, mode):
    """vertex count 1000, 10 000 samplers (:216-217) over the built-in edges"""
    rec = _want(mode, 10_000, 1000, 0xDEF, "default")[0]
    assert len(rec) > 5                     # the ring of k -> k+2, k -> k+4 holds triangles (k, k+2, k+4)
    _check(engine, mode, 10_000, 1000, 0xDEF, "default", [(0, 2000)])
    _check(engine, mode, 10_000, 1000, 0xDEF, "default", _cuts(2000, [333]), dev=False)


@pytest.mark.parametrize("samples", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("mode", MODES)
def test_sampler_counts(engine, mode, samples):
    _check(engine, mode, samples, 30, 41, "dense30", _cuts(600, [250]))


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
@pytest.mark.parametrize("mode", MODES)
def test_batch_lengths_around_the_tile(engine, mode, n):
    """one batch of n edges through 16-byte loads, then the same stream with its first edge cut off, which
    leaves the rest on an 8-byte boundary (the scalar-load variant of the pass)"""
    assert len(_want(mode, 64, 40, 7, f"len{n}")[0]) > 20
    _check(engine, mode, 64, 40, 7, f"len{n}", [(0, n)])
    _check(engine, mode, 64, 40, 7, f"len{n}", [(0, 1), (1, n)])


# ---- batch cuts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_output_does_not_depend_on_the_batch_cut(engine, mode):
    n = 5000
    _check(engine, mode, 200, 60, 99, "cut5000", [(0, n)])
    _check(engine, mode, 200, 60, 99, "cut5000", [(i, i + 1) for i in range(70)] + [(70, n)])
    _check(engine, mode, 200, 60, 99, "cut5000", _cuts(n, [7, 64, 1000, n]))
    _check(engine, mode, 200, 60, 99, "cut5000", _cuts(n, [1000]), dev=False)


@pytest.mark.parametrize("mode", MODES)
def test_carried_flags_and_a_cut_at_a_replacement(engine, mode):
    """a cut between a wedge's two closing edges (one found flag crosses it and the find comes after it), a cut
    right after a replacement's edge and one right before it"""
    trace = _want(mode, 200, 60, 99, "cut5000")[4]
    flags = {}
    between = None
    for what, k, i in trace:
        if what in ("replace", "reset"):
            flags.pop(i, None)
        elif what == "flag":
            flags.setdefault(i, k)
        elif what == "find" and i in flags and flags[i] < k and between is None and k > 200:
            between = (flags[i], k)      # first flag at flags[i], the find at k, same epoch
    assert between is not None
    cut_wedge = between[0]               # the batch ends with the first closing edge
    assert between[0] <= cut_wedge < between[1]
    repl = [k for what, k, i in trace if what in ("replace", "reset") and 300 < k < 4000]
    assert len(repl) >= 2
    _check(engine, mode, 200, 60, 99, "cut5000", _at(5000, [cut_wedge, repl[0], repl[1] - 1]))


@pytest.mark.parametrize("mode", MODES)
def test_shared_wanted_pairs(engine, mode):
    """vertex_count 5 and 1000 samplers: every wanted pair is wanted hundreds of times (one table slot, a long
    chain); the stream closes wedges in both orientations, again and again, between self-loops"""
    s, d = _stream("v5")
    assert np.any(s == d) and len({(a, b) for a, b in zip(s.tolist(), d.tolist())}) == 25
    rec, rows, beta, _, _ = _want(mode, 1000, 5, 3, "v5")
    assert beta > 100 and len(rec) > 100
    _check(engine, mode, 1000, 5, 3, "v5", _cuts(400, [150]))
    _check(engine, mode, 1000, 5, 3, "v5", [(0, 400)])


@pytest.mark.parametrize("mode", MODES)
def test_any_int64_is_an_endpoint(engine, mode):
    rec, rows, beta, _, _ = _want(mode, 500, 6, 17, "ids")
    assert len(rec) > 10                                           # triangles among the ids inside [0, 6) still close
    held = set(rows[:, 0].tolist()) | set(rows[:, 1].tolist())
    assert {-1, I64_MIN, I64_MAX, 1 << 40, (1 << 32) + 3} <= held    # and the odd ids are held as endpoints
    _check(engine, mode, 500, 6, 17, "ids", _cuts(900, [400]))


def test_a_find_and_a_reset_at_one_position_cancel(engine):
    """+1 and -1 at one position: Broadcast's sum does not change there, so it emits nothing; Incidence reports
    the find's own view"""
    hit = None
    for seed in range(300):
        b = _want("broadcast", 48, 12, seed, "k12")
        by_pos = {}
        for what, k, i in b[4]:
            by_pos.setdefault(k, []).append(what)
        for k, evs in by_pos.items():
            if evs.count("find") == 1 and evs.count("reset") == 1:
                inc = _want("incidence", 48, 12, seed, "k12")[0]
                if any(r[0] == k for r in inc) and not any(r[0] == k for r in b[0]):
                    hit = (seed, k)
                    break
        if hit:
            break
    assert hit, "no seed below 300 builds the case"
    seed, k = hit
    for cuts in ([(0, 66)], _at(66, [k - 1, k])):
        _check(engine, "broadcast", 48, 12, seed, "k12", cuts)
        _check(engine, "incidence", 48, 12, seed, "k12", cuts)


@pytest.mark.parametrize("mode", MODES)
def test_many_tiles_and_blocks(engine, mode):
    n = 1 << 17
    assert len(_want(mode, 64, 1024, 5, "rmat")[0]) > 3
    _check(engine, mode, 64, 1024, 5, "rmat", [(0, n)])


# ---- several states, one summer ------------------------------------------------------------------------------
def _steps(parts, n):
    """the global beta sum after every edge count at which it changes, from the subtasks' Broadcast records"""
    change = {}
    for q, rec in enumerate(parts):
        for k, b in rec:
            change.setdefault(k, {})[q] = b
    cur, total, out = [0] * len(parts), 0, []
    for k in sorted(change):
        for q, b in change[k].items():
            cur[q] = b
        if sum(cur) != total:
            total = sum(cur)
            out.append((k, total))
    return out


def test_disjoint_sampler_groups_equal_one_state(pkg, engine):
    """Two states of 500 samplers (ids 0.. and 500..) against one of 1000, Broadcast.  A subtask's record at
    edge count k carries its sum after edge k, so merged by (edge count, source) -- the order
    triangle_estimate.merge_estimates documents -- the summer's global sum after each edge count's records is
    the one state's sum; its records are compared as that step function, because a +1 in one group and a -1
    in the other at one edge count give the two-group summer a record (maxEdges moves) where one state has
    none.  Incidence sums are taken mid-edge in sampler order and do not split over groups."""
    from gelly_streaming_amd import triangle_estimate as te
    src, dst = _stream("dense30")
    parts = []
    for first in (0, 500):
        with engine.triangle_sampler("broadcast", 500, 30, 77, first_sampler=first) as st:
            parts.append(_feed(st, src, dst, _cuts(600, [256])))
        assert parts[-1] == _want("broadcast", 500, 30, 77, "dense30", first)[0]
    one = _want("broadcast", 1000, 30, 77, "dense30")[0]
    assert _steps(parts, 600) == one
    # and through the package's summer: after the last record the estimate is the one state's
    merged = te.merge_estimates([(q, [k for k, _ in p], [b for _, b in p]) for q, p in enumerate(parts)])
    two, single = pkg.TriangleSummer(1000, 30), pkg.TriangleSummer(1000, 30)
    out2, out1 = [], []
    for q, k, b in merged:
        two.flatMap(q, k, b, out2)
    for k, b in one:
        single.flatMap(0, k, b, out1)
    assert sum(b for _, b in two.results.values()) == one[-1][1]
    if two.maxEdges == single.maxEdges:
        assert out2[-1] == out1[-1]


# ---- checkpoint --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_checkpoint_in_mid_stream(pkg, engine, mode):
    src, dst = _stream("cut5000")
    rec, rows, beta, prev, _ = _want(mode, 200, 60, 99, "cut5000")
    with engine.triangle_sampler(mode, 200, 60, 99) as a:
        head = _feed(a, src, dst, [(0, 1777)])
        hdr, ck = a.export()
        assert np.array_equal(ck, _want(mode, 200, 60, 99, "cut5000", 0, 1777)[1])
        with engine.triangle_sampler(mode, 200, 60, 99) as b:
            b.load(hdr, ck)
            assert b.size() == a.size()
            k, v = b.edges(torch.tensor(src[1777:]).cuda(), torch.tensor(dst[1777:]).cuda())
            assert head + list(zip(_np(k).tolist(), _np(v).tolist())) == rec
            assert np.array_equal(b.export()[1], rows)
            with pytest.raises(pkg.GsError) as e:      # not fresh any more
                b.load(hdr, ck)
            assert e.value.status == -1
        for other in (dict(seed=98), dict(samples=100), dict(vertex_count=61), dict(first_sampler=1),
                      dict(mode="incidence" if mode == "broadcast" else "broadcast")):
            kw = dict(mode=mode, samples=200, vertex_count=60, seed=99, first_sampler=0)
            kw.update(other)
            with engine.triangle_sampler(**kw) as c:
                with pytest.raises(pkg.GsError) as e:
                    c.load(hdr, ck[:kw["samples"]])
                assert e.value.status == -1 and c.size() == (0, 0)
        bad = ck.copy()
        bad[3, 3] = 3          # both found flags without beta: no run leaves that
        with engine.triangle_sampler(mode, 200, 60, 99) as c:
            with pytest.raises(pkg.GsError) as e:
                c.load(hdr, bad)
            assert e.value.status == -1 and c.size() == (0, 0)


# ---- errors --------------------------------------------------------------------------------------------------------
def test_errors_leave_the_state_unchanged(pkg, engine):
    from gelly_streaming_amd import _lib
    for kw in (dict(vertex_count=2), dict(samples=0), dict(samples=1 << 31)):
        args = dict(mode="broadcast", samples=10, vertex_count=100)
        args.update(kw)
        with pytest.raises(pkg.GsError) as e:
            engine.triangle_sampler(**args)
        assert e.value.status == _lib.GS_EINVAL
    src, dst = _stream("dense30")
    rec = _want("broadcast", 300, 30, 8, "dense30")[0]
    with engine.triangle_sampler("broadcast", 300, 30, 8) as st:
        head = _feed(st, src, dst, [(0, 200)])
        size, (hdr, rows) = st.size(), st.export()

        def unchanged():
            h2, r2 = st.export()
            return st.size() == size and h2 == hdr and np.array_equal(r2, rows)
        # a batch that would take the stream past 2^31 - 1 edges: the length is fabricated, no column is read
        n_out = ctypes.c_uint64(0)
        keys, vals = np.zeros(8, np.int64), np.zeros(8, np.int64)
        vo = _lib.GsVertexOut(keys.ctypes.data, vals.ctypes.data, 8, ctypes.pointer(n_out), _lib.GS_MEM_HOST, 0)
        b = _lib.GsEdgeBatch(src.ctypes.data, dst.ctypes.data, None, (1 << 31) - 1 - 199, _lib.GS_NONE, _lib.GS_MEM_HOST, 0)
        assert engine._L.gs_trisample_edges(engine.ctx, st.handle, ctypes.byref(b), ctypes.byref(vo)) == _lib.GS_EINVAL
        assert unchanged()
        # capacity too small: the number needed, and nothing else happened
        tail = [r for r in rec if r[0] > 200]
        assert len(tail) > 4
        with pytest.raises(pkg.GsError) as e:
            st.edges(src[200:], dst[200:], capacity=3)
        assert e.value.status == _lib.GS_ECAPACITY and unchanged()
        vo.capacity = 3
        b.n = 400
        b.src, b.dst = src[200:].ctypes.data, dst[200:].ctypes.data
        assert engine._L.gs_trisample_edges(engine.ctx, st.handle, ctypes.byref(b), ctypes.byref(vo)) == _lib.GS_ECAPACITY
        assert n_out.value == len(tail) and unchanged()
        # without columns the batch only updates the state and reports the number
        assert st.advance(src[200:], dst[200:]) == len(tail)
        assert st.size() == (600, _want("broadcast", 300, 30, 8, "dense30")[2])
        assert np.array_equal(st.export()[1], _want("broadcast", 300, 30, 8, "dense30")[1])
        assert head == [r for r in rec if r[0] <= 200]


# ---- end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("micro_batch", [None, 7])
def test_broadcast_triangle_count_end_to_end(pkg, engine, micro_batch):
    """K12 shuffled: E = 66, V = 12; the exact count comes from gs_window_triangles.  A sampler ends with beta =
    1 with p = T / (E (V - 2)), so the last estimate, sum * E (V - 2) / S, lies within 5 sigma of T scaled the
    same way (and one more for the (int) cast)."""
    S, V = 4096, 12
    src, dst = _stream("k12")
    exact = engine.triangles(src, dst)[0]
    assert exact == 220
    env = pkg.StreamExecutionEnvironment.getExecutionEnvironment()
    env.setMicroBatch(micro_batch)
    try:
        g = pkg.SimpleEdgeStream(pkg.EdgeColumns(src, dst), env)
        out = pkg.broadcast_triangle_count(g, V, S, seed=0x7E57).collect()
        inc = pkg.incidence_sampling_triangle_count(g, V, S, seed=0x7E57).collect()
    finally:
        env.setMicroBatch(None)
    E = len(src)
    p = exact / (E * (V - 2))
    bound = 5 * math.sqrt(S * p * (1 - p)) * E * (V - 2) / S + 1
    assert out[-1][0] <= E and abs(out[-1][1] - exact) <= bound, out[-1]
    rs = ref.TriangleSummerRef(S, V)
    assert out == rs.feed(0, _want("broadcast", S, V, 0x7E57, "k12")[0])
    rs = ref.TriangleSummerRef(S, V)
    assert inc == rs.feed(0, _want("incidence", S, V, 0x7E57, "k12")[0])
