"""GPU: every window operator under the order-preserving id maps of tests/idmaps.py.

Each operator measures its window's id range and picks a path from it -- direct tables indexed by id ^ key_xor up
to 28 mask bits, relabel_endpoints above (32-bit sort keys up to 32 mask bits, 64-bit beyond), packed stage-2 keys
below a span of 2^32, u32 candidate chunks up to a span of 2^32 - 1 -- and undoes the transform on the way out.  A
map moves a small graph onto one of these paths and changes nothing else; the reference is always the CPU oracle
(or tests/bipartite_cpu.py canonical) run on the mapped ids, compared for exact equality, and every union-find and
triangles case asserts through the stage times that it ran the path its map is named for.

Every graph holds base ids 0 and 2^K - 1 (idmaps.pin_ends).  The spread_2p28 cases of union-find and triangles
(tables of 2^28 entries) run on engines of their own at the end of the file."""
import functools

import numpy as np
import pytest
import torch
from bipartite_cpu import canonical
from idmaps import NAMES, id_span, mask_bits, maps, pin_ends

pytestmark = pytest.mark.gpu

TABLE_MAPS = [n for n in NAMES if n != "spread_2p28"]   # (union-find, triangles: 2^28 ids on their own engines)


def _oracle():
    import __graft_entry__ as ge
    return ge.load_oracle()


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dev(*cols):
    return tuple(torch.from_numpy(np.array(c)).cuda() for c in cols)   # a copy: the shared graphs are read-only


def _both(*cols):
    """the columns as device tensors, then as host arrays"""
    yield _dev(*cols)
    yield tuple(np.array(c) for c in cols)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _same_cc(got, want):
    assert len(got) == 2
    for g, w in zip(got, want):
        g = _np(g)
        assert g.dtype == w.dtype and np.array_equal(g, w)


def _same_bip(got, want):
    assert bool(got[0]) == bool(want[0])
    for g, w in zip(got[1:], want[1:]):
        g = _np(g)
        assert g.dtype == w.dtype and np.array_equal(g, w)


def _failed(got):
    assert got[0] is False and all(len(x) == 0 for x in got[1:])


def _uf_path(engine, path, bits, records):
    """The union-find driver reports its table width on the direct path and 0 on the relabel path."""
    t = engine.stage_times()
    assert (t.path, t.records) == (path, records)
    assert t.key_bits == (max(bits, 1) if bits <= 28 else 0)


# ---- the graphs (base ids; read-only, shared) -----------------------------------------------------------
UF_GRAPHS = {"s12": (12, 5_000, 0x5EED33), "s16": (16, 300_000, 0x5EED34)}   # one pass / two-phase (>= 65536 records)


@functools.lru_cache(maxsize=None)
def _cc_graph(size):
    K, n, seed = UF_GRAPHS[size]
    return _frozen(*pin_ends(*_oracle().gen_rmat(K, n, seed), K)) + (K,)


@functools.lru_cache(maxsize=None)
def _bip_graph(size):
    """R-MAT made bipartite as in test_gpu_bipartite.py (2x, 2x + 1: base ids in [0, 2^(K + 1))) and its
    canonical state in base ids (only to choose a bad edge from)"""
    K, n, seed = UF_GRAPHS[size]
    s, d = _oracle().gen_rmat(K, n, seed)
    s, d = pin_ends(s * 2, d * 2 + 1, K + 1)
    want = canonical(s, d)
    assert want[0]
    _frozen(s, d, *want[1:])
    return s, d, K + 1, want


@functools.lru_cache(maxsize=None)
def _tri_graph():
    s, d = pin_ends(*_oracle().gen_rmat(12, 40_000, 0x5EED32, no_self_loops=True), 12)
    assert not np.any(s == d)
    return _frozen(s, d) + (12,)


@functools.lru_cache(maxsize=None)
def _loop_graph():
    """R-MAT s10 with its self-loops: the self-pair term follows the JDK HashSet order of the mapped Longs, so
    the count differs from map to map"""
    s, d = pin_ends(*_oracle().gen_rmat(10, 3_000, 0x5EED31), 10)
    assert int(np.sum(s == d)) == 22
    return _frozen(s, d) + (10,)


@functools.lru_cache(maxsize=None)
def _val_graph():
    o = _oracle()
    s, d = pin_ends(*o.gen_rmat(12, 5_000, 0x5EED35), 12)
    return _frozen(s, d, o.gen_values(len(s), 0x5EED35)) + (12,)


def _mapped(f, s, d):
    fs, fd = f(s), f(d)
    assert mask_bits(fs, fd) == f.bits and id_span(fs, fd) == f.span   # the geometry the map is named for
    return fs, fd


# ---- union-find: ConnectedComponents and BipartitenessCheck ----------------------------------------------
def _check_components(engine, oracle, f, s, d):
    fs, fd = _mapped(f, s, d)
    want = oracle.components(fs, fd)
    for cols in _both(fs, fd):
        _same_cc(engine.components(*cols), want)
        _uf_path(engine, 4, f.bits, len(fs))
        assert engine.stage_times().vertices == len(want[0])


def _check_bipartite(engine, f, s, d):
    fs, fd = _mapped(f, s, d)
    want = canonical(fs, fd)
    assert want[0]
    for cols in _both(fs, fd):
        _same_bip(engine.bipartite(*cols), want)
        _uf_path(engine, 5, f.bits, len(fs))
        assert engine.stage_times().vertices == len(want[1])


def _check_one_bad_edge(engine, f, size):
    """One edge between two vertices on the same side of the largest component, at a random position."""
    s, d, K, (_, v, lab, sign) = _bip_graph(size)
    labels, counts = np.unique(lab, return_counts=True)
    side = v[(lab == labels[np.argmax(counts)]) & (sign == 1)]
    rng = np.random.default_rng(UF_GRAPHS[size][2] + NAMES.index(f.name))
    a, b = rng.choice(side, 2, replace=False)
    at = int(rng.integers(0, len(s) + 1))
    fs, fd = _mapped(f, np.insert(s, at, a), np.insert(d, at, b))
    assert not canonical(fs, fd)[0]
    for cols in _both(fs, fd):
        _failed(engine.bipartite(*cols))
        _uf_path(engine, 5, f.bits, len(fs))


@pytest.mark.parametrize("name", TABLE_MAPS)
@pytest.mark.parametrize("size", list(UF_GRAPHS))
def test_components_under_map(engine, oracle, size, name):
    s, d, K = _cc_graph(size)
    _check_components(engine, oracle, maps(K)[name], s, d)


@pytest.mark.parametrize("name", TABLE_MAPS)
@pytest.mark.parametrize("size", list(UF_GRAPHS))
def test_bipartite_under_map(engine, size, name):
    s, d, K, _ = _bip_graph(size)
    _check_bipartite(engine, maps(K)[name], s, d)


@pytest.mark.parametrize("name", TABLE_MAPS)
@pytest.mark.parametrize("size", list(UF_GRAPHS))
def test_one_bad_edge_fails_the_window_under_map(engine, size, name):
    _check_one_bad_edge(engine, maps(_bip_graph(size)[2])[name], size)


# ---- a state computed on one path and merged on another ---------------------------------------------------
# window 1: the edges with both base endpoints below 2^(K - 1) (direct, K - 1 bits under all three maps); window 2:
# the rest, whose ids together with the state's rows give the map's own geometry
GEOMETRY_CHANGES = ["identity", "straddle_2p28", "straddle_zero"]   # direct with B grown / narrow relabel / wide relabel


def _two_windows(s, d, K):
    half = 1 << (K - 1)
    s, d = pin_ends(s, d, K, 0, half - 1, at=1)   # window 1 spans [0, 2^(K - 1)); record 0 = (0, 2^K - 1) is window 2's
    low = (s < half) & (d < half)
    assert low[1] and not low[0]
    return (s[low], d[low]), (s[~low], d[~low]), (s, d)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", GEOMETRY_CHANGES)
def test_components_state_across_a_geometry_change(engine, oracle, name, where):
    s, d, K = _cc_graph("s12")
    f = maps(K)[name]
    (s1, d1), (s2, d2), (sa, da) = ((f(a), f(b)) for a, b in _two_windows(s, d, K))
    want1 = oracle.components(s1, d1)
    want2 = oracle.components(s2, d2, want1)
    cols = _dev if where == "device" else (lambda *c: tuple(np.array(x) for x in c))
    got1 = engine.components(*cols(s1, d1))
    _same_cc(got1, want1)
    _uf_path(engine, 4, K - 1, len(s1))
    got2 = engine.components(*cols(s2, d2), got1)
    _same_cc(got2, want2)
    _uf_path(engine, 4, f.bits, len(s2) + len(want1[0]))
    _same_cc(got2, oracle.components(sa, da))   # = the components of all the edges


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("name", GEOMETRY_CHANGES)
def test_bipartite_state_across_a_geometry_change(engine, name, where):
    s, d, K, _ = _bip_graph("s12")
    f = maps(K)[name]
    (b1, e1), (b2, e2), (sa, da) = _two_windows(s, d, K)
    (s1, d1), (s2, d2), (sa, da) = ((f(a), f(b)) for a, b in ((b1, e1), (b2, e2), (sa, da)))
    want1 = canonical(s1, d1)
    want2 = canonical(s2, d2, want1)
    assert want1[0] and want2[0]
    cols = _dev if where == "device" else (lambda *c: tuple(np.array(x) for x in c))
    got1 = engine.bipartite(*cols(s1, d1))
    _same_bip(got1, want1)
    _uf_path(engine, 5, K - 1, len(s1))
    got2 = engine.bipartite(*cols(s2, d2), got1)
    _same_bip(got2, want2)
    _uf_path(engine, 5, f.bits, len(s2) + len(want1[1]))
    _same_bip(got2, canonical(sa, da))   # = the state of all the edges
    # one more window-2 edge, between two vertices the state puts on the same side of its largest component and that
    # no edge of window 2 touches: only the state rows' signs can refute it
    _, v, lab, sign = want1
    labels, counts = np.unique(lab, return_counts=True)
    side = v[(lab == labels[np.argmax(counts)]) & (sign == 1) & ~np.isin(v, np.concatenate([s2, d2]))]
    rng = np.random.default_rng(GEOMETRY_CHANGES.index(name))
    a, b = rng.choice(side, 2, replace=False)
    at = int(rng.integers(1, len(s2) + 1))
    s3, d3 = np.insert(s2, at, a), np.insert(d2, at, b)
    assert not canonical(s3, d3, want1)[0]
    _failed(engine.bipartite(*cols(s3, d3), got1))
    _uf_path(engine, 5, f.bits, len(s3) + len(want1[1]))


# ---- tiny windows: the choice is made on the XOR mask, not on the span -----------------------------------
def _tiny_windows(f):
    lo, hi = (int(x) for x in f(np.array([0, (1 << f.K) - 1])))
    a = lambda *x: np.array(x, np.int64)
    return [("edge", a(lo), a(hi), f.bits), ("loop", a(hi), a(hi), 0), ("both", a(lo, hi), a(hi, hi), f.bits)]


def _check_tiny_union_find(engine, oracle, f):
    for kind, s, d, bits in _tiny_windows(f):
        assert mask_bits(s, d) == bits
        want_cc, want_bip = oracle.components(s, d), canonical(s, d)
        assert want_bip[0] and len(want_cc[0]) == (1 if kind == "loop" else 2)
        for cols in _both(s, d):
            _same_cc(engine.components(*cols), want_cc)
            _uf_path(engine, 4, bits, len(s))
            _same_bip(engine.bipartite(*cols), want_bip)
            _uf_path(engine, 5, bits, len(s))


def _check_tiny_triangles(engine, oracle, f):
    for kind, s, d, bits in _tiny_windows(f):
        assert mask_bits(s, d) == bits
        w, ex, has, _ = oracle.window_triangles_ref(s, d)
        for cols in _both(s, d):
            assert engine.triangles(*cols) == (ex, w, has), kind
            if kind != "loop":   # (a window without a proper edge ends before the count, which writes the stage times)
                t = engine.stage_times()
                assert (t.path, t.key_bits) == (3, bits if f.direct else 1), kind   # relabeled: two compact ids
            assert engine.triangles_selfpair(*cols) == ex, kind   # no triangle in two vertices: all of it is the self-pair term


@pytest.mark.parametrize("name", TABLE_MAPS)
def test_tiny_windows_union_find(engine, oracle, name):
    _check_tiny_union_find(engine, oracle, maps(12)[name])


@pytest.mark.parametrize("name", TABLE_MAPS)
def test_tiny_windows_triangles(engine, oracle, name):
    _check_tiny_triangles(engine, oracle, maps(12)[name])


@pytest.mark.parametrize("name", NAMES)
def test_tiny_windows_candidates(engine, oracle, name):
    for kind, s, d, bits in _tiny_windows(maps(12)[name]):
        ra, rb, rf, flags = oracle.window_candidates(s, d)
        for cols in _both(s, d):
            ga, gb, gf = engine.candidates(*cols)
            assert engine.last_candidates_jdk_flags == flags, kind
            assert np.array_equal(_np(ga), ra) and np.array_equal(_np(gb), rb) and np.array_equal(_np(gf), rf), kind
            assert engine.candidate_count(*cols) == len(ra)


# ---- triangles --------------------------------------------------------------------------------------------
def _tri_bits(f, fs, fd):
    """tri_geometry's table width: the mask width when direct, else that of the compact ids"""
    return f.bits if f.direct else max(1, (len(np.unique(np.concatenate([fs, fd]))) - 1).bit_length())


def _check_triangles(engine, oracle, f):
    s, d, K = _tri_graph()
    fs, fd = _mapped(f, s, d)
    w, ex, has = oracle.window_triangles_fwd(fs, fd)
    assert ex > 1000 and has
    for cols in _both(fs, fd):
        assert engine.triangles(*cols) == (ex, w, has)
        t = engine.stage_times()
        assert (t.path, t.key_bits) == (3, _tri_bits(f, fs, fd))
    S, D = _dev(fs, fd)
    for nparts in (1, 3):
        assert sum(engine.triangles_part(S, D, p, nparts) for p in range(nparts)) == ex


def _check_triangles_with_loops(engine, oracle, f):
    s, d, K = _loop_graph()
    fs, fd = _mapped(f, s, d)
    w, ex, has, _ = oracle.window_triangles_ref(fs, fd)
    keep = fs != fd
    plain = oracle.window_triangles_fwd(fs[keep], fd[keep])[1]   # the reference's count = this + the self-pair term
    assert 0 < plain < ex
    for cols in _both(fs, fd):
        assert engine.triangles(*cols) == (ex, w, has)
        t = engine.stage_times()
        assert (t.path, t.key_bits) == (3, _tri_bits(f, fs, fd))
        assert engine.triangles_selfpair(*cols) == ex - plain


@pytest.mark.parametrize("name", TABLE_MAPS)
def test_triangles_under_map(engine, oracle, name):
    _check_triangles(engine, oracle, maps(12)[name])


@pytest.mark.parametrize("name", TABLE_MAPS)
def test_triangles_with_self_loops_under_map(engine, oracle, name):
    _check_triangles_with_loops(engine, oracle, maps(10)[name])


def test_triangles_guessed_histograms_on_other_bases(pkg, oracle):
    """tri_geometry counts the partition histograms at the previous window's width, with key_xor 0, before it
    knows this window's ids.  A fresh engine, five windows: steps 2, 3 and 5 have the previous window's width
    under another key_xor, or follow a miss (steps 4 and 5 change the width).
    Nothing the library reports shows that a guessed histogram was consumed: that B = 24 takes the partitioned keys
    (V > 2^23) and that a repeated width keeps the guess (from 8 bits up) is pinned against the source by
    test_idmaps_ref.test_guessed_histograms_are_consumed_at_24_bits."""
    s, d, K = _tri_graph()
    m = maps(K)
    steps = [("spread_2p24", 0, 24), ("spread_2p24_neg", 0, 24), ("spread_2p24", 1 << 40, 24), ("identity", 0, 12),
             ("spread_2p24_neg", 0, 24)]
    eng = pkg.Engine(0)
    try:
        for name, off, bits in steps:
            fs, fd = m[name](s) + off, m[name](d) + off
            assert mask_bits(fs, fd) == bits
            w, ex, has = oracle.window_triangles_fwd(fs, fd)
            assert eng.triangles(*_dev(fs, fd)) == (ex, w, has), (name, off)
            t = eng.stage_times()
            assert (t.path, t.key_bits) == (3, bits)
    finally:
        eng.close()


# ---- candidates ---------------------------------------------------------------------------------------------
def _chunks(engine, cols, cap, u32=False):
    total = engine.candidates_begin(*cols)
    parts, at, done, base = [], 0, False, 0
    while not done:
        if u32:
            a, b, f, first, done, base = engine.candidates_next_u32(cap)
        else:
            a, b, f, first, done = engine.candidates_next(cap)
        assert first == at and (len(a) == cap or done)
        at += len(a)
        parts.append([_np(x) for x in (a, b, f)])
    assert at == total
    return [np.concatenate([p[i] for p in parts]) for i in range(3)], base


def _same_records(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(_np(g), w)


@pytest.mark.parametrize("name", NAMES)
def test_candidates_under_map(engine, oracle, name):
    s, d, K = _loop_graph()
    fs, fd = _mapped(maps(K)[name], s, d)
    ra, rb, rf, flags = oracle.window_candidates(fs, fd)
    for cols in _both(fs, fd):
        _same_records(engine.candidates(*cols), (ra, rb, rf))
        assert engine.last_candidates_jdk_flags == flags
        assert engine.candidate_count(*cols) == len(ra)
        got, _ = _chunks(engine, cols, 1000)
        _same_records(got, (ra, rb, rf))


@pytest.mark.parametrize("name", NAMES)
def test_candidate_u32_chunks_under_map(pkg, engine, oracle, name):
    """ids relative to the window's smallest id in uint32 columns, up to a span of exactly 2^32 - 1 (there the
    largest column value is 0xFFFFFFFF); one more and the call refuses, and the session goes on with 64-bit ids."""
    s, d, K = _loop_graph()
    f = maps(K)[name]
    fs, fd = _mapped(f, s, d)
    ra, rb, rf, flags = oracle.window_candidates(fs, fd)
    lo = min(int(fs.min()), int(fd.min()))
    for cols in _both(fs, fd):
        if f.span <= 0xFFFFFFFF:
            (ga, gb, gf), base = _chunks(engine, cols, 4096, u32=True)
            assert base == lo and ga.dtype == np.uint32 and gb.dtype == np.uint32
            assert max(int(ga.max()), int(gb.max())) == f.span   # both ends of the range occur in the records
            _same_records((ga.astype(np.int64) + base, gb.astype(np.int64) + base, gf), (ra, rb, rf))
        else:
            assert engine.candidates_begin(*cols) == len(ra)
            with pytest.raises(pkg.GsError):
                engine.candidates_next_u32(4096)
            a, b, fl, first, done = engine.candidates_next(1 << 20)
            assert first == 0 and done
            _same_records((a, b, fl), (ra, rb, rf))


# ---- stage 2: keyBy(0, 1) CountTriangles + sum(0) over candidate records ----------------------------------
@functools.lru_cache(maxsize=None)
def _stage2_records():
    """GenerateCandidateEdges records of the s10 graph in base ids, and five more that put 0 and 2^K - 1 into
    each column on records whose groups a key that drops a bit would merge: (top, 0) with (0, 0), (0, top) with
    (1, 0)"""
    s, d, K = _loop_graph()
    a, b, f, _ = _oracle().window_candidates(s, d)
    top = (1 << K) - 1
    more = np.array([(0, 0, 0), (top, 0, 1), (0, top, 1), (1, 0, 0), (top, top, 0)], np.int64)
    a, b = np.concatenate([a, more[:, 0]]), np.concatenate([b, more[:, 1]])
    f = np.concatenate([f, more[:, 2].astype(np.uint8)])
    for col in (a, b):
        assert col.min() == 0 and col.max() == top
    return _frozen(a, b, f) + (K,)


STAGE2 = [("span_2p32m1", "span_2p32m1", True),      # both spans 2^32 - 1: packed, no relabel
          ("span_2p32", "identity", False),          # each side of the span test alone: relabel
          ("identity", "span_2p32", False),
          ("negative_band", "offset_2p40", True),    # packed, amin and bmin far apart
          ("extremes", "extremes", False)]


@pytest.mark.parametrize("ma,mb,packed", STAGE2, ids=[f"{x}-{y}" for x, y, _ in STAGE2])
def test_count_candidates_columns_mapped_independently(engine, oracle, ma, mb, packed):
    a, b, f, K = _stage2_records()
    m = maps(K)
    fa, fb = m[ma](a), m[mb](b)
    assert (max(int(fa.max()) - int(fa.min()), int(fb.max()) - int(fb.min())) < (1 << 32)) == packed
    w, ex, has, groups = oracle.count_candidates(fa, fb, f)
    assert ex > 1000 and has
    for cols in _both(fa, fb, f):
        assert engine.count_candidates(*cols) == (ex, w, has, groups)


# ---- reduce, fold and CSR: the bucket-or-sort decision and the sort's narrow / wide keys ---------------------
@pytest.mark.parametrize("name", NAMES)
def test_reduce_sum_all_under_map(engine, oracle, name):
    s, d, val, K = _val_graph()
    fs, fd = _mapped(maps(K)[name], s, d)
    rk, rv = oracle.window_reduce(fs, fd, val, oracle.DIR_ALL, oracle.OP_SUM)
    for cols in _both(fs, fd, val):
        gk, gv = engine.reduce(*cols, oracle.DIR_ALL, oracle.OP_SUM)
        assert np.array_equal(_np(gk), rk) and np.array_equal(_np(gv), rv)


@pytest.mark.parametrize("name", NAMES)
def test_fold_degree_max_all_under_map(engine, oracle, name):
    s, d, val, K = _val_graph()
    fs, fd = _mapped(maps(K)[name], s, d)
    want = oracle.window_fold_degree_max(fs, fd, oracle.DIR_ALL)
    for cols in _both(fs, fd):
        got = engine.fold_degree_max(*cols, oracle.DIR_ALL)
        assert len(got) == 3 and all(np.array_equal(_np(g), w) for g, w in zip(got, want))


@pytest.mark.parametrize("name", NAMES)
def test_csr_out_under_map(engine, oracle, name):
    s, d, val, K = _val_graph()
    fs, fd = _mapped(maps(K)[name], s, d)
    want = oracle.window_csr(fs, fd, val, oracle.DIR_OUT)
    for cols in _both(fs, fd, val):
        got = engine.csr(*cols, oracle.DIR_OUT)
        assert len(got) == 4 and all(np.array_equal(_np(g), w) for g, w in zip(got, want))


# ---- the largest direct tables, B = 28 ------------------------------------------------------------------------
# An engine each, closed at the end: the union-find tables alone are 21 bytes per id (5.3 GiB), and the session
# engine's buffers must not stay grown for the rest of the suite.
def test_components_spread_2p28(pkg, oracle):
    with pkg.Engine(0) as eng:
        for size in UF_GRAPHS:   # the one-pass unions, then the two-phase ones: compression and giant-tree table over 2^28 words
            s, d, K = _cc_graph(size)
            _check_components(eng, oracle, maps(K)["spread_2p28"], s, d)
            assert eng.stage_times().key_bits == 28


def test_bipartite_spread_2p28(pkg, oracle):
    with pkg.Engine(0) as eng:
        for size in UF_GRAPHS:
            s, d, K, _ = _bip_graph(size)
            _check_bipartite(eng, maps(K)["spread_2p28"], s, d)
            assert eng.stage_times().key_bits == 28
            _check_one_bad_edge(eng, maps(K)["spread_2p28"], size)
            assert eng.stage_times().key_bits == 28
        _check_tiny_union_find(eng, oracle, maps(12)["spread_2p28"])


def test_triangles_spread_2p28(pkg, oracle):
    with pkg.Engine(0) as eng:
        _check_triangles(eng, oracle, maps(12)["spread_2p28"])
        assert eng.stage_times().key_bits == 28
        _check_triangles_with_loops(eng, oracle, maps(10)["spread_2p28"])
        _check_tiny_triangles(eng, oracle, maps(12)["spread_2p28"])
