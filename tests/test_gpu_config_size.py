"""GPU parity at the BASELINE configs' own sizes, against the C oracle's large-window
restatements (oracle/gs_oracle.c: gso_window_fold_mt — the arrival-order fold spread over threads the
way keyBy spreads it over subtasks; gso_triangles_fwd_mt — an independent forward-algorithm count).

  C2  R-MAT scale 24, E = 2^28, reduceOnEdges(SUM) OUT: Long values bit-exact, Double values within
      1e-5 relative (north star), both on two distinct windows of the stream
  C3  skewed R-MAT scale 24 (.65/.15/.15/.05, no permutation) and the Zipf(1.1) source stream, E = 2^28:
      foldNeighbors(degree, max neighbour) bit-exact
  C4  WindowTriangles on self-loop-free R-MAT windows at scales 20, 22, 24 (2^28 edges) and the C4
      window itself, scale 26 (2^30 edges): the exact count equals the oracle's independent count (and
      the reference's Integer is its low 32 bits)
  C5  one 1e8-edge R-MAT scale-23 window: applyOnNeighbors' grouping (gs_window_csr, ALL: keys, offsets,
      neighbours in arrival order) equals oracle.window_csr, and the GenerateCandidateEdges sizing call
      (1.6e11 records) equals oracle.candidate_count
  C2 / C3 on one fresh ctx, two windows: the second through the speculative partition

The windows are generated on the device (gs_generate_*, bit-identical to the oracle's generators:
test_gpu_parity.test_generators_match_oracle, and re-checked here on a sample of each window)."""
import contextlib
import threading
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from valcheck import FLOAT_RTOL, assert_values  # north_star: float weight sums within 1e-5 relative

pytestmark = pytest.mark.gpu


def _sample_matches_oracle(oracle, src, dst, gen, first_edge, k=4096):
    """Spot-check a device window against the oracle generator at three offsets."""
    n = src.numel()
    for off in (0, n // 2, n - k):
        s, d = gen(k, first_edge + off)
        assert np.array_equal(src[off:off + k].cpu().numpy(), s) and np.array_equal(dst[off:off + k].cpu().numpy(), d)


@pytest.mark.parametrize("window", [0, 1])
def test_c2_full_window_long_bit_exact(engine, oracle, window):
    scale, E, seed = 24, 1 << 28, 0x5EED02
    fe = window * E
    src, dst = engine.generate_rmat(scale, E, seed, first_edge=fe)
    val = engine.generate_values(E, seed, 1, first_edge=fe)
    _sample_matches_oracle(oracle, src, dst, lambda k, f: oracle.gen_rmat(scale, k, seed, first_edge=f), fe)
    gk, gv = engine.reduce(src, dst, val, 1, 0)
    t = engine.stage_times()
    assert t.path == 2
    s_h, d_h, v_h = src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy()
    del src, dst
    rk, rv = oracle.window_reduce_mt(s_h, d_h, v_h, 1, 0)
    assert np.array_equal(gk.cpu().numpy(), rk), "vertex keys differ from the oracle"
    assert np.array_equal(gv.cpu().numpy(), rv), "per-vertex Long sums differ from the oracle"


def test_c2_full_window_double_within_tolerance(engine, oracle):
    scale, E, seed = 24, 1 << 28, 0x5EED02
    src, dst = engine.generate_rmat(scale, E, seed)
    val = engine.generate_values(E, seed, 3)
    gk, gv = engine.reduce(src, dst, val, 1, 0)
    s_h, d_h, v_h = src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy()
    del src, dst, val
    rk, rv = oracle.window_reduce_mt(s_h, d_h, v_h, 1, 0)
    assert np.array_equal(gk.cpu().numpy(), rk)
    assert_values(gv.cpu().numpy(), rv, np.float64, 0)   # Double sums within 1e-5 relative


F32_UNIT = 2.0 ** -24   # unit roundoff of Java float


def test_c2_full_window_float_within_tolerance(engine, oracle):
    """C2 with Float (f32) weights, SUM, OUT, at config size.  The reference folds Java floats one record
    at a time in arrival order (GraphWindowStream.java:116-120), rounding every add; the engine adds in
    f64 and rounds once.  At an R-MAT hub (10^5-10^6 records of ~0.5) the reference's own rounding can
    exceed 1e-5, so the test checks, per vertex:
      1. the engine's sum is the exact sum of the f32 values to within 1e-6 relative;
      2. the engine is within 1e-5 relative of the sequential f32 fold (oracle window_reduce_mt), OR the
         difference is within the sequential fold's own rounding bound |fold - exact| <= gamma_(n-1) *
         sum|v| (Higham 2002, eq. 4.4: gamma_m = m u / (1 - m u), u = 2^-24) -- i.e. the two differ only
         by the reference's rounding.
    The count of vertices that need clause 2's second half and the worst relative difference are printed
    (DESIGN.md §2 records them: f32 parity at hub scale rests on the exact sum, not on the fold)."""
    scale, E, seed = 24, 1 << 28, 0x5EED02
    src, dst = engine.generate_rmat(scale, E, seed)
    val = engine.generate_values(E, seed, 2)
    gk, gv = engine.reduce(src, dst, val, 1, 0)
    s_h, d_h, v_h = src.cpu().numpy(), dst.cpu().numpy(), val.cpu().numpy()
    del src, dst, val
    rk, rv = oracle.window_reduce_mt(s_h, d_h, v_h, 1, 0)
    del d_h
    g = gv.cpu().numpy().astype(np.float64)
    assert np.array_equal(gk.cpu().numpy(), rk)
    exact = np.bincount(s_h, weights=v_h.astype(np.float64), minlength=1 << scale)[rk]
    deg = np.bincount(s_h, minlength=1 << scale)[rk].astype(np.float64)
    del s_h, v_h
    assert (np.abs(g - exact) <= 1e-6 * exact).all(), "engine sum is not the exact sum to 1e-6"
    r = rv.astype(np.float64)
    rel = np.abs(g - r) / np.maximum(np.abs(r), 1e-30)
    mu = (deg - 1) * F32_UNIT
    bound = mu / (1 - mu) * exact + 1e-6 * exact
    ok = (rel <= FLOAT_RTOL) | (np.abs(g - r) <= bound)
    assert ok.all(), f"{int((~ok).sum())} Float sums differ beyond the reference fold's own rounding"
    outside = rel > FLOAT_RTOL
    print(f"\nC2 f32: {len(r)} vertices, {int(outside.sum())} beyond 1e-5 of the sequential f32 fold "
          f"(max degree among them {int(deg[outside].max()) if outside.any() else 0}); worst relative "
          f"difference {rel.max():.3e} at degree {int(deg[rel.argmax()])}; fold vs exact worst "
          f"{(np.abs(r - exact) / exact).max():.3e}")


@pytest.mark.parametrize("stream", ["rmat", "zipf"])
def test_c3_full_window_degree_max(engine, oracle, stream):
    scale, E, seed = 24, 1 << 28, 0x5EED03
    if stream == "rmat":
        src, dst = engine.generate_rmat(scale, E, seed, a=0.65, b=0.15, c=0.15, permute=False)
        gen = lambda k, f: oracle.gen_rmat(scale, k, seed, a=0.65, b=0.15, c=0.15, permute=False, first_edge=f)
    else:
        src, dst = engine.generate_zipf(1 << scale, E, seed, 1.1)
        gen = lambda k, f: oracle.gen_zipf(1 << scale, k, seed, 1.1, first_edge=f)
    _sample_matches_oracle(oracle, src, dst, gen, 0)
    gk, gd, gm = engine.fold_degree_max(src, dst, 1)
    s_h, d_h = src.cpu().numpy(), dst.cpu().numpy()
    del src, dst
    rk, rd, rm = oracle.window_fold_degree_max_mt(s_h, d_h, 1)
    assert np.array_equal(gk.cpu().numpy(), rk)
    assert np.array_equal(gd.cpu().numpy(), rd), "degrees differ"
    assert np.array_equal(gm.cpu().numpy(), rm), "max neighbours differ"
    assert int(rd.max()) > 1 << 20, "the skewed stream should have a hub"


@pytest.mark.parametrize("kind", ["c2_long", "c3_rmat"])
def test_speculative_partition_full_windows(pkg, oracle, kind):
    """Two consecutive config-size windows on a fresh ctx: the first takes the histogram path, the second
    the speculative partition (regions from the first's bucket counts, atomic run reservations) -- both
    bit-exact against the oracle."""
    scale, E = 24, 1 << 28
    with pkg.Engine(0) as e:
        for window in (0, 1):
            fe = window * E
            if kind == "c2_long":
                seed = 0x5EED02
                src, dst = e.generate_rmat(scale, E, seed, first_edge=fe)
                val = e.generate_values(E, seed, 1, first_edge=fe)
                got = e.reduce(src, dst, val, 1, 0)
                spec = e.stage_times().speculative
                hv = val.cpu().numpy()
                del val
            else:
                seed = 0x5EED03
                src, dst = e.generate_rmat(scale, E, seed, a=0.65, b=0.15, c=0.15, permute=False, first_edge=fe)
                got = e.fold_degree_max(src, dst, 1)
                spec = e.stage_times().speculative
            s_h, d_h = src.cpu().numpy(), dst.cpu().numpy()
            del src, dst
            want = (oracle.window_reduce_mt(s_h, d_h, hv, 1, 0) if kind == "c2_long"
                    else oracle.window_fold_degree_max_mt(s_h, d_h, 1))
            for g, w in zip(got, want):
                assert np.array_equal(g.cpu().numpy(), w), (kind, window)
            assert spec == window, (kind, window, spec)   # 0: histogram path, 1: speculative


@contextlib.contextmanager
def _keepalive(tag):
    """A long oracle call prints nothing: touch a file under gpurun_out/ every 20 s meanwhile (the GPU
    box's hang detector watches stdout / stderr / gpurun_out)."""
    out = Path(__file__).resolve().parent.parent / "gpurun_out"
    stop = threading.Event()

    def beat():
        out.mkdir(exist_ok=True)
        t0 = time.time()
        while not stop.wait(20):
            (out / "keepalive.txt").write_text(f"{tag}: oracle running {time.time() - t0:.0f} s\n")

    th = threading.Thread(target=beat, daemon=True)
    th.start()
    try:
        yield
    finally:
        stop.set()
        th.join()


def _triangles_vs_forward(engine, oracle, scale):
    E, seed = 16 << scale, 0x5EED04
    src, dst = engine.generate_rmat(scale, E, seed, no_self_loops=True)
    exact, wrapped, has = engine.triangles(src, dst)
    _sample_matches_oracle(oracle, src, dst, lambda k, f: oracle.gen_rmat(scale, k, seed, no_self_loops=True,
                                                                          first_edge=f), 0)
    s_h, d_h = src.cpu().numpy(), dst.cpu().numpy()
    del src, dst
    torch.cuda.empty_cache()
    with _keepalive(f"triangles s{scale}"):
        want = oracle.triangles_fwd_mt(s_h, d_h)
    assert exact == want, (exact, want)
    w = want & 0xFFFFFFFF
    assert wrapped == (w - (1 << 32) if w >= 1 << 31 else w) and has


@pytest.mark.parametrize("scale", [20, 22, 24])
@pytest.mark.timeout(300)
def test_c4_shape_triangles_vs_forward_algorithm(engine, oracle, scale):
    _triangles_vs_forward(engine, oracle, scale)


@pytest.mark.timeout(900)
def test_c4_window_s26_triangles_vs_forward_algorithm(engine, oracle):
    """The C4 window itself: R-MAT scale 26, 2^30 edges (the oracle needs ~50 GB of host memory and about
    a minute and a half on 16 threads since its fills went atomic-free and its count probes only the
    out-list suffixes)."""
    _triangles_vs_forward(engine, oracle, 26)


@pytest.fixture(scope="module")
def c5_window(engine, oracle):
    """One C5 window: 1e8 edges of the R-MAT scale-23 stream, on the device and host."""
    scale, E, seed = 23, 100_000_000, 0x5EED05
    src, dst = engine.generate_rmat(scale, E, seed)
    _sample_matches_oracle(oracle, src, dst, lambda k, f: oracle.gen_rmat(scale, k, seed, first_edge=f), 0)
    return src, dst, src.cpu().numpy(), dst.cpu().numpy()


@pytest.mark.timeout(300)
def test_c5_window_csr_vs_oracle(engine, oracle, c5_window):
    """applyOnNeighbors over slice(ALL) (GraphWindowStream.java:130-175): every vertex's neighbours in
    arrival order, duplicates kept -- the whole 2e8-record CSR bit-exact."""
    src, dst, s_h, d_h = c5_window
    gk, go, gn, _ = engine.csr(src, dst, None, 2)
    with _keepalive("c5 csr"):
        rk, ro, rn, _ = oracle.window_csr(s_h, d_h, None, 2)
    assert np.array_equal(gk.cpu().numpy(), rk)
    assert np.array_equal(go.cpu().numpy(), ro)
    del gk, go
    assert np.array_equal(gn.cpu().numpy(), rn)


@pytest.mark.timeout(300)
def test_c5_window_candidate_count_vs_oracle(engine, oracle, c5_window):
    """GenerateCandidateEdges' record count for the whole window (WindowTriangles.java:91-114: the
    neighbour records plus, per vertex, the HashSet-ordered pairs above it incl. self pairs)."""
    src, dst, s_h, d_h = c5_window
    got = engine.candidate_count(src, dst)
    with _keepalive("c5 candidates"):
        want = oracle.candidate_count(s_h, d_h)
    assert got == want, (got, want)
    assert want > 10 ** 11


def test_zipf_generator_matches_oracle(engine, oracle):
    n = 1 << 18
    for V, s, f in ((1 << 24, 1.1, 0), (1 << 10, 2.0, 77), (12345, 0.8, 1 << 30)):
        gs_, gd_ = engine.generate_zipf(V, n, 0x5EED03, s, first_edge=f)
        os_, od_ = oracle.gen_zipf(V, n, 0x5EED03, s, first_edge=f)
        assert np.array_equal(gs_.cpu().numpy(), os_) and np.array_equal(gd_.cpu().numpy(), od_)
    # hubs at the lowest IDs: ID 0 is the most frequent source
    c = np.bincount(os_)
    assert c.argmax() == 0


def _blocks_of(a, b, f, v0, v1):
    """The records of vertices in [v0, v1) from a GenerateCandidateEdges output (vertex order): a vertex's
    block starts at its first edge record (a = v, is_candidate = 0) and runs to the next vertex's."""
    f = f.astype(bool)
    start = ~f & np.concatenate([[True], f[:-1] | (a[1:] != a[:-1])])
    owner = np.maximum.accumulate(np.where(start, np.arange(len(a)), 0))
    keep = (a[owner] >= v0) & (a[owner] < v1)
    return a[keep], b[keep], f[keep].astype(np.uint8)


def _incident(s_h, d_h, vs):
    """the window's edges incident to a set of vertices, in stream order"""
    m = np.isin(s_h, vs) | np.isin(d_h, vs)
    return s_h[m], d_h[m]


def _gpu_span(engine, first, n):
    engine.candidates_seek(first)
    ga, gb, gf, at, _ = engine.candidates_next(n)
    assert at == first and len(ga) == n
    return ga.cpu().numpy(), gb.cpu().numpy(), gf.cpu().numpy()


@pytest.mark.timeout(300)
def test_c5_window_candidate_records_vertex_ranges(engine, oracle, c5_window):
    """GenerateCandidateEdges records of the whole C5 window (1e8 edges, 1.6e11 records) compared record
    for record on vertex ranges (WindowTriangles.java:91-114), streamed out of one gs_candidates session
    with gs_candidates_vertex_range + gs_candidates_seek + gs_candidates_next:
      * three ranges of consecutive ids (around the median-degree vertex, the lowest and the highest ids):
        the oracle's gso_window_candidates over the edges incident to the range (a vertex's records
        depend only on its own neighbour records), its blocks for the range's vertices;
      * the hub (largest degree): its block length, its edge records and first pair rows, a slice from
        its middle and its last rows, against the exact JDK HashSet order of its neighbours
        (oracle.hashset_order) expanded by the reference's loop rule."""
    src, dst, s_h, d_h = c5_window
    total = engine.candidates_begin(src, dst)
    V = int(max(s_h.max(), d_h.max())) + 1
    deg = np.bincount(s_h, minlength=V) + np.bincount(d_h, minlength=V)   # slice(ALL) records per vertex
    present = np.nonzero(deg)[0]
    med = present[np.argsort(deg[present], kind="stable")[len(present) // 2]]
    checked = 0
    for lo_id in (int(med), int(present[0]), int(present[-1000])):
        width = 1000
        while True:
            ids = present[(present >= lo_id) & (present < lo_id + width)]
            first, _ = engine.candidates_vertex_range(int(ids[0]))
            last_first, last_n = engine.candidates_vertex_range(int(ids[-1]))
            span = last_first + last_n - first
            if span <= 30_000_000 or width == 1:
                break
            width //= 4
        v0, v1 = lo_id, lo_id + width
        ss, dd = _incident(s_h, d_h, ids)
        ra, rb, rf, _ = oracle.window_candidates(ss, dd)
        ra, rb, rf = _blocks_of(ra, rb, rf, v0, v1)
        assert len(ra) == span, (v0, v1, len(ra), span)
        ga, gb, gf = _gpu_span(engine, first, span)
        assert np.array_equal(ga, ra) and np.array_equal(gb, rb) and np.array_equal(gf, rf), (v0, v1)
        checked += span
    # an id absent from the window has no records
    absent = np.setdiff1d(np.arange(present[0], present[0] + 4096), present)
    if len(absent):
        assert engine.candidates_vertex_range(int(absent[0]))[1] == 0
    # the hub
    hub = int(np.argmax(deg))
    m = (s_h == hub) | (d_h == hub)
    ss, dd = s_h[m], d_h[m]
    # ALL (SimpleEdgeStream.java:354-365): per edge (src, dst) then (dst, src); the hub's neighbour records
    recs = np.stack([dd, ss], axis=1).reshape(-1)
    mine = np.stack([ss == hub, dd == hub], axis=1).reshape(-1)
    nbrs = recs[mine]
    _, fi = np.unique(nbrs, return_index=True)
    order, _, flags = oracle.hashset_order(nbrs[np.sort(fi)])
    G = order[order > hub]
    k = len(G)
    rows = k - int(order[-1] > hub) if k else 0
    d = len(nbrs)
    first, n = engine.candidates_vertex_range(hub)
    assert n == d + rows * k - rows * (rows - 1) // 2, (n, d, k, rows)
    row_off = np.arange(rows + 1, dtype=np.int64)
    row_off = row_off * k - row_off * (row_off - 1) // 2

    def expected(p0, p1):   # block positions [p0, p1) of the hub
        p = np.arange(p0, p1, dtype=np.int64)
        ea = np.full(len(p), hub, np.int64)
        eb = np.empty(len(p), np.int64)
        ef = (p >= d).astype(np.uint8)
        eb[p < d] = nbrs[p[p < d]]
        q = p[p >= d] - d
        r = np.searchsorted(row_off, q, side="right") - 1
        ea[p >= d] = G[r]
        eb[p >= d] = G[r + (q - row_off[r])]
        return ea, eb, ef

    for p0, p1 in ((0, min(n, d + 3 * k)), (n // 2, min(n, n // 2 + 1_000_000)), (max(0, n - 3 * k), n)):
        ga, gb, gf = _gpu_span(engine, first + p0, p1 - p0)
        ea, eb, ef = expected(p0, p1)
        assert np.array_equal(ga, ea) and np.array_equal(gb, eb) and np.array_equal(gf, ef), (hub, p0, p1)
        checked += p1 - p0
    print(f"\nC5 candidates: {total} records in the window, {checked} compared record for record; hub {hub}: "
          f"{d} edge records, {k} ids above it, block {n}, JDK flags {flags}")
