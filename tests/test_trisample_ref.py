"""CPU: the restatement of the sampling triangle estimators (tests/trisample_ref.py) behaves as the reference's
state machine must -- the replacement chain keeps the held edge uniform, the estimator is unbiased, the
Incidence variant orders its records by sampler -- and the new ABI surface is sound without a device.

The reference draws from Math.random(), so none of its outputs can be pinned; the bounds below are derived,
not measured."""
import ctypes
import math
import random
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import trisample_ref as ref

ROOT = Path(__file__).resolve().parent.parent
ENTRY_POINTS = ("gs_trisample_create", "gs_trisample_destroy", "gs_trisample_edges", "gs_trisample_size",
                "gs_trisample_export", "gs_trisample_import")


def k12_stream(seed=12):
    """the 66 edges of K12, shuffled: V = 12, T = C(12, 3) = 220 triangles"""
    edges = [(a, b) for a in range(12) for b in range(a + 1, 12)]
    random.Random(seed).shuffle(edges)
    return [e[0] for e in edges], [e[1] for e in edges]


# ---- header and layout -----------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_modes():
    header = (ROOT / "include" / "gelly_hip.h").read_text()
    names = set(re.findall(r"^GS_API\s+[\w\s\*]+?\b(gs_\w+)\s*\(", header, re.M))
    assert set(ENTRY_POINTS) <= names
    assert "typedef struct gs_trisample gs_trisample;" in header
    assert re.search(r"GS_TRISAMPLE_BROADCAST = 0, GS_TRISAMPLE_INCIDENCE = 1", header)
    assert re.search(r"#define GS_ABI_VERSION 2\b", header)           # additive: the version stays


def test_library_exports_the_entry_points_and_constants(pkg):
    from gelly_streaming_amd import _lib
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and callable(getattr(lib, name))
    header = (ROOT / "include" / "gelly_hip.h").read_text()
    assert int(re.search(r"#define GS_TRISAMPLE_TILE (\d+)", header).group(1)) == _lib.GS_TRISAMPLE_TILE
    assert int(re.search(r"#define GS_TRISAMPLE_ROW_WORDS (\d+)", header).group(1)) == _lib.GS_TRISAMPLE_ROW_WORDS == 8


def test_header_layout_matches_header(pkg, tmp_path):
    """GsTrisampleHeader has the size and field offsets the C compiler gives gs_trisample_header."""
    from gelly_streaming_amd import _lib
    t = _lib.GsTrisampleHeader
    lines, want = ['printf("%zu\\n", sizeof(gs_trisample_header));'], [ctypes.sizeof(t)]
    for f, _ in t._fields_:
        lines.append(f'printf("%zu\\n", offsetof(gs_trisample_header, {f}));')
        want.append(getattr(t, f).offset)
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gelly_hip.h\"\nint main(){" + "".join(lines) + "}"
    (tmp_path / "sz_ts.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "sz_ts.c"), "-o", str(tmp_path / "sz_ts")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz_ts")], capture_output=True, text=True).stdout.split()]
    assert got == want


def test_entry_points_reject_null_handles_without_a_device(pkg):
    from gelly_streaming_amd import _lib
    lib = pkg.load_library()
    h = ctypes.c_void_p()
    assert lib.gs_trisample_create(None, 0, 10, 0, 100, 1, ctypes.byref(h)) == _lib.GS_EINVAL and not h.value
    n, s = ctypes.c_uint64(7), ctypes.c_int64(7)
    assert lib.gs_trisample_size(None, ctypes.byref(n), ctypes.byref(s)) == _lib.GS_EINVAL
    n_out = ctypes.c_uint64(0)
    vo = _lib.GsVertexOut(None, None, 0, ctypes.pointer(n_out), _lib.GS_MEM_HOST, 0)
    b = _lib.GsEdgeBatch(None, None, None, 0, _lib.GS_NONE, _lib.GS_MEM_HOST, 0)
    assert lib.gs_trisample_edges(None, None, ctypes.byref(b), ctypes.byref(vo)) == _lib.GS_EINVAL
    hdr = _lib.GsTrisampleHeader()
    assert lib.gs_trisample_export(None, None, ctypes.byref(hdr), None, 0, 0, ctypes.byref(n_out)) == _lib.GS_EINVAL
    assert lib.gs_trisample_import(None, None, ctypes.byref(hdr), None, 0, 0) == _lib.GS_EINVAL
    lib.gs_trisample_destroy(None)   # a no-op, like free(NULL)


def test_api_surface(pkg):
    assert callable(pkg.Engine.triangle_sampler)
    for name in ("edges", "size", "export", "load", "close"):
        assert callable(getattr(pkg.TriangleSamplerState, name))
    assert callable(pkg.broadcast_triangle_count) and callable(pkg.incidence_sampling_triangle_count)
    with pytest.raises(ValueError):
        pkg.TriangleSamplerState(None, "exact", 10, 100)   # the mode is checked before the engine is touched


# ---- the replacement chain ----------------------------------------------------------------------------------
def test_chain_is_integer_and_saturates():
    assert ref.next_position(1, 0) == ref.NEVER                       # r32 = 0: 2^32 + 1 > 2^31 - 1
    assert ref.next_position(1, ref.M64) == 2                         # r32 + 1 = 2^32: the very next edge
    assert ref.next_position(5, ref.M64) == 6
    assert ref.next_position(3, (1 << 63)) == 6                       # r32 + 1 = 2^31 + 1: floor(3 * 2^32 / (2^31 + 1)) + 1
    assert ref.next_position(ref.INT_MAX, ref.M64) == ref.NEVER       # 2^31 is past the int range
    assert ref.draw(1, 2, 3, 4) != ref.draw(1, 2, 4, 3) and ref.draw(0, 0, 0, 0) == ref.mix(ref.mix(ref.mix(0, 0), 0), 0)


def test_held_position_is_uniform():
    """20 000 samplers over 10 edges: the held edge is each position with probability 1/10, so a cell's count
    is binomial(S, 0.1) and must lie within 5 sigma of S / 10."""
    S, n = 20_000, 10
    st = ref.TriangleSamplerRef("broadcast", S, 1000, seed=0xC01)
    st.edges(list(range(100, 100 + n)), list(range(200, 200 + n)))
    counts = np.bincount(st.last, minlength=n + 1)
    assert counts[0] == 0 and counts.sum() == S
    sigma = math.sqrt(S * 0.1 * 0.9)
    assert np.all(np.abs(counts[1:] - S / n) <= 5 * sigma), counts
    assert np.array_equal(st.src, st.last + 99) and np.array_equal(st.trg, st.last + 199)   # the edge at that position
    assert np.all((st.next > n) & (st.next <= ref.NEVER)) and np.all(st.j >= 1)


# ---- the estimator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["broadcast", "incidence"])
def test_estimator_is_unbiased_on_k12(mode):
    """Duplicate-free stream, ids in [0, V): a sampler ends with beta = 1 exactly when it holds the first
    arriving edge of a triangle and drew that triangle's apex, p = T / (E (V - 2)) = 220 / (66 * 10) = 1/3."""
    S, V, E, T = 4096, 12, 66, 220
    p = T / (E * (V - 2))
    src, dst = k12_stream()
    st = ref.TriangleSamplerRef(mode, S, V, seed=0x7E57)
    records = st.edges(src, dst)
    total = st.beta_sum()
    assert abs(total - S * p) <= 5 * math.sqrt(S * p * (1 - p)), total
    # every third vertex avoids the held edge's endpoints and lies in [0, V)
    assert np.all((st.third != st.src) & (st.third != st.trg) & (st.third >= 0) & (st.third < V))
    summer = ref.TriangleSummerRef(S, V)
    out = summer.feed(0, records)
    k, b = records[-1]
    assert out[-1] == (k, int((1.0 / S) * b * k * (V - 2)))
    if mode == "broadcast":
        assert b == total                                             # the last record is the final sum
        assert all(x[0] < y[0] for x, y in zip(records, records[1:]))   # at most one record per edge


def test_summer_hand_cases():
    s = ref.TriangleSummerRef(10, 12)
    assert s.estimate(0, 5, 0) == [] and s.estimate(0, 6, 0) == []    # the result stays 0: nothing
    assert s.estimate(0, 7, 1) == [(7, 7)]                            # (1/10) * 1 * 7 * 10
    assert s.estimate(0, 7, 1) == []                                  # unchanged
    # two sources replace their own estimates, never each other's; maxEdges only grows
    assert s.estimate(1, 9, 2) == [(9, 27)]                           # (1/10) * 3 * 9 * 10
    assert s.estimate(0, 8, 0) == [(9, 18)]                           # source 0 drops to 0: (1/10) * 2 * 9 * 10
    assert s.estimate(1, 10, 0) == [(10, 0)]
    # (int) saturates at 2^31 - 1
    big = ref.TriangleSummerRef(1, ref.INT_MAX)
    assert big.estimate(0, ref.INT_MAX, 1000) == [(ref.INT_MAX, ref.INT_MAX)]
    assert ref.java_int_cast(float("nan")) == 0 and ref.java_int_cast(-1e300) == ref.INT_MIN and ref.java_int_cast(-2.9) == -2


def test_package_summer_agrees_with_the_restatement(pkg):
    """gelly_streaming_amd.TriangleSummer against the restatement on the K12 records of two sources."""
    src, dst = k12_stream()
    a = ref.TriangleSamplerRef("broadcast", 200, 12, seed=5).edges(src, dst)
    b = ref.TriangleSamplerRef("broadcast", 200, 12, seed=5, first_sampler=200).edges(src, dst)
    merged = sorted([(k, 0, i, x) for i, (k, x) in enumerate(a)] + [(k, 1, i, x) for i, (k, x) in enumerate(b)])
    want, got = [], []
    rs, ps = ref.TriangleSummerRef(400, 12), pkg.TriangleSummer(400, 12)
    for k, source, _, x in merged:
        want.extend(rs.estimate(source, k, x))
        ps.flatMap(source, k, x, got)
    assert got == want and len(got) > 10
    from gelly_streaming_amd import triangle_estimate as te
    assert te.merge_estimates([(0, [k for k, _ in a], [x for _, x in a]), (1, [k for k, _ in b], [x for _, x in b])]) == \
        [(source, k, x) for k, source, _, x in merged]
    assert te.java_int_cast(3e9) == ref.INT_MAX and te.java_int_cast(float("nan")) == 0


# ---- Incidence ordering ---------------------------------------------------------------------------------------
def _incidence_case(want):
    """search the seeds for a K12 run whose trace holds `want` at one position; (state's records, position,
    the samplers involved)"""
    src, dst = k12_stream()
    for seed in range(400):
        st = ref.TriangleSamplerRef("incidence", 48, 12, seed=seed, trace=True)
        rec = st.edges(src, dst)
        by_pos = {}
        for what, k, i in st.trace:
            by_pos.setdefault(k, []).append((what, i))
        for k, evs in by_pos.items():
            hit = want(evs)
            if hit:
                return seed, rec, k, hit
    raise AssertionError("no seed below 400 builds the case")


def test_incidence_two_finds_at_one_position_give_two_records():
    def want(evs):
        finds = [i for w, i in evs if w == "find"]
        return finds if len(finds) == 2 and not any(w == "reset" for w, _ in evs) else None
    seed, rec, k, finds = _incidence_case(want)
    at = [r for r in rec if r[0] == k]
    assert len(at) == 2 and at[1][1] == at[0][1] + 1                  # same edge count, one more each
    # Broadcast reports that position once, with the sum after both
    src, dst = k12_stream()
    b = ref.TriangleSamplerRef("broadcast", 48, 12, seed=seed).edges(src, dst)
    assert [r for r in b if r[0] == k] == [(k, at[1][1])]


def test_incidence_reset_before_a_find_shows_in_its_sum():
    def want(evs):
        resets = [i for w, i in evs if w == "reset"]
        finds = [i for w, i in evs if w == "find"]
        return (resets, finds) if len(resets) == 1 and len(finds) == 1 else None
    # a lower-numbered sampler is replaced out of beta = 1 at the edge a higher-numbered one finds at: the sum
    # is unchanged, so Incidence's previousResult comparison drops the record -- and the other order emits
    src, dst = k12_stream()
    seen = set()
    for seed in range(400):
        st = ref.TriangleSamplerRef("incidence", 48, 12, seed=seed, trace=True)
        rec = st.edges(src, dst)
        by_pos = {}
        for what, k, i in st.trace:
            by_pos.setdefault(k, []).append((what, i))
        for k, evs in by_pos.items():
            hit = want(evs)
            if not hit:
                continue
            (r,), (f,) = hit
            at = [x for x in rec if x[0] == k]
            # the state just before this edge: its beta sum s0 and its last emitted sum
            head = ref.TriangleSamplerRef("incidence", 48, 12, seed=seed)
            head.edges(src[:k - 1], dst[:k - 1])
            s0 = head.beta_sum()
            if r < f:      # the reset is in the find's sum: s0 - 1 + 1
                assert at == ([] if s0 == head.previous else [(k, s0)])
                seen.add("reset first")
            else:          # the find does not see the reset yet: s0 + 1
                assert at == ([] if s0 + 1 == head.previous else [(k, s0 + 1)])
                seen.add("find first")
        if len(seen) == 2:
            break
    assert seen == {"reset first", "find first"}
