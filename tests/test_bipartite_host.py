"""CPU: BipartitenessCheck's semantics (DESIGN.md "BipartitenessCheck") and ABI surface, without a GPU.

The canonical state (tests/bipartite_cpu.py canonical, what gs_window_bipartite returns) against a
restatement of the reference's Candidates (reference_candidates): equal on the reference's two fixtures and
on every stream whose edges arrive in ascending order of min(src, dst); the documented deviation pinned."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
from bipartite_cpu import canonical, reference_candidates

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "gelly_hip.h"
FIX = json.loads((Path(__file__).parent / "golden" / "bipartiteness_fixtures.json").read_text())
CASES = ("BipartitenessCheckTest", "NonBipartitnessCheckTest")


def test_fixture_holds_the_two_reference_cases():
    assert FIX["BipartitenessCheckTest"]["edges"] == [[1, 2], [1, 3], [1, 4], [4, 5], [4, 7], [4, 9]]
    assert FIX["BipartitenessCheckTest"]["expected"] == \
        "(true,{1={1=(1,true), 2=(2,false), 3=(3,false), 4=(4,false), 5=(5,true), 7=(7,true), 9=(9,true)}})"
    assert FIX["NonBipartitnessCheckTest"]["edges"] == [[1, 2], [2, 3], [3, 1], [4, 5], [5, 7], [4, 1]]
    assert FIX["NonBipartitnessCheckTest"]["expected"] == "(false,{})"
    assert all(FIX[c]["merge_window_ms"] == 500 for c in CASES)


def test_restatement_reproduces_the_fixtures():
    for c in CASES:
        assert reference_candidates(FIX[c]["edges"]) == FIX[c]["expected"], c


def test_canonical_rendering_reproduces_the_fixtures(pkg):
    for c in CASES:
        e = np.array(FIX[c]["edges"], dtype=np.int64)
        assert str(pkg.Candidates(*canonical(e[:, 0], e[:, 1]))) == FIX[c]["expected"], c


def test_candidates_value_class(pkg):
    a = pkg.Candidates(True, np.array([1, 2, 7]), np.array([1, 1, 7]), np.array([1, 0, 1], np.uint8))
    assert str(a) == "(true,{1={1=(1,true), 2=(2,false)}, 7={7=(7,true)}})"
    assert a == pkg.Candidates(True, [1, 2, 7], [1, 1, 7], [True, False, True])
    assert a != pkg.Candidates(True, [1, 2, 7], [1, 1, 7], [True, True, True])
    assert a != pkg.Candidates(False) and str(pkg.Candidates(False)) == "(false,{})"
    neg = pkg.Candidates(True, np.array([-5, 3]), np.array([-5, -5]), np.array([1, 0], np.uint8))
    assert str(neg) == "(true,{-5={-5=(-5,true), 3=(3,false)}})"


def _min_ordered_stream(rng):
    nv, ne = int(rng.integers(3, 26)), int(rng.integers(1, 31))
    e = rng.integers(1, nv + 1, size=(ne, 2))           # self-loops allowed
    e = e[rng.permutation(ne)]                           # ties shuffled ...
    return e[np.argsort(e.min(axis=1), kind="stable")]   # ... under a stable sort by min(src, dst)


def test_canonical_is_the_reference_on_min_ordered_streams(pkg):
    """500 seeded streams of 1-30 edges on 3-25 vertices in ascending order of min(src, dst): the restatement's
    line equals the canonical state's rendering on every one; both outcomes are well represented."""
    rng = np.random.default_rng(0xB1A)
    ok = 0
    for i in range(500):
        e = _min_ordered_stream(rng)
        want = reference_candidates(e.tolist())
        got = pkg.Candidates(*canonical(e[:, 0], e[:, 1]))
        assert str(got) == want, (i, e.tolist())
        ok += got.success
    assert 125 <= ok <= 375, ok


def test_documented_deviation_is_pinned(pkg):
    """A triangle fed as 2-3, 1-2, 1-3 (not min-ordered): Candidates.merge leaves the retired component 2
    unretired (Candidates.java:117-122) and reports success; the canonical state is (false,{})."""
    tri = [[2, 3], [1, 2], [1, 3]]
    # by hand: 1-2 meets component 2 at vertex 2 with opposite signs, so it enters component 1 reversed (1 false,
    # 2 true) and component 2 = {2 true, 3 false} stays; 1-3 then adds 3 true to component 1; merging component 2
    # into it fails on vertex 3, the failure is dropped (:129) and component 2 is removed (:132)
    line = reference_candidates(tri)
    assert line.startswith("(true,") and line == "(true,{1={1=(1,false), 2=(2,true), 3=(3,true)}})"
    e = np.array(tri, dtype=np.int64)
    assert str(pkg.Candidates(*canonical(e[:, 0], e[:, 1]))) == "(false,{})"


def test_canonical_feeds_back(pkg):
    """canonical over (prev, window) = canonical over all the edges; a failed state stays failed."""
    rng = np.random.default_rng(5)
    s = rng.integers(0, 40, 60) * 2
    d = rng.integers(0, 40, 60) * 2 + 1
    whole = canonical(s, d)
    part = canonical(s[30:], d[30:], canonical(s[:30], d[:30]))
    assert whole[0] and pkg.Candidates(*whole) == pkg.Candidates(*part)
    bad = canonical([1, 2, 3], [2, 3, 1])
    assert not bad[0] and not canonical([8], [9], bad)[0]
    assert pkg.Candidates(*canonical([], [], whole)) == pkg.Candidates(*whole)


def test_bipartiteness_emits_one_candidates_per_partial(pkg):
    """BipartitenessCheck's host logic with a stub engine whose bipartite() is `canonical`: at parallelism 3 a
    window emits one Candidates record per non-empty round-robin partition, the state fed back; the edge 3-1
    of the second window closes the odd cycle 1-2-3 and the state stays failed."""
    class Stub:
        calls = []

        def bipartite(self, src, dst, prev=None):
            self.calls.append(len(src))
            return canonical(np.asarray(src), np.asarray(dst), prev)

    src = np.array([1, 2, 1, 6, 8, 3, 10, 3, 12], dtype=np.int64)
    dst = np.array([2, 3, 5, 7, 9, 4, 11, 1, 13], dtype=np.int64)
    ts = np.array([0, 10, 20, 30, 40, 50, 60, 400, 410], dtype=np.int64)   # windows of 7 and 2 records
    env = pkg.StreamExecutionEnvironment()
    env._engine = Stub()
    env.setParallelism(3)
    out = pkg.SimpleEdgeStream(pkg.EdgeColumns(src, dst, None, ts), env).aggregate(pkg.BipartitenessCheck(400))
    assert [w.start for w in out.windows] == [0, 0, 0, 400, 400] and Stub.calls == [3, 2, 2, 1, 1]
    recs = out.collect()
    assert len(recs) == 5 and all(isinstance(r, pkg.Candidates) for r in recs)
    assert recs[0] == pkg.Candidates(*canonical(src[[0, 3, 6]], dst[[0, 3, 6]]))
    assert recs[2] == pkg.Candidates(*canonical(src[:7], dst[:7])) and recs[2].success
    assert str(recs[3]) == "(false,{})" and str(recs[4]) == "(false,{})"


STRUCTS = {"gs_signed_batch": "GsSignedBatch", "gs_signed_out": "GsSignedOut"}


def test_signed_struct_layouts_match_header(pkg, tmp_path):
    """The ctypes mirrors of the two new ABI structs have the sizes and offsets the C compiler gives them."""
    from gelly_streaming_amd import _lib
    lines, want = [], []
    for c_name, py_name in STRUCTS.items():
        t = getattr(_lib, py_name)
        lines.append(f'printf("%zu\\n", sizeof({c_name}));')
        want.append(ctypes.sizeof(t))
        for f, _ in t._fields_:
            lines.append(f'printf("%zu\\n", offsetof({c_name}, {f}));')
            want.append(getattr(t, f).offset)
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gelly_hip.h\"\nint main(){" + "".join(lines) + "}"
    tmp = tmp_path
    (tmp / "sz_signed.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp / "sz_signed.c"), "-o", str(tmp / "sz_signed")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp / "sz_signed")], capture_output=True, text=True).stdout.split()]
    assert got == want


def test_entry_point_declared_and_exported(pkg):
    assert re.search(r"^GS_API\s+gs_status\s+gs_window_bipartite\s*\(", HEADER.read_text(), re.M)
    lib = pkg.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT gs_window_bipartite\b", out)
    assert lib.gs_window_bipartite is not None
    assert issubclass(pkg.BipartitenessCheck, pkg.WindowGraphAggregation)


def test_java_natives_name_the_entry_point():
    java = ROOT / "java/src/main"
    assert "static native long[] windowBipartite(" in (
        java / "java/org/apache/flink/graph/streaming/gpu/GellyHip.java").read_text()
    assert "JNI_FN(windowBipartite)" in (java / "c/gellyhip_jni.c").read_text()
    assert 'fn("gs_window_bipartite"' in (
        java / "java/org/apache/flink/graph/streaming/gpu/GellyHipPanama.java").read_text()
