"""CPU: the plain-Python restatement of distinct() (tests/distinct_ref.py) reproduces TestDistinct's lines and
the literal mapper's, and the new ABI surface is sound without a device."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import pytest

import distinct_ref as ref

ROOT = Path(__file__).resolve().parent.parent
FIX = json.loads((Path(__file__).parent / "golden" / "distinct_fixtures.json").read_text())
ENTRY_POINTS = ("gs_distinct_create", "gs_distinct_destroy", "gs_distinct_edges", "gs_distinct_size",
                "gs_distinct_capacity", "gs_distinct_export", "gs_distinct_import")


def _doubled():
    return [tuple(e) for e in FIX["edges"]] * 2


def test_restatement_reproduces_both_line_sets():
    """compareResultsByLinesInMemory: both sides as sorted lines."""
    assert ref.lines(ref.distinct(_doubled(), ref.KEYED)) == sorted(FIX["distinct"])
    assert ref.lines(ref.distinct(_doubled(), ref.INSTANCE)) == sorted(FIX["instance"])
    assert len(FIX["distinct"]) == 7 and len(FIX["instance"]) == 5


def test_restatement_order_batch_cuts_and_pairs():
    e = _doubled()
    assert ref.distinct(e) == e[:7]                                   # first arrivals, in arrival order
    assert ref.distinct([(1, 2), (2, 1), (1, 2), (3, 3), (3, 3)]) == [(1, 2), (2, 1), (3, 3)]
    assert ref.distinct([(1, 2), (2, 1), (7, 2), (3, 3)], ref.INSTANCE) == [(1, 2), (2, 1), (3, 3)]
    src, dst = [x[0] for x in e], [x[1] for x in e]
    whole, cut = ref.DistinctState(), ref.DistinctState()
    want = whole.edges(src, dst)
    a, b = cut.edges(src[:5], dst[:5]), cut.edges(src[5:], dst[5:])
    assert [r[:2] for r in a + b] == [r[:2] for r in want] and cut.log == whole.log and cut.records == 14
    assert [r[3] for r in b] == [0, 1]                                # index: the position inside its batch


def test_header_declares_the_entry_points_and_modes():
    header = (ROOT / "include" / "gelly_hip.h").read_text()
    names = set(re.findall(r"^GS_API\s+[\w\s\*]+?\b(gs_\w+)\s*\(", header, re.M))
    assert set(ENTRY_POINTS) <= names
    assert "typedef struct gs_distinct gs_distinct;" in header
    assert re.search(r"GS_DISTINCT_KEYED = 0, GS_DISTINCT_INSTANCE = 1", header)
    assert re.search(r"#define GS_ABI_VERSION 2\b", header)           # additive: the version stays


def test_edge_out_layout_matches_header(pkg, tmp_path):
    """GsEdgeOut has the size and field offsets the C compiler gives gs_edge_out."""
    from gelly_streaming_amd import _lib
    t = _lib.GsEdgeOut
    lines, want = ['printf("%zu\\n", sizeof(gs_edge_out));'], [ctypes.sizeof(t)]
    for f, _ in t._fields_:
        lines.append(f'printf("%zu\\n", offsetof(gs_edge_out, {f}));')
        want.append(getattr(t, f).offset)
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gelly_hip.h\"\nint main(){" + "".join(lines) + "}"
    (tmp_path / "sz_ds.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "sz_ds.c"), "-o", str(tmp_path / "sz_ds")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz_ds")], capture_output=True, text=True).stdout.split()]
    assert got == want
    assert [f for f, _ in t._fields_] == ["src", "dst", "val", "index", "capacity", "n_out", "mem", "reserved"]


def test_distinct_entry_points_reject_null_handles_without_a_device(pkg):
    from gelly_streaming_amd import _lib
    lib = pkg.load_library()
    h = ctypes.c_void_p()
    assert lib.gs_distinct_create(None, _lib.GS_DISTINCT_KEYED, 0, ctypes.byref(h)) == _lib.GS_EINVAL and not h.value
    d, r = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.gs_distinct_size(None, ctypes.byref(d), ctypes.byref(r)) == _lib.GS_EINVAL
    assert lib.gs_distinct_capacity(None, ctypes.byref(d), ctypes.byref(r)) == _lib.GS_EINVAL
    n_out = ctypes.c_uint64(0)
    eo = _lib.GsEdgeOut(None, None, None, None, 0, ctypes.pointer(n_out), _lib.GS_MEM_HOST, 0)
    b = _lib.GsEdgeBatch(None, None, None, 0, _lib.GS_NONE, _lib.GS_MEM_HOST, 0)
    assert lib.gs_distinct_edges(None, None, ctypes.byref(b), ctypes.byref(eo)) == _lib.GS_EINVAL
    assert lib.gs_distinct_export(None, None, ctypes.byref(eo)) == _lib.GS_EINVAL
    assert lib.gs_distinct_import(None, None, ctypes.byref(b)) == _lib.GS_EINVAL
    lib.gs_distinct_destroy(None)   # a no-op, like free(NULL)


def test_api_surface(pkg):
    assert callable(pkg.SimpleEdgeStream.distinct) and callable(pkg.Engine.distinct)
    for name in ("edges", "size", "capacity", "export", "load", "close"):
        assert callable(getattr(pkg.DistinctState, name))
    with pytest.raises(ValueError):
        pkg.DistinctState(None, mode="per-key")   # the mode is checked before the engine is touched
