"""CPU: the plain-Python restatement of the continuous operators (tests/continuous_ref.py) reproduces the
reference's TestGetDegrees / TestGetVertices / TestNumberOfEntities lines, and the new ABI surface is
sound without a device."""
import ctypes
import json
import subprocess
from pathlib import Path

import pytest

import continuous_ref as ref

ROOT = Path(__file__).resolve().parent.parent
FIX = json.loads((Path(__file__).parent / "golden" / "continuous_fixtures.json").read_text())

CASES = {
    "getDegrees": lambda e: ref.get_degrees(e, ref.ALL),
    "getInDegrees": lambda e: ref.get_degrees(e, ref.IN),
    "getOutDegrees": lambda e: ref.get_degrees(e, ref.OUT),
    "getVertices": ref.get_vertices,
    "numberOfVertices": ref.number_of_vertices,
    "numberOfEdges": ref.number_of_edges,
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_reproduces_the_reference_lines(case):
    """compareResultsByLinesInMemory: both sides as sorted lines."""
    assert ref.lines(CASES[case](FIX["edges"])) == sorted(FIX[case])


def test_restatement_order_and_batch_cuts():
    """the P = 1 record order (source's record, then target's), and the state carried across batches"""
    e = FIX["edges"]
    assert ref.get_degrees(e, ref.ALL)[:6] == [(1, 1), (2, 1), (1, 2), (3, 1), (2, 2), (3, 2)]
    assert ref.get_vertices(e) == [(1,), (2,), (3,), (4,), (5,)]
    assert ref.get_degrees([(7, 7)], ref.ALL) == [(7, 1), (7, 2)]   # a self-loop: two records of one vertex
    src, dst = [x[0] for x in e], [x[1] for x in e]
    whole, cut = ref.DegreeState(), ref.DegreeState()
    want = whole.degrees(src, dst, ref.ALL)
    got = cut.degrees(src[:3], dst[:3], ref.ALL) + cut.degrees(src[3:], dst[3:], ref.ALL)
    assert got == want and cut.export() == whole.export() and cut.records == 14


def test_continuous_entry_points_share_the_existing_structs(pkg, tmp_path):
    """The continuous entry points add no struct to the ABI: they take gs_edge_batch, gs_vertex_out and
    gs_partial_batch, whose ctypes mirrors must match the header's layout (gcc offsetof, as
    test_struct_layouts_match_header does), and the opaque gs_cont is declared."""
    from gelly_streaming_amd import _lib
    header = (ROOT / "include" / "gelly_hip.h").read_text()
    assert "typedef struct gs_cont gs_cont;" in header
    structs = {"gs_edge_batch": "GsEdgeBatch", "gs_vertex_out": "GsVertexOut", "gs_partial_batch": "GsPartialBatch"}
    lines, want = [], []
    for c_name, py_name in structs.items():
        t = getattr(_lib, py_name)
        lines.append(f'printf("%zu\\n", sizeof({c_name}));')
        want.append(ctypes.sizeof(t))
        for f, _ in t._fields_:
            lines.append(f'printf("%zu\\n", offsetof({c_name}, {f}));')
            want.append(getattr(t, f).offset)
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gelly_hip.h\"\nint main(){" + "".join(lines) + "}"
    tmp = tmp_path
    (tmp / "sz_cont.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp / "sz_cont.c"), "-o", str(tmp / "sz_cont")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp / "sz_cont")], capture_output=True, text=True).stdout.split()]
    assert got == want


def test_cont_entry_points_reject_null_handles_without_a_device(pkg):
    from gelly_streaming_amd import _lib
    lib = pkg.load_library()
    h = ctypes.c_void_p()
    assert lib.gs_cont_create(None, 0, ctypes.byref(h)) == _lib.GS_EINVAL and not h.value
    d, r = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.gs_cont_size(None, ctypes.byref(d), ctypes.byref(r)) == _lib.GS_EINVAL
    assert lib.gs_cont_capacity(None, ctypes.byref(d), ctypes.byref(r)) == _lib.GS_EINVAL
    n_out = ctypes.c_uint64(0)
    vo = _lib.GsVertexOut(None, None, 0, ctypes.pointer(n_out), _lib.GS_MEM_HOST, 0)
    b = _lib.GsEdgeBatch(None, None, None, 0, _lib.GS_NONE, _lib.GS_MEM_HOST, 0)
    assert lib.gs_cont_degrees(None, None, ctypes.byref(b), 2, ctypes.byref(vo)) == _lib.GS_EINVAL
    assert lib.gs_cont_vertices(None, None, ctypes.byref(b), ctypes.byref(vo)) == _lib.GS_EINVAL
    assert lib.gs_cont_export(None, None, ctypes.byref(vo)) == _lib.GS_EINVAL
    assert lib.gs_cont_import(None, None, None) == _lib.GS_EINVAL
    lib.gs_cont_destroy(None)   # a no-op, like free(NULL)


def test_api_surface(pkg):
    for name in ("getDegrees", "getInDegrees", "getOutDegrees", "getVertices", "numberOfVertices", "numberOfEdges"):
        assert callable(getattr(pkg.SimpleEdgeStream, name))
    assert callable(pkg.Engine.continuous) and pkg.ContinuousState is not None
    env = pkg.StreamExecutionEnvironment()
    assert env.getMicroBatch() is None and env.setMicroBatch(3).getMicroBatch() == 3
    with pytest.raises(ValueError):
        env.setMicroBatch(0)
    # numberOfEdges is host arithmetic: no engine is created for it
    e = FIX["edges"]
    g = pkg.SimpleEdgeStream(env.fromCollection(e), env)
    assert ref.lines(g.numberOfEdges().collect()) == sorted(FIX["numberOfEdges"])
    assert g.numberOfEdges().collect() == [1, 2, 3, 4, 5, 6, 7] and env._engine is None
