"""CPU: the plain-Python restatement of aggregate / globalAggregate (tests/aggregate_ref.py) is pinned to the
reference's own degree golden, its Java arithmetic is checked on the special values, and the new ABI surface is
sound without a device."""
import ctypes
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aggregate_ref as ref
import continuous_ref as cref

ROOT = Path(__file__).resolve().parent.parent
FIX = json.loads((Path(__file__).parent / "golden" / "continuous_fixtures.json").read_text())
ENTRY_POINTS = ("gs_agg_create", "gs_agg_destroy", "gs_agg_size", "gs_agg_capacity", "gs_agg_edges", "gs_agg_global",
                "gs_agg_export", "gs_agg_import")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _plain(rows):
    return [(k, v.item()) for k, v in rows]


@pytest.mark.parametrize("direction,case", [(ref.IN, "getInDegrees"), (ref.OUT, "getOutDegrees"), (ref.ALL, "getDegrees")])
def test_count_is_the_degree_stream(direction, case):
    """aggregate(DegreeTypeSeparator, DegreeMapFunction) is getDegrees: TestGetDegrees' golden pins the restatement."""
    got = _plain(ref.aggregate(FIX["edges"], ref.COUNT, "i64", direction))
    assert got == cref.get_degrees(FIX["edges"], direction)
    assert cref.lines(got) == sorted(FIX[case])


def test_global_count_with_updates_is_number_of_edges():
    got = [v.item() for v in ref.global_aggregate(FIX["edges"], ref.COUNT, "i64", ref.OUT, True)]
    assert got == cref.number_of_edges(FIX["edges"]) and cref.lines(got) == sorted(FIX["numberOfEdges"])


def test_sum_min_max_on_the_fixture():
    e = FIX["edges"]
    assert _plain(ref.aggregate(e, ref.SUM, "i64", ref.OUT)) == [(1, 12), (1, 25), (2, 23), (3, 34), (3, 69), (4, 45), (5, 51)]
    assert _plain(ref.aggregate(e, ref.MAX, "i64", ref.IN)) == [(2, 12), (3, 13), (3, 23), (4, 34), (5, 35), (5, 45), (1, 51)]
    assert _plain(ref.aggregate(e, ref.MIN, "i32", ref.ALL))[:6] == [(1, 12), (2, 12), (1, 12), (3, 13), (2, 12), (3, 13)]
    assert [v.item() for v in ref.global_aggregate(e, ref.MAX, "i64", ref.ALL, True)] == [12, 13, 23, 34, 35, 45, 51]
    assert [v.item() for v in ref.global_aggregate(e, ref.MIN, "i64", ref.ALL, True)] == [12]
    assert len(ref.global_aggregate(e, ref.MIN, "i64", ref.ALL, False)) == 14


def _bits(x):
    return x.tobytes()


def test_nan_signed_zero_and_wrap():
    f = np.float64
    nan, nz, pz = f("nan"), f(-0.0), f(0.0)
    # Math.min / Math.max: NaN wins from either side, -0.0 < +0.0
    for op in (ref.MIN, ref.MAX):
        assert np.isnan(ref.combine(op, nan, f(1))) and np.isnan(ref.combine(op, f(1), nan))
    assert _bits(ref.combine(ref.MIN, pz, nz)) == _bits(nz) and _bits(ref.combine(ref.MIN, nz, pz)) == _bits(nz)
    assert _bits(ref.combine(ref.MAX, pz, nz)) == _bits(pz) and _bits(ref.combine(ref.MAX, nz, pz)) == _bits(pz)
    # a NaN, then a smaller value: the accumulator stays NaN
    rows = ref.KeyedState(ref.MIN, "f32").edges([1, 1, 1], [0, 0, 0], [5.0, float("nan"), 1.0], ref.OUT)
    assert rows[0][1] == 5 and np.isnan(rows[1][1]) and np.isnan(rows[2][1])
    # +inf then -inf under SUM: NaN from there on
    rows = ref.KeyedState(ref.SUM, "f64").edges([1] * 3, [0] * 3, [float("inf"), float("-inf"), 1.0], ref.OUT)
    assert rows[0][1] == np.inf and np.isnan(rows[1][1]) and np.isnan(rows[2][1])
    # a first -0.0 is the accumulator unchanged; -0.0 + -0.0 = -0.0; -0.0 + 0.0 = +0.0
    rows = ref.KeyedState(ref.SUM, "f32").edges([1] * 3, [0] * 3, [-0.0, -0.0, 0.0], ref.OUT)
    assert [_bits(v) for _, v in rows] == [_bits(np.float32(-0.0)), _bits(np.float32(-0.0)), _bits(np.float32(0.0))]
    # integer sums wrap at their own width
    rows = ref.KeyedState(ref.SUM, "i64").edges([1] * 3, [0] * 3, [I64_MAX, 1, I64_MIN], ref.OUT)
    assert _plain(rows) == [(1, I64_MAX), (1, I64_MIN), (1, 0)]
    rows = ref.KeyedState(ref.SUM, "i32").edges([1] * 2, [0] * 2, [2**31 - 1, 1], ref.OUT)
    assert _plain(rows) == [(1, 2**31 - 1), (1, -2**31)] and rows[1][1].dtype == np.int32
    # float32 sums round at every step
    rows = ref.KeyedState(ref.SUM, "f32").edges([1] * 3, [0] * 3, [2.0**24, 1.0, 1.0], ref.OUT)
    assert rows[2][1] == np.float32(2.0**24) and rows[2][1].dtype == np.float32


def test_update_filter_is_java_equals():
    f = np.float64
    assert ref.java_equals(f("nan"), f("nan")) and not ref.java_equals(f(0.0), f(-0.0)) and not ref.java_equals(f(1), None)
    # a running MAX emits the record highs only, each once
    g = ref.GlobalState(ref.MAX, "i64")
    rows = g.run([1, 2, 3, 4, 5, 6], [0] * 6, [3, 1, 3, 7, 7, 2], ref.OUT, True)
    assert _plain(rows) == [(1, 3), (4, 7)]
    # a cut inside a plateau emits nothing twice: previousValue is the latest running value
    assert _plain(g.run([7, 8], [0, 0], [7, 9], ref.OUT, True)) == [(8, 9)]
    # 0.0 and -0.0 differ; NaN equals NaN
    g = ref.GlobalState(ref.MIN, "f64")
    rows = g.run([1, 2, 3, 4, 5], [0] * 5, [0.0, -0.0, -0.0, float("nan"), float("nan")], ref.OUT, True)
    assert [k for k, _ in rows] == [1, 2, 4]


# ---- the ABI surface, without a device ---------------------------------------------------------------------
def test_header_declares_the_entry_points_and_modes():
    header = (ROOT / "include" / "gelly_hip.h").read_text()
    names = set(re.findall(r"^GS_API\s+[\w\s\*]+?\b(gs_\w+)\s*\(", header, re.M))
    assert set(ENTRY_POINTS) <= names
    assert "typedef struct gs_agg gs_agg;" in header


def test_enum_values_and_struct_layouts_match_lib(pkg, tmp_path):
    """the C compiler's values of the enums the new entry points take, and the layouts of the structs they share"""
    from gelly_streaming_amd import _lib
    consts = ["GS_AGG_KEYED", "GS_AGG_GLOBAL", "GS_OP_SUM", "GS_OP_MIN", "GS_OP_MAX", "GS_OP_COUNT", "GS_I32", "GS_I64",
              "GS_F32", "GS_F64", "GS_NONE", "GS_DIR_IN", "GS_DIR_OUT", "GS_DIR_ALL", "GS_EINVAL", "GS_ECAPACITY"]
    want = [getattr(_lib, c) if hasattr(_lib, c) else {"GS_DIR_IN": 0, "GS_DIR_OUT": 1, "GS_DIR_ALL": 2}[c] for c in consts]
    lines = [f'printf("%d\\n", (int){c});' for c in consts]
    for cname, t in (("gs_vertex_out", _lib.GsVertexOut), ("gs_partial_batch", _lib.GsPartialBatch),
                     ("gs_edge_batch", _lib.GsEdgeBatch)):
        lines.append(f'printf("%zu\\n", sizeof({cname}));')
        want.append(ctypes.sizeof(t))
        for f, _ in t._fields_:
            lines.append(f'printf("%zu\\n", offsetof({cname}, {f}));')
            want.append(getattr(t, f).offset)
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"gelly_hip.h\"\nint main(){" + "".join(lines) + "}"
    (tmp_path / "sz_ag.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(tmp_path / "sz_ag.c"), "-o", str(tmp_path / "sz_ag")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "sz_ag")], capture_output=True, text=True).stdout.split()]
    assert got == want


def test_entry_points_reject_null_handles_without_a_device(pkg):
    from gelly_streaming_amd import _lib
    lib = pkg.load_library()
    a, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.gs_agg_size(None, ctypes.byref(a), ctypes.byref(b)) == _lib.GS_EINVAL
    assert lib.gs_agg_capacity(None, ctypes.byref(a), ctypes.byref(b)) == _lib.GS_EINVAL
    lib.gs_agg_destroy(None)
    h = ctypes.c_void_p()
    assert lib.gs_agg_create(None, 0, 0, 1, 0, ctypes.byref(h)) == _lib.GS_EINVAL and not h.value
    n = ctypes.c_uint64(0)
    vo = _lib.GsVertexOut(None, None, 0, ctypes.pointer(n), _lib.GS_MEM_HOST, 0)
    eb = _lib.GsEdgeBatch(None, None, None, 0, _lib.GS_I64, _lib.GS_MEM_HOST, 0)
    assert lib.gs_agg_edges(None, None, ctypes.byref(eb), 2, ctypes.byref(vo)) == _lib.GS_EINVAL
    assert lib.gs_agg_global(None, None, ctypes.byref(eb), 2, 1, ctypes.byref(vo)) == _lib.GS_EINVAL
    assert lib.gs_agg_export(None, None, ctypes.byref(vo)) == _lib.GS_EINVAL
    pb = _lib.GsPartialBatch(None, None, None, 0, _lib.GS_I64, _lib.GS_MEM_HOST)
    assert lib.gs_agg_import(None, None, ctypes.byref(pb), 0) == _lib.GS_EINVAL


def test_api_surface_and_host_mappers(pkg):
    assert callable(pkg.SimpleEdgeStream.globalAggregate) and callable(pkg.Engine.aggregate_state)
    for name in ("edges", "global_", "size", "capacity", "export", "load", "close"):
        assert callable(getattr(pkg.AggregateState, name))
    sep = pkg.EdgeValueSeparator(True, True)
    out = pkg.Collector()
    sep.flatMap((1, 2, 12), out)
    assert out.records == [(1, 12), (2, 12)] and sep.direction == 2
    assert pkg.EdgeValueSeparator(True, False).direction == 0 and pkg.EdgeValueSeparator(False, True).direction == 1
    # the built-in mappers' own host code agrees with the restatement (it documents what the device runs)
    for cls, op in ((pkg.RunningSum, ref.SUM), (pkg.RunningMin, ref.MIN), (pkg.RunningMax, ref.MAX), (pkg.RunningCount, ref.COUNT)):
        m, recs = cls(), [(k, np.int64(v)) for k, v in ref.expand(*zip(*FIX["edges"]), ref.ALL)]
        assert [(k, int(v)) for k, v in map(m.map, recs)] == _plain(ref.aggregate(FIX["edges"], op, "i64", ref.ALL))
    g, out = pkg.GlobalRunningMax(), pkg.Collector()
    for r in ref.expand(*zip(*FIX["edges"]), ref.OUT):
        g.flatMap(r, out)
    assert out.records == [12, 13, 23, 34, 35, 45, 51]
