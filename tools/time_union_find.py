"""Time of the two union-find window aggregations on one window (not a bench line): gs_window_bipartite and
gs_window_components over the same ids -- an R-MAT window generated on the device and made bipartite
(src * 2, dst * 2 + 1: it keeps R-MAT's skew), device columns, preallocated device outputs, no previous state.
One warm-up and --windows timed windows of each; prints the medians of the union-find stage (pass_ms[1]) and
of total_ms as one JSON line.  GELLY_HIP_LIB selects the library, so two builds alternate run by run.

    python tools/time_union_find.py [--scale 24] [--edge-factor 16] [--windows 5]"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=24)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    pkg = ge.load_package()
    L = pkg._lib
    eng = pkg.Engine(0)
    lib = eng._L
    n, cap = a.edge_factor << a.scale, (2 << a.scale) + 1
    src, dst = eng.generate_rmat(a.scale, n, 0x5EED05)
    src.mul_(2)
    dst.mul_(2).add_(1)
    dev = src.device
    keys, labels = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)
    signs = torch.empty(cap, dtype=torch.uint8, device=dev)
    n_out, success = ctypes.c_uint64(0), ctypes.c_int32(0)
    batch = L.GsEdgeBatch(src.data_ptr(), dst.data_ptr(), None, n, L.GS_NONE, L.GS_MEM_DEVICE, 0)
    so = L.GsSignedOut(keys.data_ptr(), labels.data_ptr(), signs.data_ptr(), cap, ctypes.pointer(n_out),
                       ctypes.pointer(success), L.GS_MEM_DEVICE, 0)
    vo = L.GsVertexOut(keys.data_ptr(), labels.data_ptr(), cap, ctypes.pointer(n_out), L.GS_MEM_DEVICE, 0)
    calls = {"bipartite": lambda: lib.gs_window_bipartite(eng.ctx, ctypes.byref(batch), None, ctypes.byref(so)),
             "components": lambda: lib.gs_window_components(eng.ctx, ctypes.byref(batch), None, ctypes.byref(vo))}
    out = {"scale": a.scale, "edges": n, "windows": a.windows, "lib": str(L.LIB_PATH)}
    for name, call in calls.items():
        times = []
        for _ in range(a.windows + 1):   # the first is the warm-up
            eng._check(call())
            times.append(eng.stage_times_raw())
        assert name == "components" or success.value == 1
        t = times[1:]
        out[name] = {"vertices": n_out.value, "key_bits": t[0].key_bits,
                     "union_find_ms": round(statistics.median(x.pass_ms[1] for x in t), 4),
                     "total_ms": round(statistics.median(x.total_ms for x in t), 4),
                     "total_ms_all": [round(x.total_ms, 4) for x in t]}
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
