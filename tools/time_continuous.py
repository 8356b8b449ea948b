"""Time of the continuous operators per micro-batch (not a bench line): gs_cont_degrees and gs_cont_vertices
on an R-MAT scale-22 stream cut into 8 batches of 2^22 edges (device columns, preallocated outputs,
GS_DIR_ALL), against gs_window_csr with ALL on the same batches in the same process -- the same sort_window
followed by a gather.  Device events around each call, after a warm-up pass over every batch; the three calls
alternate batch by batch.  Two timed passes: states that start empty (the table grows while the stream
runs) and states created with room for the stream's vertices (no growth).  Prints one JSON line.

    python tools/time_continuous.py [--scale 22] [--batches 8] [--log2-batch 22] [--passes 3]"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import __graft_entry__ as ge  # noqa: E402

ALL = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--log2-batch", type=int, default=22)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    pkg = ge.load_package()
    L = pkg._lib
    eng = pkg.Engine(0)
    lib = eng._L
    n, R = 1 << a.log2_batch, 2 << a.log2_batch
    cols = [eng.generate_rmat(a.scale, n, 0x5EEDC2, first_edge=k * n) for k in range(a.batches)]
    dev = "cuda:0"
    ok, ov = torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, dtype=torch.int64, device=dev)
    ck, cn = torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, dtype=torch.int64, device=dev)
    co = torch.empty(R + 1, dtype=torch.int64, device=dev)
    n_out, nv, nr = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    vo = L.GsVertexOut(ok.data_ptr(), ov.data_ptr(), R, ctypes.pointer(n_out), L.GS_MEM_DEVICE, 0)
    cso = L.GsCsrOut(ck.data_ptr(), co.data_ptr(), cn.data_ptr(), None, R, R, ctypes.pointer(nv), ctypes.pointer(nr),
                     L.GS_MEM_DEVICE, 0)
    batches = [L.GsEdgeBatch(s.data_ptr(), d.data_ptr(), None, n, L.GS_NONE, L.GS_MEM_DEVICE, 0) for s, d in cols]

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = f()
        e1.record()
        e1.synchronize()
        if st != L.GS_OK:
            raise pkg.GsError(st, lib.gs_last_error(eng.ctx).decode())
        return e0.elapsed_time(e1)

    runs_per_batch = []

    def one_pass(reserve):
        """every batch through csr, a degree state and a vertex state; per-batch ms of each, the states' sizes"""
        sd, sv = eng.continuous(reserve), eng.continuous(reserve)
        ms = {"csr": [], "degrees": [], "vertices": []}
        runs_per_batch.clear()
        for b in batches:
            ms["csr"].append(timed(lambda: lib.gs_window_csr(eng.ctx, ctypes.byref(b), ALL, ctypes.byref(cso))))
            runs_per_batch.append(nv.value)   # the batch's distinct vertices: the lanes of the table kernel
            ms["degrees"].append(timed(lambda: lib.gs_cont_degrees(eng.ctx, sd.handle, ctypes.byref(b), ALL, ctypes.byref(vo))))
            ms["vertices"].append(timed(lambda: lib.gs_cont_vertices(eng.ctx, sv.handle, ctypes.byref(b), ctypes.byref(vo))))
        info = {"distinct": sd.size()[0], "records": sd.size()[1], "slots": sd.capacity()[0], "growths": sd.capacity()[1]}
        sd.close()
        sv.close()
        return ms, info

    _, info = one_pass(0)   # warm-up: every shape once (code objects, workspace), and the stream's vertex count
    out = {"scale": a.scale, "batches": a.batches, "edges_per_batch": n, "records_per_batch": R, "passes": a.passes,
           "distinct_per_batch": list(runs_per_batch)}
    for name, reserve in (("growing", 0), ("reserved", 2 * info["distinct"])):
        runs = [one_pass(reserve) for _ in range(a.passes)]
        res = {}
        for k in ("csr", "degrees", "vertices"):
            per_batch = [statistics.median(r[0][k][i] for r in runs) for i in range(a.batches)]
            total = [sum(r[0][k]) for r in runs]
            res[k] = {"ms_per_batch": [round(x, 3) for x in per_batch], "ms_stream_min_med_max":
                      [round(min(total), 3), round(statistics.median(total), 3), round(max(total), 3)],
                      "records_per_s": round(a.batches * R / (statistics.median(total) * 1e-3))}
        for k in ("degrees", "vertices"):
            res[k]["ratio_to_csr"] = round(res[k]["ms_stream_min_med_max"][1] / res["csr"]["ms_stream_min_med_max"][1], 3)
        st = runs[-1][1]
        res["table"] = dict(st, load_factor=round(st["distinct"] / st["slots"], 4))
        out[name] = res
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
