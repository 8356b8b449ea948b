"""Time of the running aggregates on a stream (not a bench line): gs_agg_edges / gs_agg_global against
gs_cont_degrees on the same batches.  An R-MAT stream generated on the device goes through one state per case in
batches of --batch-edges; device columns, preallocated device outputs.  Batch by batch every case takes its call in
turn (so the cases alternate inside one run), each call timed by a host clock around the call and a stream
synchronise.  The first batch is the warm-up; prints the medians over the others as one JSON line, each case's
median over gs_cont_degrees' as `vs_cont_degrees`.  gs_cont_degrees is the running COUNT the library had before
gs_agg_*: its median is the yardstick.  GELLY_HIP_LIB selects the library.

    python tools/time_aggregate.py [--scale 22] [--edge-factor 16] [--batch-edges 4194304] [--only NAME]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import __graft_entry__ as ge  # noqa: E402

ALL = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--batch-edges", type=int, default=1 << 22)
    ap.add_argument("--only", default=None, help="one case (and gs_cont_degrees), e.g. for a kernel trace")
    a = ap.parse_args()
    pkg = ge.load_package()
    L = pkg._lib
    eng = pkg.Engine(0)
    n, mb = a.edge_factor << a.scale, a.batch_edges
    src, dst = eng.generate_rmat(a.scale, n, 0x5EEDA6)
    vl = eng.generate_values(n, 0x5EEDA7, L.GS_I64)
    vd = (vl % 1024).to(torch.float64) / 8.0 + 1.0
    R = 2 * mb
    out = {dt: (torch.empty(R, dtype=torch.int64, device=src.device), torch.empty(R, dtype=dt, device=src.device))
           for dt in (torch.int64, torch.float64)}
    cases = {
        "cont_degrees": (eng.continuous(), None, None),
        "count_all": (eng.aggregate_state(L.GS_OP_COUNT, None), None, None),
        "long_sum_all": (eng.aggregate_state(L.GS_OP_SUM, L.GS_I64), vl, None),
        "double_sum_all": (eng.aggregate_state(L.GS_OP_SUM, L.GS_F64), vd, None),
        "long_max_all": (eng.aggregate_state(L.GS_OP_MAX, L.GS_I64), vl, None),
        "global_long_max_updates_all": (eng.aggregate_state(L.GS_OP_MAX, L.GS_I64, mode="global"), vl, True),
    }
    if a.only:
        cases = {k: c for k, c in cases.items() if k in ("cont_degrees", a.only)}
    times = {k: [] for k in cases}
    kept = {k: 0 for k in cases}
    for lo in range(0, n, mb):
        s, d = src[lo:lo + mb], dst[lo:lo + mb]
        for name, (state, val, collect) in cases.items():
            v = None if val is None else val[lo:lo + mb]
            o = out[torch.float64 if val is vd else torch.int64]
            eng.synchronize()
            t0 = time.perf_counter()
            if name == "cont_degrees":
                k, x = state.degrees(s, d, ALL, out=o)
            elif collect is None:
                k, x = state.edges(s, d, v, ALL, out=o)
            else:
                k, x = state.global_(s, d, v, ALL, collect, out=o)
            eng.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            kept[name] += len(x)
    res = {"scale": a.scale, "edges": n, "batch_edges": mb, "records_per_batch": R, "batches_timed": len(times["cont_degrees"]) - 1,
           "lib": Path(L.LIB_PATH).name}
    base = statistics.median(times["cont_degrees"][1:])
    for name, (state, _, _) in cases.items():
        t = times[name][1:]   # the first batch is the warm-up
        med = statistics.median(t)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                     "records_per_s": round(R / med * 1e3), "vs_cont_degrees": round(med / base, 4),
                     "records_out": kept[name], "vertices": state.size()[0]}
        state.close()
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
