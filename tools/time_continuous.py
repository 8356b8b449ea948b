"""Time of the continuous operators per micro-batch (not a bench line): gs_cont_degrees, gs_cont_vertices and
gs_distinct_edges (KEYED; src, dst and index columns out)
on an R-MAT scale-22 stream cut into 8 batches of 2^22 edges (device columns, preallocated outputs,
GS_DIR_ALL), against gs_window_csr with ALL on the same batches in the same process -- the same sort_window
followed by a gather.  Device events around each call, after a warm-up pass over every batch; the four calls
alternate batch by batch.  Two timed passes: states that start empty (the tables grow while the stream
runs) and states created with room for the stream's vertices / edges (no growth).  Prints one JSON line.
The `matching` leg: gs_match_edges (all five event columns out, room for 3n events) on the same batches with
16-bit values, a cold state and then a second pass of the same stream over the warm state -- per batch ms,
edges/s, rounds, blocking iterations, edges pending after rounds 1, 2, 4 and 8, events, and the ratio to
gs_window_csr -- next to one host thread running tools/matching_cpu.cpp on the same stream.
The `assign` leg: gs_assign_edges (vertex, label and edge columns out) on the same batches, a cold state and then
a second pass of the same stream over the warm state, --passes times over; per batch the median ms, edges/s,
rounds, records and the edges live after rounds 1, 2, 4 and 8.  In the same process, alternating batch by batch:
gs_window_components on the batch with the previous call's output fed back as `prev` (the way to the same
information today: it re-emits every vertex) and gs_window_csr; and one host thread running tools/assign_cpu.cpp.

    python tools/time_continuous.py [--scale 22] [--batches 8] [--log2-batch 22] [--passes 3]"""
import argparse
import ctypes
import json
import statistics
import subprocess
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
    ap.add_argument("--legs", default="tables,trisample,matching")
    ap.add_argument("--samples", default="10000,1000000")
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
    es, ed, ei = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3))
    ne = ctypes.c_uint64(0)
    eo = L.GsEdgeOut(es.data_ptr(), ed.data_ptr(), None, ei.data_ptr(), n, ctypes.pointer(ne), L.GS_MEM_DEVICE, 0)
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

    runs_per_batch, kept_per_batch = [], []

    def one_pass(reserve, reserve_edges=0):
        """every batch through csr, a degree state, a vertex state and an edge set; per-batch ms of each, the
        states' sizes"""
        sd, sv, se = eng.continuous(reserve), eng.continuous(reserve), eng.distinct("keyed", reserve_edges)
        ms = {"csr": [], "degrees": [], "vertices": [], "distinct": []}
        runs_per_batch.clear()
        kept_per_batch.clear()
        for b in batches:
            ms["csr"].append(timed(lambda: lib.gs_window_csr(eng.ctx, ctypes.byref(b), ALL, ctypes.byref(cso))))
            runs_per_batch.append(nv.value)   # the batch's distinct vertices: the lanes of the table kernel
            ms["degrees"].append(timed(lambda: lib.gs_cont_degrees(eng.ctx, sd.handle, ctypes.byref(b), ALL, ctypes.byref(vo))))
            ms["vertices"].append(timed(lambda: lib.gs_cont_vertices(eng.ctx, sv.handle, ctypes.byref(b), ctypes.byref(vo))))
            ms["distinct"].append(timed(lambda: lib.gs_distinct_edges(eng.ctx, se.handle, ctypes.byref(b), ctypes.byref(eo))))
            kept_per_batch.append(ne.value)
        einfo = {"distinct": se.size()[0], "records": se.size()[1], "slots": se.capacity()[0], "growths": se.capacity()[1]}
        se.close()
        info = {"distinct": sd.size()[0], "records": sd.size()[1], "slots": sd.capacity()[0], "growths": sd.capacity()[1]}
        sd.close()
        sv.close()
        return ms, info, einfo

    def trisample_pass(samples):
        """every batch through csr and a fresh sampler state; per-batch ms of each, records per batch, the state's size"""
        st = eng.triangle_sampler("broadcast", samples, 1 << a.scale, 0x5A3)
        ms, recs = {"csr": [], "trisample": []}, []
        for b in batches:
            ms["csr"].append(timed(lambda: lib.gs_window_csr(eng.ctx, ctypes.byref(b), ALL, ctypes.byref(cso))))
            ms["trisample"].append(timed(lambda: lib.gs_trisample_edges(eng.ctx, st.handle, ctypes.byref(b), ctypes.byref(vo))))
            recs.append(n_out.value)
        size = st.size()
        st.close()
        return ms, recs, size

    def matching_leg():
        """a cold state, then the same stream again over the warm state; one host thread on the same stream"""
        import numpy as np

        vals = [eng.generate_values(n, 0x5EEDC3, first_edge=k * n) & 0xFFFF for k in range(a.batches)]
        mb = [L.GsEdgeBatch(s.data_ptr(), d.data_ptr(), v.data_ptr(), n, L.GS_I64, L.GS_MEM_DEVICE, 0)
              for (s, d), v in zip(cols, vals)]
        mt = torch.empty(3 * n, dtype=torch.uint8, device=dev)
        ms_, md, mv, mi = (torch.empty(3 * n, dtype=torch.int64, device=dev) for _ in range(4))
        nm = ctypes.c_uint64(0)
        mo = L.GsMatchOut(mt.data_ptr(), ms_.data_ptr(), md.data_ptr(), mv.data_ptr(), mi.data_ptr(), 3 * n, ctypes.pointer(nm),
                          L.GS_MEM_DEVICE, 0)
        with eng.weighted_matching() as w:     # warm-up: code objects and workspace, on one batch
            timed(lambda: lib.gs_match_edges(eng.ctx, w.handle, ctypes.byref(mb[0]), ctypes.byref(mo)))
        res = {}
        st = eng.weighted_matching((1 << a.scale) + 2 * n)      # no table growth inside the timed calls
        for name in ("cold", "warm"):
            rows = []
            for b, bm in zip(batches, mb):
                csr = timed(lambda: lib.gs_window_csr(eng.ctx, ctypes.byref(b), ALL, ctypes.byref(cso)))
                ms = timed(lambda: lib.gs_match_edges(eng.ctx, st.handle, ctypes.byref(bm), ctypes.byref(mo)))
                info = st.last_batch()
                rows.append({"ms": round(ms, 3), "edges_per_s": round(n / (ms * 1e-3)), "csr_ms": round(csr, 3),
                             "ratio_to_csr": round(ms / csr, 2), "rounds": info["rounds"],
                             "block_iterations": info["block_iterations"],
                             "pending_after": {str(k): v for k, v in info["pending_after"].items()}, "events": nm.value})
            total = sum(r["ms"] for r in rows)
            res[name] = {"per_batch": rows, "ms_stream": round(total, 3), "edges_per_s": round(a.batches * n / (total * 1e-3)),
                         "ratio_to_csr": round(total / sum(r["csr_ms"] for r in rows), 2)}
        res["matched_edges"], res["records"], res["total_weight"] = st.size()
        st.close()
        # one host thread (the reference's parallelism for this operator) on the same stream
        root = Path(__file__).resolve().parent
        exe, cpp = root / "matching_cpu", root / "matching_cpu.cpp"
        if not exe.exists() or exe.stat().st_mtime < cpp.stat().st_mtime:      # never time a stale binary
            subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(cpp)], check=True)
        # the stream goes down a pipe, column by column (it prints only after it has read everything)
        proc = subprocess.Popen([str(exe), "-", str(n), str(a.batches), "2"], stdin=subprocess.PIPE, stdout=subprocess.PIPE)
        for part in ([s for s, _ in cols], [d for _, d in cols], vals):
            for t in part:
                proc.stdin.write(t.cpu().numpy().astype(np.int64).tobytes())
        proc.stdin.close()
        text = proc.stdout.read()
        if proc.wait() != 0:
            raise RuntimeError(f"matching_cpu ended with status {proc.returncode}")
        cpu = json.loads(text)
        for name, p in zip(("cold", "warm"), cpu["passes"]):
            total = sum(p["ms_per_batch"])
            if p["events_per_batch"] != [r["events"] for r in res[name]["per_batch"]]:
                raise RuntimeError(f"matching: the host restatement counts other events on the {name} pass")
            res[name]["cpu_one_thread"] = {"ms_per_batch": p["ms_per_batch"], "ms_stream": round(total, 3),
                                           "edges_per_s": round(a.batches * n / (total * 1e-3))}
            res[name]["gpu_over_cpu_time"] = round(res[name]["ms_stream"] / total, 3)
            res[name]["faster"] = "gpu" if res[name]["ms_stream"] < total else "one cpu thread"
        return res

    def assign_leg():
        """cold and warm passes of gs_assign_edges next to gs_window_components with its state fed back and
        gs_window_csr, alternating batch by batch; medians over a.passes repetitions; one host thread"""
        import numpy as np

        room = [2 * n]      # records per batch depend on the data: the columns grow when a call asks for more
        cols_out = []
        na = ctypes.c_uint64(0)

        def columns():
            cols_out[:] = [torch.empty(room[0], dtype=torch.int64, device=dev), torch.empty(room[0], dtype=torch.int64, device=dev),
                           torch.empty(room[0], dtype=torch.uint32, device=dev)]
            return L.GsAssignOut(cols_out[0].data_ptr(), cols_out[1].data_ptr(), cols_out[2].data_ptr(), room[0],
                                 ctypes.pointer(na), L.GS_MEM_DEVICE, 0)

        ao = [columns()]

        def assign_call(st, b):
            """the batch's ms; a call that asks for more room changes nothing and is timed again with it"""
            for _ in range(2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                status = lib.gs_assign_edges(eng.ctx, st.handle, ctypes.byref(b), ctypes.byref(ao[0]))
                e1.record()
                e1.synchronize()
                if status != L.GS_ECAPACITY:
                    break
                room[0] = na.value + na.value // 8
                ao[0] = columns()
            if status != L.GS_OK:
                raise pkg.GsError(status, lib.gs_last_error(eng.ctx).decode())
            return e0.elapsed_time(e1)

        V = 1 << a.scale
        pk = [torch.empty(V + 2 * n + 1, dtype=torch.int64, device=dev) for _ in range(4)]   # components: prev / out, ping-pong
        ncc = ctypes.c_uint64(0)

        def one_run():
            st = eng.assign_components(V + 2 * n)      # no table growth inside the timed calls
            res, m, flip = {}, 0, 0
            for name in ("cold", "warm"):
                rows = []
                for b in batches:
                    csr = timed(lambda: lib.gs_window_csr(eng.ctx, ctypes.byref(b), ALL, ctypes.byref(cso)))
                    prev = L.GsPartialBatch(pk[flip].data_ptr(), pk[flip + 1].data_ptr(), None, m, L.GS_I64, L.GS_MEM_DEVICE)
                    co_ = L.GsVertexOut(pk[2 - flip].data_ptr(), pk[3 - flip].data_ptr(), V + 2 * n + 1, ctypes.pointer(ncc),
                                        L.GS_MEM_DEVICE, 0)
                    cc = timed(lambda: lib.gs_window_components(eng.ctx, ctypes.byref(b), ctypes.byref(prev) if m else None,
                                                                ctypes.byref(co_)))
                    m, flip = ncc.value, 2 - flip
                    ms = assign_call(st, b)
                    info = st.last_batch()
                    rows.append({"ms": ms, "csr_ms": csr, "components_ms": cc, "rounds": info["rounds"],
                                 "merging_edges": info["merging_edges"], "records": info["records"],
                                 "live_after": {str(k): v for k, v in info["live_after"].items()}})
                res[name] = rows
            size = st.size()
            if size[0] != m:
                raise RuntimeError(f"assign: {size[0]} vertices, gs_window_components kept {m}")
            st.close()
            return res, size

        with eng.assign_components() as w:     # warm-up: code objects and workspace, on one batch
            assign_call(w, batches[0])
        one_run()
        runs = [one_run() for _ in range(a.passes)]
        res = {}
        for name in ("cold", "warm"):
            rows = []
            for i in range(a.batches):
                r = dict(runs[-1][0][name][i])
                for k in ("ms", "csr_ms", "components_ms"):
                    r[k] = round(statistics.median(run[0][name][i][k] for run in runs), 3)
                r["edges_per_s"] = round(n / (r["ms"] * 1e-3))
                r["ratio_to_components"] = round(r["ms"] / r["components_ms"], 3)
                rows.append(r)
            tot = {k: sum(r[k] for r in rows) for k in ("ms", "csr_ms", "components_ms")}
            res[name] = {"per_batch": rows, "ms_stream": round(tot["ms"], 3), "components_ms_stream": round(tot["components_ms"], 3),
                         "csr_ms_stream": round(tot["csr_ms"], 3), "edges_per_s": round(a.batches * n / (tot["ms"] * 1e-3)),
                         "ratio_to_components": round(tot["ms"] / tot["components_ms"], 3),
                         "ratio_to_csr": round(tot["ms"] / tot["csr_ms"], 3)}
        res["vertices"], res["components"], res["records"] = runs[-1][1]
        # one host thread (the reference's parallelism for this operator) on the same stream
        root = Path(__file__).resolve().parent
        exe, cpp = root / "assign_cpu", root / "assign_cpu.cpp"
        if not exe.exists() or exe.stat().st_mtime < cpp.stat().st_mtime:      # never time a stale binary
            subprocess.run(["g++", "-O2", "-std=c++17", "-o", str(exe), str(cpp)], check=True)
        proc = subprocess.Popen([str(exe), "-", str(n), str(a.batches), "2"], stdin=subprocess.PIPE, stdout=subprocess.PIPE)
        for part in ([s for s, _ in cols], [d for _, d in cols]):
            for t in part:
                proc.stdin.write(t.cpu().numpy().astype(np.int64).tobytes())
        proc.stdin.close()
        text = proc.stdout.read()
        if proc.wait() != 0:
            raise RuntimeError(f"assign_cpu ended with status {proc.returncode}")
        cpu = json.loads(text)
        for name, p in zip(("cold", "warm"), cpu["passes"]):
            total = sum(p["ms_per_batch"])
            if p["records_per_batch"] != [r["records"] for r in res[name]["per_batch"]]:
                raise RuntimeError(f"assign: the host restatement counts other records on the {name} pass")
            res[name]["cpu_one_thread"] = {"ms_per_batch": p["ms_per_batch"], "ms_stream": round(total, 3),
                                           "edges_per_s": round(a.batches * n / (total * 1e-3))}
            res[name]["gpu_over_cpu_time"] = round(res[name]["ms_stream"] / total, 3)
        return res

    legs = a.legs.split(",")
    out = {"scale": a.scale, "batches": a.batches, "edges_per_batch": n, "records_per_batch": R, "passes": a.passes}
    if "matching" in legs:
        out["matching"] = matching_leg()
    if "assign" in legs:
        out["assign"] = assign_leg()
    if "trisample" in legs:
        out["trisample"] = {}
        for samples in (int(x) for x in a.samples.split(",")):
            trisample_pass(samples)   # warm-up
            runs = [trisample_pass(samples) for _ in range(a.passes)]
            res = {"records_per_batch": runs[-1][1], "edges_seen": runs[-1][2][0], "beta_sum": runs[-1][2][1]}
            for k in ("csr", "trisample"):
                per_batch = [statistics.median(r[0][k][i] for r in runs) for i in range(a.batches)]
                res[k] = {"ms_per_batch": [round(x, 3) for x in per_batch],
                          "ms_later_batches_median": round(statistics.median(per_batch[1:] or per_batch), 3)}
            res["ratio_to_csr_first_batch"] = round(res["trisample"]["ms_per_batch"][0] / res["csr"]["ms_per_batch"][0], 3)
            res["ratio_to_csr_later_batches"] = round(res["trisample"]["ms_later_batches_median"] /
                                                      res["csr"]["ms_later_batches_median"], 3)
            res["edges_per_s_later_batches"] = round(n / (res["trisample"]["ms_later_batches_median"] * 1e-3))
            out["trisample"][str(samples)] = res
    if "tables" not in legs:
        print(json.dumps(out))
        eng.close()
        return
    _, info, _ = one_pass(0)   # warm-up: every shape once (code objects, workspace), and the stream's vertex count
    out.update({"distinct_per_batch": list(runs_per_batch), "kept_edges_per_batch": list(kept_per_batch)})
    # an edge set that never grows: room for every edge of the stream plus one batch (gs_distinct_create)
    for name, reserve, reserve_edges in (("growing", 0, 0), ("reserved", 2 * info["distinct"], (a.batches + 1) * n)):
        runs = [one_pass(reserve, reserve_edges) for _ in range(a.passes)]
        res = {}
        for k in ("csr", "degrees", "vertices", "distinct"):
            per_batch = [statistics.median(r[0][k][i] for r in runs) for i in range(a.batches)]
            total = [sum(r[0][k]) for r in runs]
            res[k] = {"ms_per_batch": [round(x, 3) for x in per_batch], "ms_stream_min_med_max":
                      [round(min(total), 3), round(statistics.median(total), 3), round(max(total), 3)],
                      "records_per_s": round(a.batches * R / (statistics.median(total) * 1e-3))}
        res["distinct"]["edges_per_s"] = round(a.batches * n / (res["distinct"]["ms_stream_min_med_max"][1] * 1e-3))
        del res["distinct"]["records_per_s"]   # its records are edges (no direction expansion)
        for k in ("degrees", "vertices", "distinct"):
            res[k]["ratio_to_csr"] = round(res[k]["ms_stream_min_med_max"][1] / res["csr"]["ms_stream_min_med_max"][1], 3)
        st = runs[-1][1]
        res["table"] = dict(st, load_factor=round(st["distinct"] / st["slots"], 4))
        et = runs[-1][2]
        res["edge_table"] = dict(et, load_factor=round(et["distinct"] / et["slots"], 4))
        out[name] = res
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
