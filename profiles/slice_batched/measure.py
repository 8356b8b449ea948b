"""Time the per-window loop against the one batched call (gs_slice_reduce) on one MI355X.

    python profiles/slice_batched/measure.py --out DIR [--log2-edges 24] [--reps 5]

Stream: device-resident R-MAT s20, 2^24 edges.  Operators: I64 SUM OUT (Engine.reduce / slice_reduce) and the degree /
max-neighbour fold ALL.  Cuts: W = 2^2, 2^4, ..., 2^16 windows of equal length, timestamps ascending and once
shuffled (the loop then runs on slices split before the clock starts, the batched call on the shuffled columns).
Per W the two paths alternate `reps` times after a warm-up of each, the device synchronised before every clock read,
and their outputs are compared before anything is timed.  Then the whole slice().reduceOnEdges under
setSliceBatching(False) and (True), which adds the host's split of the stream to the loop.
Every repetition goes to DIR/times.json; README.md in this directory is written from it."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SIZE_MS = 10


def clock():
    torch.cuda.synchronize()
    return time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--log2-edges", type=int, default=24)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--api-reps", type=int, default=3)
    ap.add_argument("--max-log2-windows", type=int, default=16)
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    pkg = ge.load_package()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    eng = pkg.Engine(0)
    n = 1 << a.log2_edges
    src, dst = eng.generate_rmat(a.scale, n, 0x51CE)
    val = eng.generate_values(n, 0x51CE)
    OUT, ALL, SUM = pkg.EdgeDirection.OUT, pkg.EdgeDirection.ALL, 0
    ops = {
        "i64_sum_out": (lambda s, d, v: eng.reduce(s, d, v, OUT, SUM),
                        lambda s, d, v, t, W: eng.slice_reduce(s, d, v, t, SIZE_MS, OUT, SUM, windows_hint=W)[2:]),
        "degree_max_all": (lambda s, d, v: eng.fold_degree_max(s, d, ALL),
                           lambda s, d, v, t, W: eng.slice_fold_degree_max(s, d, t, SIZE_MS, ALL, windows_hint=W)[2:]),
    }
    results = {"edges": n, "scale": a.scale, "reps": a.reps, "size_ms": SIZE_MS, "device": torch.cuda.get_device_name(0),
               "cuts": [], "api": []}
    for lw in range(2, a.max_log2_windows + 1, 2):
        W = 1 << lw
        per = n // W
        win = torch.arange(n, device=src.device, dtype=torch.int64) // per
        for order in ("ascending", "shuffled"):
            if order == "ascending":
                s, d, v, t = src, dst, val, win * SIZE_MS
                ls, ld, lv = s, d, v                      # the loop's columns: windows are contiguous slices
            else:
                p = torch.randperm(n, device=src.device, generator=torch.Generator(src.device).manual_seed(lw))
                s, d, v, t = src[p].contiguous(), dst[p].contiguous(), val[p].contiguous(), (win * SIZE_MS)[p].contiguous()
                by_window = torch.sort(win[p], stable=True).indices    # split before the clock starts
                ls, ld, lv = s[by_window].contiguous(), d[by_window].contiguous(), v[by_window].contiguous()
            for name, (one, batched) in ops.items():
                def loop():
                    return [one(ls[w * per:(w + 1) * per], ld[w * per:(w + 1) * per], lv[w * per:(w + 1) * per])
                            for w in range(W)]

                # equal outputs first (this is also each path's warm-up)
                got, want = batched(s, d, v, t, W), loop()
                for c in range(len(got)):
                    assert torch.equal(got[c], torch.cat([r[c] for r in want])), (W, order, name, c)
                del got, want
                loop_s, batch_s = [], []
                for _ in range(a.reps):
                    t0 = clock()
                    loop()
                    t1 = clock()
                    batched(s, d, v, t, W)
                    t2 = clock()
                    loop_s.append(t1 - t0)
                    batch_s.append(t2 - t1)
                row = {"windows": W, "mean_records": per * (2 if name == "degree_max_all" else 1), "order": order,
                       "op": name, "loop_s": loop_s, "batched_s": batch_s,
                       "batched_wins_every_rep": max(batch_s) < min(loop_s)}
                results["cuts"].append(row)
                print(json.dumps(row), flush=True)
                (out / "times.json").write_text(json.dumps(results, indent=1))
    # the whole API call: the loop pays the host's split (numpy argsort of the window starts) on top
    for lw in (4, 10, a.max_log2_windows):
        W = 1 << lw
        per = n // W
        ts = (np.arange(n, dtype=np.int64) // per) * SIZE_MS
        times = {False: [], True: []}
        for rep in range(a.api_reps + 1):     # (the first repetition is the warm-up)
            for mode in (False, True):
                env = pkg.StreamExecutionEnvironment()
                env._engine = eng
                env.setSliceBatching(mode)
                stream = pkg.SimpleEdgeStream(pkg.EdgeColumns(src, dst, val, ts), env)
                t0 = clock()
                res = stream.slice(pkg.Time.milliseconds(SIZE_MS), OUT).reduceOnEdges(pkg.SumReduce())
                t1 = clock()
                assert len(res.windows) == W and env.slice_counts["batched" if mode else "loop"] == 1
                if rep:
                    times[mode].append(t1 - t0)
        row = {"windows": W, "mean_records": per, "op": "slice().reduceOnEdges i64 SUM OUT",
               "loop_s": times[False], "batched_s": times[True]}
        results["api"].append(row)
        print(json.dumps(row), flush=True)
        (out / "times.json").write_text(json.dumps(results, indent=1))
    eng.close()


if __name__ == "__main__":
    main()
