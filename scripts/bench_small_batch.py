"""Small batches: the tree-parallel walk (TI_OPT_SMALL_BATCH_ROWS) against the
forest's own walk, in one process, on bench.py's C2 / C3 / C4 models.

Per model and row count: the answers are compared bit for bit, then ROUNDS
rounds alternate the option off and on.  A round times the host-to-host call
(ti_predict from numpy rows: p50 and p99 over CALLS calls) and a launch on
device-resident rows (LAUNCHES back-to-back launches between two events: at
small sizes the launch rate, not the kernel's own duration).  One JSON line a
(model, rows) into profiles/small_batch_bench.jsonl: the medians over rounds,
their spread (min, max) and the ratio own / tree-parallel; a last line a model
names the largest row count at which the tree-parallel walk still wins.

    python scripts/bench_small_batch.py [--models c2,c3,c4] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from kfserving_amd.engine import OPT_SMALL_BATCH_ROWS, DeviceForest  # noqa: E402
from kfserving_amd.forest import OUT_LEAF, OUT_MARGIN, OUT_PREDICT  # noqa: E402

SIZES = (1, 8, 64, 256, 1024, 4096)
ROUNDS, CALLS, LAUNCHES = 5, 200, 50
ON = 1 << 20   # every size of SIZES takes the walk


def models(names):
    if "c2" in names:
        yield "c2", bench.build_model()[2], bench.N_FEAT
    if "c3" in names:
        yield "c3", bench.c3_forest()[0], 100
    if "c4" in names:
        yield "c4", bench.c4_forest()[0], 64


def host_call_ms(dev, X):
    t = np.empty(CALLS)
    for i in range(CALLS):
        t0 = time.perf_counter()
        dev.predict(X, OUT_PREDICT)
        t[i] = (time.perf_counter() - t0) * 1e3
    return float(np.percentile(t, 50)), float(np.percentile(t, 99))


def launch_ms(dev, torch, xt, out, rows, cols):
    stream = torch.cuda.current_stream().cuda_stream
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def launch():
        dev.predict_device(xt.data_ptr(), 0, rows, cols, cols, OUT_PREDICT, out.data_ptr(),
                           out.numel(), stream=stream)
    launch()
    torch.cuda.synchronize()
    a.record()
    for _ in range(LAUNCHES):
        launch()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / LAUNCHES


def spread(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c2,c3,c4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_batch_bench.jsonl"))
    args = ap.parse_args()
    import torch
    with open(args.out, "w") as fh:
        for name, forest, F in models(args.models.split(",")):
            dev = DeviceForest(forest, [0])
            info = dev.info()
            out_dt = torch.float32 if forest.output_dtype(OUT_PREDICT) == np.float32 else torch.float64
            wins, still_winning = 0, True
            for rows in SIZES:
                X = np.random.default_rng(rows).standard_normal((rows, F)).astype(np.float32)
                for kind in (OUT_MARGIN, OUT_PREDICT, OUT_LEAF):   # the same bits first
                    dev.set_option(OPT_SMALL_BATCH_ROWS, ON)
                    got = dev.predict(X, kind)
                    dev.set_option(OPT_SMALL_BATCH_ROWS, 0)
                    assert np.array_equal(got, dev.predict(X, kind)), (name, rows, kind)
                xt = torch.from_numpy(X).cuda()
                out = torch.empty(rows * forest.output_width(OUT_PREDICT), dtype=out_dt, device="cuda")
                t = {k: {"p50": [], "p99": [], "launch": []} for k in ("own", "tree_lanes")}
                for _ in range(ROUNDS):
                    for k, value in (("own", 0), ("tree_lanes", ON)):
                        dev.set_option(OPT_SMALL_BATCH_ROWS, value)
                        p50, p99 = host_call_ms(dev, X)
                        t[k]["p50"].append(p50)
                        t[k]["p99"].append(p99)
                        t[k]["launch"].append(launch_ms(dev, torch, xt, out, rows, F))
                rec = {"model": name, "rows": rows, "layout": info["layout"], "trees": info["n_trees"],
                       "rounds": ROUNDS, "calls": CALLS, "launches": LAUNCHES}
                for k in t:
                    rec[k] = {m + "_ms": spread(v) for m, v in t[k].items()}
                rec["ratio_launch"] = rec["own"]["launch_ms"]["median"] / rec["tree_lanes"]["launch_ms"]["median"]
                rec["ratio_call_p50"] = rec["own"]["p50_ms"]["median"] / rec["tree_lanes"]["p50_ms"]["median"]
                still_winning = still_winning and rec["ratio_call_p50"] > 1.0
                if still_winning:
                    wins = rows
                print(json.dumps(rec), flush=True)
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
            rec = {"model": name, "tree_lanes_wins_up_to_rows": wins, "device_bytes": dev.info()["device_bytes"],
                   "device_bytes_before": info["device_bytes"]}
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            dev.close()


if __name__ == "__main__":
    main()
