#!/usr/bin/env python
"""A/B of the binned kernels' pre-walk phase in one process: A = the 5-ary
rank search and the LDS-staged X chunks (TI_BIN_BUCKETS=0 at pack time,
TI_BIN_XPF=0 at launch, and the fixed walk's pair slots numbered sequentially,
TI_FIX_SPREAD=0: the kernel as it was before the bucket tables), B = the
defaults.  Two sides in between price each part on its own: X = A's forest
launched with the register-staged X chunks (X against A: the prefetch), C =
B with the sequential pair slots (C against X: the bucket search; B against
C: the bank-spread slot order).  One build, one box, one clock state serve
all four.

Workloads, each at bench.py's own shape (3 rotating X buffers, OUT_PREDICT):
  c2        500 x depth 8, 28 features, --rows rows (the headline)
  c2_nan    the same with 1 % NaN (every tile on the NaN-checking step)
  c2_64k    the same forest at 65,536 rows, the serving batch
  c2_hist   thresholds on 253 bin bounds (u8 bins)
For each, per round and per side: the one-stream kernel_ms from events, and
the two-stream ms per batch (wall over steps, batches alternating on two
streams), as bench.py times them.  A and B alternate inside every round.
One JSON line per (round, workload, side) goes to --out; the summary printed
at the end gives each side's median with its spread (max - min over the
rounds) in brackets, and the differences of the medians.  A difference counts only when it exceeds twice that spread.

  python scripts/ab_bin_search.py --rounds 7 --out profiles/ab_bin_search.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TI_DEV_KNOBS"] = "1"

import torch  # noqa: E402

import bench  # noqa: E402
from kfserving_amd.engine import DeviceForest  # noqa: E402
from kfserving_amd.forest import OUT_PREDICT, TI_F32  # noqa: E402

A_PACK = {"TI_BIN_BUCKETS": "0", "TI_FIX_SPREAD": "0"}
A_LAUNCH = {"TI_BIN_XPF": "0"}
C_PACK = {"TI_FIX_SPREAD": "0"}


class env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def pair(forest):
    with env(A_PACK):
        a = DeviceForest(forest, devices=[0])
    with env(C_PACK):
        c = DeviceForest(forest, devices=[0])
    return {"A": a, "X": a, "C": c, "B": DeviceForest(forest, devices=[0])}


def measure(dev, Xs, rows, steps, warmup, s1):
    """(one-stream kernel ms from events, two-stream ms per batch from the wall).
    s1 is the second stream, the same for every call: a new one each time
    lands on the first stream's hardware queue every few calls, and the two
    batches then run one after the other."""
    n_feat = Xs[0].shape[1]
    s0 = torch.cuda.current_stream()
    outs = [torch.empty(rows, dtype=torch.float32, device="cuda") for _ in range(2)]
    it = [0]

    def launch(k):
        Xi = Xs[it[0] % len(Xs)]
        it[0] += 1
        dev.predict_device(Xi.data_ptr(), TI_F32, rows, n_feat, n_feat, OUT_PREDICT,
                           outs[k].data_ptr(), rows, slot=0,
                           stream=(s0 if k == 0 else s1).cuda_stream)

    for _ in range(warmup):
        launch(0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        launch(0)
    e1.record()
    torch.cuda.synchronize()
    one = e0.elapsed_time(e1) / steps
    for _ in range(warmup):
        launch(it[0] % 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s1.wait_stream(s0)
    for _ in range(steps):
        launch(it[0] % 2)
    s0.wait_stream(s1)
    torch.cuda.synchronize()
    two = (time.perf_counter() - t0) / steps * 1e3
    return one, two


def second_stream(dev, Xs, rows):
    """A stream on which a second batch really runs beside the first: the
    first of up to 4 new streams whose two-stream time per batch is below the
    one-stream time (a stream that shares the first one's hardware queue runs
    the batches one after the other).  None of the four: the run stops, since
    its two-stream figures would be one-stream ones."""
    for _ in range(4):
        s1 = torch.cuda.Stream()
        one, two = measure(dev, Xs, rows, 20, 5, s1)
        print(json.dumps({"second_stream_probe": {"kernel_ms": round(one, 5),
                                                  "two_stream_ms_per_batch": round(two, 5)}}), flush=True)
        if two < 0.97 * one:
            return s1
    sys.exit("no second stream on which two batches overlap")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rows", type=int, default=bench.ROWS)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_bin_search.jsonl"))
    args = p.parse_args()
    rows = args.rows
    _, _, c2 = bench.build_model()
    hist = bench.c2_hist_forest()[0]
    Xs = [bench.device_normal(rows, bench.N_FEAT, 7919 + i, "cuda") for i in range(3)]
    Xn = []
    for i in range(3):
        x = Xs[i].clone()
        g = torch.Generator(device="cuda")
        g.manual_seed(100 + i)
        x[torch.rand(x.shape, generator=g, device="cuda") < 0.01] = float("nan")
        Xn.append(x)
    forests = {"c2": pair(c2), "c2_hist": pair(hist)}
    work = [("c2", "c2", Xs, rows), ("c2_nan", "c2", Xn, rows),
            ("c2_64k", "c2", [x[:65536] for x in Xs], 65536), ("c2_hist", "c2_hist", Xs, rows)]
    # the two sides compute the same thing (checked before anything is timed)
    for name, fk, X, n in work:
        got = {}
        for side, dev in forests[fk].items():
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            with env(A_LAUNCH if side == "A" else {}):
                dev.predict_device(X[0].data_ptr(), TI_F32, n, bench.N_FEAT, bench.N_FEAT,
                                   OUT_PREDICT, out.data_ptr(), n)
            torch.cuda.synchronize()
            got[side] = out
        assert all(torch.equal(got["A"], got[sd]) for sd in "XCB"), name
    lines = []
    s1 = second_stream(forests["c2"]["B"], Xs, rows)
    for r in range(args.rounds):
        for name, fk, X, n in work:
            for side in ("AXCB" if r % 2 == 0 else "BCXA"):
                with env(A_LAUNCH if side == "A" else {}):
                    one, two = measure(forests[fk][side], X, n, args.steps, args.warmup, s1)
                rec = {"round": r, "workload": name, "side": side, "rows": n, "steps": args.steps,
                       "kernel_ms": round(one, 5), "two_stream_ms_per_batch": round(two, 5),
                       "device_bytes": forests[fk][side].info()["device_bytes"]}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    for name, _, _, _ in work:
        for key in ("kernel_ms", "two_stream_ms_per_batch"):
            v = {sd: [x[key] for x in lines if x["workload"] == name and x["side"] == sd]
                 for sd in "AXCB"}
            m = {sd: statistics.median(v[sd]) for sd in "AXCB"}
            print(f"{name:8s} {key:24s} " +
                  "  ".join(f"{sd} {m[sd]:.4f} ({max(v[sd]) - min(v[sd]):.4f})" for sd in "AXCB") +
                  "  " + "  ".join(f"{p}-{q} {100 * (m[p] - m[q]) / m[q]:+.2f}%"
                                   for p, q in ("BA", "XA", "CX", "BC")))


if __name__ == "__main__":
    main()
