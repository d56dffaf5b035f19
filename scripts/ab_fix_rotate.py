#!/usr/bin/env python
"""A/B of the fixed walk's rotated 4-tree group (treeinfer_kernels.h,
TI_FIX_ROT) and of what was tried on top of it, in one process: every side is
a library of its own, built with scripts/build_variant.py, and the sides
alternate inside every round, so one box and one clock state serve them all.

  A  fr_parent  -DTI_FIX_ROT=0                   the kernel as it was
  R  fr_rot     -DTI_FIX_ROT=1                   the rotation alone
  D  fr_dma     rotation + a one-barrier, two-buffer stage filled by LDS-DMA:
                built, measured and not merged (in
                profiles/fix_rotate_ab_dma.jsonl it is side B, the library of
                that tree)
  P  fr_prio    rotation + s_setprio 1 for waves 4-7: measured and dropped, code
                and macro (in profiles/fix_rotate_ab.jsonl)
  N  the in-tree library launched with TI_BHEAP_NG=2 (8 trees a stage, 47,104 B
     of LDS, three workgroups a CU: what a two-buffer stage's footprint costs)
  B  the in-tree library (the defaults)

A side whose library is absent is left out.  Workloads and figures are those of
scripts/ab_bin_search.py: c2, c2_nan, c2_64k and c2_hist at bench.py's shape
(3 rotating X buffers), the one-stream kernel ms from events and the
two-stream ms per batch.  One JSON line per (round, workload, side) goes to
--out; the summary gives each side's median with its spread (max - min over
the rounds) and the differences of the medians against A.  A difference
counts only when it exceeds twice A's spread (marked ~ when it does not).

  python scripts/ab_fix_rotate.py --rounds 7 --out profiles/fix_rotate_ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

import bench  # noqa: E402
from ab_bin_search import env, measure, second_stream  # noqa: E402
from ab_fix_floor import with_library  # noqa: E402
from kfserving_amd import engine  # noqa: E402
from kfserving_amd.forest import OUT_PREDICT, TI_F32  # noqa: E402

VARIANTS = {"A": "fr_parent", "R": "fr_rot", "D": "fr_dma", "P": "fr_prio"}
LAUNCH_ENV = {"N": {"TI_BHEAP_NG": "2"}}   # sides that are a launch knob on the in-tree library


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rows", type=int, default=bench.ROWS)
    p.add_argument("--sides", default="ARDPNB")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fix_rotate_ab.jsonl"))
    args = p.parse_args()
    rows = args.rows
    libs = {"B": engine.load_library()}
    libs["N"] = libs["B"]
    for side, name in VARIANTS.items():
        path = os.path.join(ROOT, "kfserving_amd", "lib", "variants", name, "libtreeinfer.so")
        if os.path.exists(path):
            libs[side] = engine.load_library(path)
    sides = "".join(s for s in args.sides if s in libs)
    if "A" not in sides or "B" not in sides:
        sys.exit("needs the parent-behaviour variant (fr_parent) and the in-tree library")
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
    forests = {k: {s: with_library(libs[s], f) for s in sides} for k, f in (("c2", c2), ("c2_hist", hist))}
    work = [("c2", "c2", Xs, rows), ("c2_nan", "c2", Xn, rows),
            ("c2_64k", "c2", [x[:65536] for x in Xs], 65536), ("c2_hist", "c2_hist", Xs, rows)]
    # every side computes the same thing (checked before anything is timed)
    for name, fk, X, n in work:
        got = {}
        for side, dev in forests[fk].items():
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            with env(LAUNCH_ENV.get(side, {})):
                dev.predict_device(X[0].data_ptr(), TI_F32, n, bench.N_FEAT, bench.N_FEAT, OUT_PREDICT,
                                   out.data_ptr(), n)
            torch.cuda.synchronize()
            got[side] = out
        assert all(torch.equal(got["A"], got[sd]) for sd in sides), name
    lines = []
    s1 = second_stream(forests["c2"]["B"], Xs, rows)
    for r in range(args.rounds):
        for name, fk, X, n in work:
            for side in (sides if r % 2 == 0 else sides[::-1]):
                with env(LAUNCH_ENV.get(side, {})):
                    one, two = measure(forests[fk][side], X, n, args.steps, args.warmup, s1)
                rec = {"round": r, "workload": name, "side": side, "rows": n, "steps": args.steps,
                       "kernel_ms": round(one, 5), "two_stream_ms_per_batch": round(two, 5)}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    for name, _, _, _ in work:
        for key in ("kernel_ms", "two_stream_ms_per_batch"):
            v = {sd: [x[key] for x in lines if x["workload"] == name and x["side"] == sd] for sd in sides}
            m = {sd: statistics.median(v[sd]) for sd in sides}
            spread_a = max(v["A"]) - min(v["A"])
            print(f"{name:8s} {key:24s} " +
                  "  ".join(f"{sd} {m[sd]:.4f} ({max(v[sd]) - min(v[sd]):.4f})" for sd in sides) + "  " +
                  "  ".join(f"{sd}-A {100 * (m[sd] - m['A']) / m['A']:+.2f}%"
                            f"{'' if abs(m[sd] - m['A']) > 2 * spread_a else '~'}"
                            for sd in sides if sd != "A"))


if __name__ == "__main__":
    main()
