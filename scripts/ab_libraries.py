#!/usr/bin/env python
"""A/B of builds of libtreeinfer.so on the fixed walk's workloads, in one
process: every side is a library (and, optionally, launch environment) of its
own, and the sides alternate inside every round, so one box and one clock
state serve them all.

A side is LABEL=LIBRARY[,KEY=VALUE...]: LIBRARY is `tree` (the in-tree
library), the name of a variant under kfserving_amd/lib/variants/
(scripts/build_variant.py) or a path to a libtreeinfer.so; the KEY=VALUE pairs
are set in the environment around that side's launches.  The first side is the
one the others are compared against.

  python scripts/build_variant.py parent --source ../parent
  python scripts/ab_libraries.py --side A=parent --side B=tree \\
      --side N=tree,TI_BHEAP_NG=2 --rounds 7 --out run_out/ab.jsonl

A parent side is built from the parent commit's own sources, since the kernel
header keeps one path and no switch back to an earlier one:
`git worktree add ../parent <commit>`, then build_variant.py with --source as
above.  (N is the in-tree library at 8 trees a stage: 47,104 B of LDS, three
workgroups a CU.)

Workloads and figures are those of scripts/ab_bin_search.py: c2, c2_nan,
c2_64k and c2_hist at bench.py's shape (3 rotating X buffers), the one-stream
kernel ms from events and the two-stream ms per batch, the second stream taken
only after ab_bin_search.second_stream's overlap check.  All sides must give
the same bits before anything is timed.  One JSON line per (round, workload,
side) goes to --out; the summary gives each side's median with its spread
(max - min over the rounds) and the differences of the medians against the
first side.  A difference counts only when it exceeds twice the first side's
spread (marked ~ when it does not).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def parse_side(text):
    """LABEL=LIBRARY[,KEY=VALUE...] -> (label, library path or None for the
    in-tree one, launch environment)."""
    label, _, rest = text.partition("=")
    lib, *pairs = rest.split(",")
    if not label or not lib or any("=" not in kv for kv in pairs):
        raise argparse.ArgumentTypeError(f"{text!r} is not LABEL=LIBRARY[,KEY=VALUE...]")
    if lib == "tree":
        path = None
    elif os.sep in lib or lib.endswith(".so"):
        path = os.path.abspath(lib)
    else:
        path = os.path.join(ROOT, "kfserving_amd", "lib", "variants", lib, "libtreeinfer.so")
    return label, path, dict(kv.split("=", 1) for kv in pairs)


def with_library(lib, forest):
    """A DeviceForest bound to `lib` (a DeviceForest keeps the library that
    was current when it was made)."""
    from kfserving_amd import engine
    default = engine.load_library()
    engine._lib = lib
    try:
        return engine.DeviceForest(forest, devices=[0])
    finally:
        engine._lib = default


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--side", type=parse_side, action="append", required=True, dest="sides",
                   metavar="LABEL=LIBRARY[,KEY=VALUE...]", help="two at least; the first is the baseline")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rows", type=int, default=None, help="default: bench.py's")
    p.add_argument("--out", required=True, help="the JSON lines' file")
    args = p.parse_args()
    sides = [s[0] for s in args.sides]
    if len(sides) < 2 or len(set(sides)) != len(sides):
        p.error("needs two sides or more, each with a label of its own")

    import torch

    import bench
    from ab_bin_search import env, measure, second_stream
    from kfserving_amd import engine
    from kfserving_amd.forest import OUT_PREDICT, TI_F32

    rows = args.rows or bench.ROWS
    libs = {label: engine.load_library(path) for label, path, _ in args.sides}
    launch = {label: kv for label, _, kv in args.sides}
    base = sides[0]
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
    n64 = min(65536, rows)
    work = [("c2", "c2", Xs, rows), ("c2_nan", "c2", Xn, rows),
            ("c2_64k", "c2", [x[:n64] for x in Xs], n64), ("c2_hist", "c2_hist", Xs, rows)]
    # every side computes the same thing (checked before anything is timed)
    for name, fk, X, n in work:
        got = {}
        for side, dev in forests[fk].items():
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            with env(launch[side]):
                dev.predict_device(X[0].data_ptr(), TI_F32, n, bench.N_FEAT, bench.N_FEAT, OUT_PREDICT,
                                   out.data_ptr(), n)
            torch.cuda.synchronize()
            got[side] = out
        assert all(torch.equal(got[base], got[sd]) for sd in sides), name
    lines = []
    s1 = second_stream(forests["c2"][base], Xs, rows)
    for r in range(args.rounds):
        for name, fk, X, n in work:
            for side in (sides if r % 2 == 0 else sides[::-1]):
                with env(launch[side]):
                    one, two = measure(forests[fk][side], X, n, args.steps, args.warmup, s1)
                rec = {"round": r, "workload": name, "side": side, "rows": n, "steps": args.steps,
                       "kernel_ms": round(one, 5), "two_stream_ms_per_batch": round(two, 5)}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    for name, _, _, _ in work:
        for key in ("kernel_ms", "two_stream_ms_per_batch"):
            v = {sd: [x[key] for x in lines if x["workload"] == name and x["side"] == sd] for sd in sides}
            m = {sd: statistics.median(v[sd]) for sd in sides}
            spread = max(v[base]) - min(v[base])
            print(f"{name:8s} {key:24s} " +
                  "  ".join(f"{sd} {m[sd]:.4f} ({max(v[sd]) - min(v[sd]):.4f})" for sd in sides) + "  " +
                  "  ".join(f"{sd}-{base} {100 * (m[sd] - m[base]) / m[base]:+.2f}%"
                            f"{'' if abs(m[sd] - m[base]) > 2 * spread else '~'}"
                            for sd in sides[1:]))


if __name__ == "__main__":
    main()
