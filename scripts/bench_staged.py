"""Time TI_OUTPUT_STAGED on device-resident rows of the C2 model (500 x depth 8,
28 features): the whole call, its pass 1 alone (OUT_LEAF; pass 2 is the
difference) and the only route there was before it -- S ``tree_subset`` device
forests, each predicting OUT_MARGIN, one after the other -- in one process, the
three alternating round by round.  Appends one JSON line a stage count to
profiles/staged_bench.jsonl.

    python scripts/bench_staged.py [--rounds 5] [--rows 100000] [--out FILE]

Times are host clocks around `calls` enqueued calls that end in a device
synchronise, `calls` sized per route so that a timed window lasts about 0.3 s,
after a warm-up; the S-forests route is timed with its forests already
resident (their S uploads are not counted against it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_TREES, DEPTH, F = 500, 8, 28
WINDOW_S = 0.3      # a timed window: `calls` enqueued calls, then one synchronise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--stages", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "staged_bench.jsonl"))
    args = ap.parse_args()
    import torch
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_LEAF, OUT_MARGIN, OUT_STAGED, TI_F32
    from kfserving_amd.formats.xgboost_format import forest_from_raw_trees, synthetic_complete_trees
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev_t = torch.device("cuda", 0)
    trees, ti = synthetic_complete_trees(N_TREES, DEPTH, F, seed=0)
    forest = forest_from_raw_trees(trees, ti, F, 0, 0.5, "binary:logistic")
    rows = args.rows
    Xh = np.random.default_rng(1).standard_normal((rows, F)).astype(np.float32)
    x = torch.from_numpy(Xh).to(dev_t)
    dev = DeviceForest(forest, devices=[0])
    out_l = torch.empty((rows, N_TREES), dtype=torch.int32, device=dev_t)

    def timed(fn, calls):
        torch.cuda.synchronize(dev_t)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev_t)
        return (time.perf_counter() - t0) / calls

    def call(d, kind, out):
        d.predict_device(x.data_ptr(), TI_F32, rows, F, F, kind, out.data_ptr(), out.numel())

    for S in args.stages:
        ends = [N_TREES * (s + 1) // S for s in range(S)]
        dev.set_stages(ends)
        out_s = torch.empty((rows, S), dtype=torch.float32, device=dev_t)
        subs = [DeviceForest(forest.tree_subset(0, e), devices=[0]) for e in ends]
        out_m = torch.empty((S, rows), dtype=torch.float32, device=dev_t)

        def staged():
            call(dev, OUT_STAGED, out_s)

        def leaf():
            call(dev, OUT_LEAF, out_l)

        def forests():
            for s, d in enumerate(subs):
                call(d, OUT_MARGIN, out_m[s])

        for fn in (staged, leaf, forests):
            timed(fn, 2)
        assert torch.equal(out_s.T.contiguous(), out_m), "stages differ from the subset forests"
        calls = [max(5, int(WINDOW_S / timed(fn, 3))) for fn in (staged, leaf, forests)]
        whole, p1, old = [], [], []
        for _ in range(args.rounds):
            whole.append(timed(staged, calls[0]))
            p1.append(timed(leaf, calls[1]))
            old.append(timed(forests, calls[2]))
        w, l, o = (float(np.median(v)) for v in (whole, p1, old))
        rec = {"model": f"C2 {N_TREES}x{DEPTH}, {F} features", "rows": rows, "stages": S,
               "rounds": args.rounds, "calls": calls, "whole_ms": w * 1e3, "pass1_ms": l * 1e3,
               "pass2_ms": (w - l) * 1e3, "s_forests_ms": o * 1e3, "s_forests_over_whole": o / w,
               "whole_ms_min_max": [min(whole) * 1e3, max(whole) * 1e3],
               "pass1_ms_min_max": [min(p1) * 1e3, max(p1) * 1e3],
               "s_forests_ms_min_max": [min(old) * 1e3, max(old) * 1e3]}
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(rec) + "\n")
        for d in subs:
            d.close()
    dev.close()


if __name__ == "__main__":
    main()
