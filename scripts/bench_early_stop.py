"""Time TI_OUTPUT_EARLY_STOP on device-resident rows of C3's shape as a binary
model (LightGBM leaf-wise, 1000 trees x 255 leaves, 100 features) against
TI_OUTPUT_MARGIN of the same forest in the same process, the two alternating
round by round, for float32 and float64 rows.  R is 10 iterations.  Three
thresholds are taken from a CPU restatement of the rule on a sample of the rows
so that a row walks about 25 %, 50 % and 100 % of the trees; the fraction the
sample walks is recorded beside each time.  Appends one JSON line a (dtype,
threshold) to profiles/early_stop_bench.jsonl.

    python scripts/bench_early_stop.py [--rounds 5] [--rows 1000000] [--out FILE]

Times are host clocks around `calls` enqueued calls that end in a device
synchronise, `calls` sized so that a timed window lasts about 0.3 s, after a
warm-up."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_TREES, LEAVES, F, FREQ = 1000, 255, 100, 10
WINDOW_S = 0.3
SAMPLE = 2000


def walked(stats, m):
    """Fraction of the trees a row walks at threshold m: stats [rows, checks]
    are 2 |acc| after each whole round of the unstopped chain, which is the
    stopped chain's up to the row's first stop."""
    hit = stats > m
    first = np.where(hit.any(axis=1), hit.argmax(axis=1) + 1, 0)
    trees = np.where(first > 0, first * FREQ, N_TREES)
    return float(trees.mean() / N_TREES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "early_stop_bench.jsonl"))
    args = ap.parse_args()
    import torch
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_EARLY_STOP, OUT_MARGIN, TI_F32, TI_F64
    from kfserving_amd.formats import lightgbm_format as lf, load_lightgbm_model
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import canon_eval
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev_t = torch.device("cuda", 0)
    trees = lf.synthetic_leafwise_trees(N_TREES, LEAVES, F, seed=0)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.txt")
        lf.write_lightgbm_text(p, trees, F, "binary sigmoid:1")
        forest = load_lightgbm_model(p)
    rows = args.rows
    Xh = np.random.default_rng(1).standard_normal((rows, F))
    # the unstopped chain of a sample, on the CPU: 2 |acc| after every round
    lv = canon_eval.leaves(forest, Xh[:SAMPLE])
    vals = forest.leaf_value[forest.tree_offset[:-1][None, :] + lv][:, :, 0]
    chain = forest.base_margin[0] + np.cumsum(vals, axis=1)
    stats = 2.0 * np.abs(chain[:, FREQ - 1::FREQ])
    grid = np.quantile(stats, np.linspace(0.0, 1.0, 401))
    margins = [float(grid[np.argmin([abs(walked(stats, m) - want) for m in grid])]) for want in (0.25, 0.5)]
    margins.append(float("inf"))
    dev = DeviceForest(forest, devices=[0])

    def timed(fn, calls):
        torch.cuda.synchronize(dev_t)
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize(dev_t)
        return (time.perf_counter() - t0) / calls

    for np_t, ti_t in ((np.float32, TI_F32), (np.float64, TI_F64)):
        x = torch.from_numpy(Xh.astype(np_t)).to(dev_t)
        out_m = torch.empty(rows, dtype=torch.float64, device=dev_t)
        out_e = torch.empty(rows, dtype=torch.float64, device=dev_t)

        def call(kind, out):
            dev.predict_device(x.data_ptr(), ti_t, rows, F, F, kind, out.data_ptr(), out.numel())

        def plain():
            call(OUT_MARGIN, out_m)

        def stopped():
            call(OUT_EARLY_STOP, out_e)

        for m in margins:
            dev.set_early_stop(FREQ, m)
            for fn in (plain, stopped):
                timed(fn, 2)
            if m == float("inf"):
                assert torch.equal(out_m, out_e), "no row stops, yet the margins differ"
            calls = [max(3, int(WINDOW_S / timed(fn, 2))) for fn in (plain, stopped)]
            tp, ts = [], []
            for _ in range(args.rounds):
                tp.append(timed(plain, calls[0]))
                ts.append(timed(stopped, calls[1]))
            a, b = float(np.median(tp)), float(np.median(ts))
            rec = {"model": f"C3 shape, binary: {N_TREES} x {LEAVES} leaves, {F} features", "rows": rows,
                   "x_dtype": np_t.__name__, "round_trees": FREQ, "margin": m if m != float("inf") else "inf",
                   "trees_walked_fraction": walked(stats, m), "rounds": args.rounds, "calls": calls,
                   "margin_ms": a * 1e3, "early_stop_ms": b * 1e3, "margin_over_early_stop": a / b,
                   "margin_ms_min_max": [min(tp) * 1e3, max(tp) * 1e3],
                   "early_stop_ms_min_max": [min(ts) * 1e3, max(ts) * 1e3],
                   "layout": dev.info()["layout"]}
            print(json.dumps(rec), flush=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
