"""Time TI_OUTPUT_TREE_QUANTILE on device-resident rows: the whole call, its
pass 1 alone (OUT_LEAF) and sklearn's own predict on the host, per case, in one
process with the three alternating round by round.  Appends one JSON line a
case to profiles/tree_quantile_bench.jsonl.

    python scripts/bench_tree_quantile.py [--rounds 5] [--out FILE]

Pass 2 (the sort and the scan) is reported as whole - pass 1, and as a multiple
of pass 1.  Times are host clocks around `calls` enqueued calls that end in a
device synchronise, `calls` sized so that a window lasts about 0.3 s; a case
is warmed up before its first round.  At 4,096 rows a call is a handful of
launches of a few microseconds each: those lines measure launch overhead."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = 20


def fit(kind, n_trees, depth):
    from sklearn.ensemble import AdaBoostRegressor, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    rng = np.random.default_rng(0)
    X = rng.standard_normal((4000, F)).astype(np.float32)
    y = X[:, 0] * X[:, 1] + np.sin(2 * X[:, 2]) + 0.3 * rng.standard_normal(4000)
    if kind == "adaboost":
        est = AdaBoostRegressor(DecisionTreeRegressor(max_depth=depth), n_estimators=n_trees,
                                loss="square", random_state=0)
    else:
        est = RandomForestRegressor(n_estimators=n_trees, max_depth=depth, random_state=0, n_jobs=16)
    return est.fit(X, y)


CASES = [("adaboost", 50, 3, (0.5,)), ("adaboost", 500, 3, (0.5,)), ("forest", 200, 10, (0.05, 0.5, 0.95))]
ROWS = (4096, 1 << 20)
WINDOW_S = 0.3      # a timed window: `calls` enqueued calls, then one synchronise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_quantile_bench.jsonl"))
    args = ap.parse_args()
    import torch
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_LEAF, OUT_TREE_QUANTILE, TI_F32
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    dev_t = torch.device("cuda", 0)
    for kind, n_trees, depth, levels in CASES:
        est = fit(kind, n_trees, depth)
        forest = forest_from_sklearn(est)
        T = forest.n_trees
        dev = DeviceForest(forest, devices=[0])
        dev.set_quantiles(levels)
        for rows in ROWS:
            Xh = np.random.default_rng(1).standard_normal((rows, F)).astype(np.float32)
            x = torch.from_numpy(Xh).to(dev_t)
            out_q = torch.empty((rows, len(levels)), dtype=torch.float64, device=dev_t)
            out_l = torch.empty((rows, T), dtype=torch.int32, device=dev_t)

            def run(k, out, calls):
                torch.cuda.synchronize(dev_t)
                t0 = time.perf_counter()
                for _ in range(calls):
                    dev.predict_device(x.data_ptr(), TI_F32, rows, F, F, k, out.data_ptr(), out.numel())
                torch.cuda.synchronize(dev_t)
                return (time.perf_counter() - t0) / calls

            # warm up both kinds, then size the timed windows to WINDOW_S each
            run(OUT_LEAF, out_l, 3)
            run(OUT_TREE_QUANTILE, out_q, 3)      # the first call uploads the tables
            calls = max(3, int(WINDOW_S / run(OUT_TREE_QUANTILE, out_q, 3)))
            host_rows = min(rows, 16384)      # sklearn's rate is flat in the batch beyond this
            whole, leaf, host = [], [], []
            for _ in range(args.rounds):
                whole.append(run(OUT_TREE_QUANTILE, out_q, calls))
                leaf.append(run(OUT_LEAF, out_l, calls))
                t0 = time.perf_counter()
                want = est.predict(Xh[:host_rows])
                host.append((time.perf_counter() - t0) * rows / host_rows)
            if kind == "adaboost":
                assert np.array_equal(out_q[:host_rows, 0].cpu().numpy(), want), "median differs from sklearn"
            w, p1 = float(np.median(whole)), float(np.median(leaf))
            rec = {"case": f"{kind} {T}x{depth}", "rows": rows, "levels": list(levels), "calls": calls,
                   "rounds": args.rounds, "whole_ms": w * 1e3, "pass1_ms": p1 * 1e3,
                   "pass2_ms": (w - p1) * 1e3, "pass2_over_pass1": (w - p1) / p1,
                   "whole_ms_min_max": [min(whole) * 1e3, max(whole) * 1e3],
                   "pass1_ms_min_max": [min(leaf) * 1e3, max(leaf) * 1e3],
                   "sklearn_host_ms": float(np.median(host)) * 1e3, "sklearn_rows_timed": host_rows,
                   "rows_per_s": rows / w}
            print(json.dumps(rec), flush=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        dev.close()


if __name__ == "__main__":
    main()
