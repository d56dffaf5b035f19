"""sklearn HistGradientBoosting on the device beside sklearn on the host.

Fits a default-shaped HistGradientBoostingRegressor (100 iterations, 31
leaves, 20 features of which 2 are categorical), checks that the device
answers as ``est.predict`` does (bit for bit: the link is the identity), and
times, at 100k rows:

* ``ti_predict_device`` on rows resident on the device (float64, as the
  forest reads them), in device-event windows of at least a quarter of a
  second, the median of the rounds;
* ``DeviceForest.predict`` from host memory (the copies included);
* ``est.predict`` on this host with 16 OpenMP threads, the median of the
  rounds.

One JSON line with the timings and the layout the library chose goes to
stdout and to --out.  Nothing in the project rests on these rates.

Usage: python scripts/bench_hgb.py [--rows 100000] [--rounds 5]
           [--out profiles/hgb_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "16")
HOST_THREADS = 16
ITERATIONS, LEAVES, FEATURES, CAT_COLS, N_CATEGORIES = 100, 31, 20, (3, 11), 40
TRAIN_ROWS = 20000
WARMUP = 2


def data(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, FEATURES))
    for c in CAT_COLS:
        X[:, c] = rng.integers(0, N_CATEGORIES, size=n)
    X[rng.random(X.shape) < 0.05] = np.nan
    return X


def fit():
    import numpy as np
    from sklearn.ensemble import HistGradientBoostingRegressor
    X = data(TRAIN_ROWS, 0)
    z = np.nan_to_num(X)
    y = z[:, :6].sum(axis=1) + (z[:, 3] % 3 == 0) * 2.0 + np.sin(z[:, 11]) * z[:, 7] \
        + 0.1 * np.random.default_rng(1).standard_normal(TRAIN_ROWS)
    return HistGradientBoostingRegressor(max_iter=ITERATIONS, max_leaf_nodes=LEAVES,
                                         categorical_features=list(CAT_COLS),
                                         random_state=0).fit(X, y)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=100000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hgb_bench.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch
    from threadpoolctl import threadpool_limits
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_PREDICT, TI_F64
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device")
    est = fit()
    forest = forest_from_sklearn(est)
    n, F = a.rows, FEATURES
    X = data(n, 5)
    dev = DeviceForest(forest, [0])
    info = dev.info()

    with threadpool_limits(limits=HOST_THREADS):
        want = est.predict(X)
        host_ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            est.predict(X)
            host_ms.append((time.perf_counter() - t0) * 1e3)
    got = dev.predict(X, OUT_PREDICT)
    if not np.array_equal(got, want):
        raise SystemExit("device and est.predict disagree: nothing to time")

    copy_ms = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        dev.predict(X, OUT_PREDICT)
        copy_ms.append((time.perf_counter() - t0) * 1e3)

    sh = torch.cuda.current_stream().cuda_stream
    Xd = torch.from_numpy(X).to("cuda:0")
    out = torch.empty(n, dtype=torch.float64, device="cuda:0")

    def run():
        dev.predict_device(Xd.data_ptr(), TI_F64, n, F, F, OUT_PREDICT, out.data_ptr(), n, stream=sh)
    for _ in range(WARMUP):
        run()
    torch.cuda.synchronize()
    if not np.array_equal(out.cpu().numpy(), want):
        raise SystemExit("resident rows and est.predict disagree: nothing to time")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    reps = max(1, min(2000, int(250.0 / max(e0.elapsed_time(e1), 1e-3))))
    dev_ms = []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1) / reps)
    dev.close()

    def stats(ms):
        med = statistics.median(ms)
        return {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "rows_per_s": n / (med * 1e-3)}
    rec = {"model": "HistGradientBoostingRegressor", "iterations": ITERATIONS,
           "max_leaf_nodes": LEAVES, "features": F, "categorical_features": len(CAT_COLS),
           "trees": forest.n_trees, "nodes": forest.n_nodes, "max_depth": int(forest.depths().max()),
           "rows": n, "rounds": a.rounds, "warmup_calls": WARMUP, "layout": info["layout"],
           "device_resident": {"reps": reps, **stats(dev_ms)},
           "device_from_host": stats(copy_ms),
           "sklearn_host": {"threads": HOST_THREADS, **stats(host_ms)},
           "bit_exact": True}
    rec["resident_over_sklearn"] = rec["device_resident"]["rows_per_s"] / rec["sklearn_host"]["rows_per_s"]
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
