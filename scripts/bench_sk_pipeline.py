"""A sklearn Pipeline on the device: what the pre-pass costs.

Fits SimpleImputer -> StandardScaler -> RandomForestRegressor (100 trees of
depth 10, 20 features), checks that the device answers as ``Pipeline.predict``
does (bit for bit), and times, at 100k rows, three pairs:

* the pipeline forest (float64 rows, steps on the device) against the same
  forest without steps fed sklearn-transformed float32 rows -- the path that
  existed before pre-steps, so the difference is the pre-pass's cost -- both
  on rows resident on the device (``ti_predict_device``, device-event windows
  of at least a quarter of a second, the median of the rounds) and from host
  buffers (``DeviceForest.predict``, the copies included);
* sklearn's own ``Pipeline[:-1].transform`` against ``Pipeline.predict`` on
  this host with 16 threads (``n_jobs=16``; the answer the device is held to
  is the one-thread predict, whose sum is in tree order);
* ``pre_steps_kernel`` alone (``ti_pretransform_device``) against the time to
  move rows * F * (8 + 4) bytes at the HBM rate (--hbm-tbs, default the 8 TB/s
  specification; about 6.3 TB/s is what a copy achieves).

One JSON line goes to stdout and to --out.  Nothing in the project rests on
these rates, and no counter pass is taken here: the record does not say which
resource bounds the kernel.

Usage: python scripts/bench_sk_pipeline.py [--rows 100000] [--rounds 5]
           [--out profiles/sk_pipeline_bench.jsonl]
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
TREES, DEPTH, FEATURES = 100, 10, 20
TRAIN_ROWS = 20000
WARMUP = 2


def data(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, FEATURES)) * np.logspace(-3, 6, FEATURES) + np.linspace(-50, 50, FEATURES)
    X[rng.random(X.shape) < 0.05] = np.nan
    return X


def fit():
    import numpy as np
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    X = data(TRAIN_ROWS, 0)
    z = np.nan_to_num((X - np.linspace(-50, 50, FEATURES)) / np.logspace(-3, 6, FEATURES))
    y = z[:, :6].sum(axis=1) + np.sin(z[:, 11]) * z[:, 7] \
        + 0.1 * np.random.default_rng(1).standard_normal(TRAIN_ROWS)
    pipe = Pipeline([("imp", SimpleImputer(strategy="median")), ("std", StandardScaler()),
                     ("rf", RandomForestRegressor(n_estimators=TREES, max_depth=DEPTH, n_jobs=HOST_THREADS,
                                                  random_state=0))])
    return pipe.fit(X, y)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=100000)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--hbm-tbs", type=float, default=8.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sk_pipeline_bench.jsonl"))
    a = p.parse_args()
    import dataclasses
    import numpy as np
    import torch
    from threadpoolctl import threadpool_limits
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_PREDICT, TI_F32, TI_F64
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device")
    pipe = fit()
    forest = forest_from_sklearn(pipe)
    plain = dataclasses.replace(forest, pre_ops=None, pre_consts=None, input_dtype=TI_F32,
                                meta=dict(forest.meta))
    n, F = a.rows, FEATURES
    X = data(n, 5)

    def wall(fn):
        fn()
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    with threadpool_limits(limits=HOST_THREADS):
        # the reference answer on one thread: with n_jobs > 1 the forest adds its
        # trees in the order its threads finish, and the last bits vary
        pipe[-1].n_jobs = 1
        want = pipe.predict(X)
        pipe[-1].n_jobs = HOST_THREADS
        Xt = pipe[:-1].transform(X).astype(np.float32)
        sk_transform_ms = wall(lambda: pipe[:-1].transform(X))
        sk_predict_ms = wall(lambda: pipe.predict(X))

    dev, ref = DeviceForest(forest, [0]), DeviceForest(plain, [0])
    info = dev.info()
    if not np.array_equal(dev.predict(X, OUT_PREDICT), want) or \
            not np.array_equal(ref.predict(Xt, OUT_PREDICT), want):
        raise SystemExit("device and Pipeline.predict disagree: nothing to time")
    if not np.array_equal(dev.pretransform(X).view(np.uint32), Xt.view(np.uint32)):
        raise SystemExit("pre-pass and Pipeline[:-1].transform disagree: nothing to time")
    host_pipe_ms = wall(lambda: dev.predict(X, OUT_PREDICT))
    host_plain_ms = wall(lambda: ref.predict(Xt, OUT_PREDICT))

    sh = torch.cuda.current_stream().cuda_stream
    Xd = torch.from_numpy(X).to("cuda:0")
    Xtd = torch.from_numpy(Xt).to("cuda:0")
    out = torch.empty(n, dtype=torch.float64, device="cuda:0")
    pre = torch.empty((n, F), dtype=torch.float32, device="cuda:0")

    def run_pipe():
        dev.predict_device(Xd.data_ptr(), TI_F64, n, F, F, OUT_PREDICT, out.data_ptr(), n, stream=sh)

    def run_plain():
        ref.predict_device(Xtd.data_ptr(), TI_F32, n, F, F, OUT_PREDICT, out.data_ptr(), n, stream=sh)

    def run_pre():
        dev.pretransform_device(Xd.data_ptr(), TI_F64, n, F, F, pre.data_ptr(), stream=sh)

    def events(run):
        for _ in range(WARMUP):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        reps = max(1, min(5000, int(250.0 / max(e0.elapsed_time(e1), 1e-3))))
        ms = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / reps)
        return reps, ms

    pipe_reps, dev_pipe_ms = events(run_pipe)
    if not np.array_equal(out.cpu().numpy(), want):
        raise SystemExit("resident rows and Pipeline.predict disagree: nothing to time")
    plain_reps, dev_plain_ms = events(run_plain)
    pre_reps, pre_ms = events(run_pre)
    dev.close()
    ref.close()

    def stats(ms, **more):
        med = statistics.median(ms)
        return {**more, "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
                "rows_per_s": n / (med * 1e-3)}
    moved = n * F * (8 + 4)
    rec = {"model": "SimpleImputer -> StandardScaler -> RandomForestRegressor", "trees": TREES,
           "max_depth": int(forest.depths().max()), "features": F, "pre_steps": forest.n_pre_steps,
           "nodes": forest.n_nodes, "rows": n, "rounds": a.rounds, "warmup_calls": WARMUP,
           "layout": info["layout"], "bit_exact": True,
           "device_resident": {"pipeline_f64_rows": stats(dev_pipe_ms, reps=pipe_reps),
                               "stepless_f32_transformed_rows": stats(dev_plain_ms, reps=plain_reps)},
           "device_from_host": {"pipeline_f64_rows": stats(host_pipe_ms),
                                "stepless_f32_transformed_rows": stats(host_plain_ms)},
           "sklearn_host": {"threads": HOST_THREADS, "transform": stats(sk_transform_ms),
                            "predict": stats(sk_predict_ms)},
           "pre_steps_kernel": {**stats(pre_ms, reps=pre_reps), "bytes_moved": moved,
                                "hbm_tb_per_s": a.hbm_tbs,
                                "ms_at_hbm_rate": moved / (a.hbm_tbs * 1e12) * 1e3}}
    rec["pre_pass_cost_ms_resident"] = (rec["device_resident"]["pipeline_f64_rows"]["ms_median"]
                                        - rec["device_resident"]["stepless_f32_transformed_rows"]["ms_median"])
    rec["pre_pass_cost_ms_from_host"] = (rec["device_from_host"]["pipeline_f64_rows"]["ms_median"]
                                         - rec["device_from_host"]["stepless_f32_transformed_rows"]["ms_median"])
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
