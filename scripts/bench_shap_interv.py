"""Interventional TreeSHAP (TI_OUTPUT_CONTRIB_INTERV) of the C2 model (500
trees of depth 8 on 28 features, 128,000 paths) against B = 100 and 1,000
background rows, at 1, 256 and 4,096 request rows, with plain TI_OUTPUT_CONTRIB
in the same process for scale.  One JSON line a measurement into
profiles/shap_interv_bench.jsonl.

What is timed: whole ti_predict calls from host rows to host output (the call
returns after its device synchronise), by a host clock, after two warm-up
calls of the same shape, repeated until at least --min-s seconds have passed;
the median call gives rows_per_s, the fastest and slowest are kept beside it.
set_background is the host wall time of ti_forest_set_background (path tables
already built: the second call of a shape), which ends in a device
synchronise too.  No GPU: the script fails.

Usage: python scripts/bench_shap_interv.py [--out profiles/shap_interv_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, min_s, max_calls=200):
    call()
    call()
    ts = []
    while sum(ts) < min_s and len(ts) < max_calls:
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_interv_bench.jsonl"))
    p.add_argument("--min-s", type=float, default=1.0)
    a = p.parse_args()
    import numpy as np
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.formats import xgboost_format as xf
    from kfserving_amd.forest import OUT_CONTRIB, OUT_CONTRIB_INTERV
    trees, ti = xf.synthetic_complete_trees(500, 8, 28, seed=0)
    f = xf.forest_from_raw_trees(trees, ti, 28, 0, 0.5, "binary:logistic")
    dev = DeviceForest(f, [0])
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4096, 28)).astype(np.float32)
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def measure(kind, name, rows, extra):
        ts = timed(lambda: dev.predict(X[:rows], kind), a.min_s)
        med = statistics.median(ts)
        emit(dict({"kind": name, "rows": rows, "calls": len(ts), "call_ms": med * 1e3,
                   "call_ms_min": min(ts) * 1e3, "call_ms_max": max(ts) * 1e3,
                   "rows_per_s": rows / med}, **extra))

    for rows in (1, 256, 4096):
        measure(OUT_CONTRIB, "TI_OUTPUT_CONTRIB", rows, {})
    for B in (100, 1000):
        Z = rng.standard_normal((B, 28)).astype(np.float32)
        dev.set_background(Z)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            dev.set_background(Z)
            ts.append(time.perf_counter() - t0)
        emit({"kind": "ti_forest_set_background", "B": B, "ms": statistics.median(ts) * 1e3,
              "mask_table_mib": 128000 * B * 4 / 2 ** 20})
        for rows in (1, 256, 4096):
            measure(OUT_CONTRIB_INTERV, "TI_OUTPUT_CONTRIB_INTERV", rows, {"B": B})
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
