"""What a categorical XGBoost forest costs on the device, layout by layout.

Workload: C2's shape (500 trees x depth 8 x 28 features, 1M float32 rows
resident on one GPU) with features 0-3 categorical over 64 categories
(xgboost_format.add_categorical_splits on the C2 generator's trees).  Timed,
device-resident and event-timed as bench.py / bench_configs.py time their
loops, one kernel per call:

  cat_layout10   the categorical forest on the categorical heap (layout 10)
  cat_layout1    the same forest under TI_FORCE_LAYOUT=explicit (layout 1, the
                 only kernel that evaluated categorical nodes before layout 10)
  num_heap       the same trees without the categorical nodes under
                 TI_FORCE_LAYOUT=heap (layout 0, the float heap kernel layout 10
                 extends): what the categorical test costs the walk

Each on NaN-free rows (the tiles take the NaN-free walk) and on rows with 1 %
NaN (every tile takes the checking walk).  The configurations alternate within
each of --rounds rounds; the median, minimum and maximum over rounds are kept.
The predictions of layouts 10 and 1 are compared bit for bit on the device.

One JSON line per configuration is appended to --out and printed.

Usage: python scripts/bench_xgb_categorical.py [--rows N] [--steps K] [--warmup W]
                                               [--rounds R] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TI_DEV_KNOBS", "1")    # TI_FORCE_LAYOUT is a developer knob

N_TREES, DEPTH, N_FEAT = 500, 8, 28
CAT_FEATURES, N_CATEGORIES = (0, 1, 2, 3), 64


def make_forest(categorical: bool):
    from kfserving_amd.formats import xgboost_format as xf
    trees, ti = xf.synthetic_complete_trees(N_TREES, DEPTH, N_FEAT, seed=0)
    if categorical:
        xf.add_categorical_splits(trees, list(CAT_FEATURES), N_CATEGORIES, seed=1)
    f = xf.forest_from_raw_trees(trees, ti, N_FEAT, 0, 0.5, "binary:logistic", legacy=False)
    n_cat = sum(len(t.get("cats", {})) for t in trees)
    return f, n_cat


def device_forest(forest, layout):
    from kfserving_amd.engine import DeviceForest
    import torch
    old = os.environ.pop("TI_FORCE_LAYOUT", None)
    if layout:
        os.environ["TI_FORCE_LAYOUT"] = layout
    try:
        return DeviceForest(forest, [torch.cuda.current_device()])
    finally:
        os.environ.pop("TI_FORCE_LAYOUT", None)
        if old is not None:
            os.environ["TI_FORCE_LAYOUT"] = old


def make_rows(rows, nan_fraction, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    X = torch.randn((rows, N_FEAT), generator=g, device="cuda", dtype=torch.float32)
    for j in CAT_FEATURES:
        X[:, j] = torch.randint(0, N_CATEGORIES, (rows,), generator=g, device="cuda").float()
    if nan_fraction > 0:
        X[torch.rand(X.shape, generator=g, device="cuda") < nan_fraction] = float("nan")
    return X


def time_calls(dev, X, out, steps, warmup):
    """Event time per call, ms (one kernel per call; the launch gaps of a
    back-to-back loop are inside it, as in bench.py's device loop)."""
    import torch
    from kfserving_amd.forest import OUT_PREDICT, TI_F32
    stream = torch.cuda.current_stream()
    rows, cols = X.shape

    def call():
        dev.predict_device(X.data_ptr(), TI_F32, rows, cols, cols, OUT_PREDICT, out.data_ptr(),
                           out.numel(), stream=stream.cuda_stream)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--nan-fraction", type=float, default=0.01)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "xgb_cat_layouts.jsonl"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_xgb_categorical.py needs a GPU: nothing is timed on the CPU")

    cat_forest, n_cat = make_forest(True)
    num_forest, _ = make_forest(False)
    configs = [("cat_layout10", cat_forest, "cheap", 10), ("cat_layout1", cat_forest, "explicit", 1),
               ("num_heap", num_forest, "heap", 0)]
    devs = {}
    for name, forest, layout, want in configs:
        devs[name] = device_forest(forest, layout)
        got = devs[name].info()["layout"]
        if got != want:
            raise SystemExit(f"{name}: expected layout {want}, the library chose {got}")
    default_layout = device_forest(cat_forest, "")
    default_id = default_layout.info()["layout"]
    default_layout.close()

    variants = [("nan_free", 0.0), ("nan_%g" % a.nan_fraction, a.nan_fraction)]
    inputs = {v: make_rows(a.rows, frac, seed=11 + i) for i, (v, frac) in enumerate(variants)}
    out = torch.empty(a.rows, dtype=torch.float32, device="cuda")
    identical = {}
    for v, X in inputs.items():
        res = {}
        for name in ("cat_layout10", "cat_layout1"):
            time_calls(devs[name], X, out, 1, 0)
            res[name] = out.clone()
        identical[v] = bool(torch.equal(res["cat_layout10"], res["cat_layout1"]))
    ms = {(name, v): [] for name, *_ in configs for v, _ in variants}
    for _ in range(a.rounds):
        for v, X in inputs.items():
            for name, *_ in configs:
                ms[(name, v)].append(time_calls(devs[name], X, out, a.steps, a.warmup))

    lines = []
    for name, forest, layout, want in configs:
        info = devs[name].info()
        line = {"bench": "xgb_categorical", "config": name, "layout": info["layout"],
                "force_layout": layout, "default_layout_of_categorical_forest": default_id,
                "trees": N_TREES, "depth": DEPTH, "features": N_FEAT, "rows": a.rows,
                "categorical_features": list(CAT_FEATURES), "categories": N_CATEGORIES,
                "categorical_nodes": n_cat if forest is cat_forest else 0,
                "tree_stride_bytes": info["tree_stride_bytes"], "n_stages": info["n_stages"],
                "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                "device": torch.cuda.get_device_name(0)}
        for v, _ in variants:
            t = ms[(name, v)]
            med = statistics.median(t)
            line[v] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(min(t), 4),
                       "kernel_ms_max": round(max(t), 4),
                       "rows_per_s": round(a.rows / (med * 1e-3), 1)}
            if forest is cat_forest:
                line[v]["layout10_equals_layout1"] = identical[v]
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            s = json.dumps(line)
            fh.write(s + "\n")
            print(s, flush=True)
    for d in devs.values():
        d.close()
    if not all(identical.values()):
        raise SystemExit("layouts 10 and 1 disagree")


if __name__ == "__main__":
    main()
