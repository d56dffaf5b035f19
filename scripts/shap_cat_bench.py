"""What a categorical path element costs TreeSHAP contributions
(TI_OUTPUT_CONTRIB): one LightGBM-shaped forest (200 trees of
255 leaves, 100 features) with and without lightgbm_format's
add_categorical_splits on 10 of the features at 300 categories, rows/s of
ti_predict_device at a few batch sizes, one JSON line each; then the ratio
per batch size and the device bytes of the TreeSHAP tables of both forests
(ti_forest_info device_bytes after the first contributions call minus before:
for the categorical forest that includes the {first, nwords} array and the
category sets).

Usage: python scripts/shap_cat_bench.py [--rows 4096,100000] [--reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TREES, LEAVES, FEATURES, CAT_FEATURES, CATEGORIES = 200, 255, 100, 10, 300


def forest(categorical: bool):
    import tempfile
    from kfserving_amd.formats import lightgbm_format as lf
    trees = lf.synthetic_leafwise_trees(TREES, LEAVES, FEATURES, seed=17)
    if categorical:
        lf.add_categorical_splits(trees, list(range(0, FEATURES, FEATURES // CAT_FEATURES)),
                                  CATEGORIES, seed=18)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.txt")
        lf.write_lightgbm_text(p, trees, FEATURES, "binary sigmoid:1")
        return lf.load_lightgbm_model(p)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="4096,100000")
    p.add_argument("--reps", type=int, default=3)
    a = p.parse_args()
    import numpy as np
    import torch
    from kfserving_amd.engine import OPT_SHAP_TABLE_ROWS, DeviceForest
    from kfserving_amd.forest import OUT_CONTRIB, OUT_MARGIN, TI_F64
    sh = torch.cuda.current_stream().cuda_stream
    sizes = [int(x) for x in a.rows.split(",")]
    rng = np.random.default_rng(5)
    X = rng.standard_normal((max(sizes), FEATURES))
    cat_cols = list(range(0, FEATURES, FEATURES // CAT_FEATURES))
    X[:, cat_cols] = rng.integers(0, CATEGORIES, size=(X.shape[0], len(cat_cols)))
    Xd = torch.from_numpy(X).to("cuda:0")
    rate = {}
    for kind in ("numerical", "categorical"):
        f = forest(kind == "categorical")
        dev = DeviceForest(f, [0])
        dev.set_option(OPT_SHAP_TABLE_ROWS, 0)       # paths are longer than the table's 8
        dev.predict(X[:64], OUT_MARGIN)
        before = dev.info()["device_bytes"]
        W = f.output_width(OUT_CONTRIB)
        for n in sizes:
            out = torch.empty(n * W, dtype=torch.float64, device="cuda")

            def run():
                dev.predict_device(Xd.data_ptr(), TI_F64, n, FEATURES, FEATURES, OUT_CONTRIB,
                                   out.data_ptr(), out.numel(), stream=sh)
            run()                                     # the first call builds the path tables
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / a.reps
            rate[kind, n] = n / (ms * 1e-3)
            print(json.dumps({"forest": kind, "rows": n, "ms": ms, "rows_per_s": rate[kind, n]}),
                  flush=True)
        cat_nodes = int(((f.flags & 4) != 0).sum())
        print(json.dumps({"forest": kind, "categorical_nodes": cat_nodes,
                          "predict_bytes": before,
                          "shap_table_bytes": dev.info()["device_bytes"] - before}), flush=True)
        dev.close()
    for n in sizes:
        print(json.dumps({"rows": n, "categorical_over_numerical":
                          rate["categorical", n] / rate["numerical", n]}), flush=True)


if __name__ == "__main__":
    main()
