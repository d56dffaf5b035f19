"""The categorical records (layout 11) beside the float explicit kernel
(layout 1) on deep forests with categorical splits.

Two forests, each created twice in this process -- under
TI_FORCE_LAYOUT=crecord and TI_FORCE_LAYOUT=explicit -- and timed on the same
resident rows (float32 and float64), PREDICT output:

* ``lgb``: scripts/shap_cat_bench.py's generator, 200 LightGBM trees of 255
  leaves over 100 features, 10 of them categorical at 300 categories, with
  the numerical splits the generator leaves on those 10 moved one feature up
  (a trained model never splits a categorical feature numerically, and layout
  11 refuses a forest that does);
* ``hgb``: the HistGradientBoostingRegressor of scripts/bench_hgb.py
  (XGBoost's rule).

Device-event windows of at least a quarter of a second each, the two layouts
alternating round by round; a line per (forest, input type) with each layout's
median, minimum and maximum and the spread (max - min) / median of its rounds
goes to stdout and to --out.  The margins of the two layouts are compared bit
for bit before anything is timed.

--layouts explicit times layout 1 alone, which a library without layout 11
(TREEINFER_LIB) can run too: layout 1 on the parent build against this one.

Usage: python scripts/bench_cat_records.py [--rows 1000000] [--rounds 7]
           [--forests lgb,hgb] [--layouts crecord,explicit]
           [--out profiles/cat_records_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
os.environ["TI_DEV_KNOBS"] = "1"
WARMUP = 2


def lgb_forest():
    import tempfile
    import numpy as np
    import shap_cat_bench as sc
    from kfserving_amd.formats import lightgbm_format as lf
    cats = list(range(0, sc.FEATURES, sc.FEATURES // sc.CAT_FEATURES))
    trees = lf.synthetic_leafwise_trees(sc.TREES, sc.LEAVES, sc.FEATURES, seed=17)
    lf.add_categorical_splits(trees, cats, sc.CATEGORIES, seed=18)
    for t in trees:
        f = np.asarray(t["split_feature"]).copy()
        f[((np.asarray(t["decision_type"]) & 1) == 0) & np.isin(f, cats)] += 1
        t["split_feature"] = f
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.txt")
        lf.write_lightgbm_text(p, trees, sc.FEATURES, "binary sigmoid:1")
        forest = lf.load_lightgbm_model(p)

    def rows(n):
        rng = np.random.default_rng(3)
        X = rng.standard_normal((n, sc.FEATURES))
        for c in cats:
            X[:, c] = rng.integers(0, sc.CATEGORIES + 20, size=n)
        X[rng.random(X.shape) < 0.001] = np.nan    # about one tile in four holds a NaN
        return X
    return forest, rows


def hgb_forest():
    import bench_hgb as bh
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    return forest_from_sklearn(bh.fit()), lambda n: bh.data(n, 5)


def create(forest, layout, xdt):
    import dataclasses
    from kfserving_amd.engine import DeviceForest
    os.environ["TI_FORCE_LAYOUT"] = layout
    try:
        return DeviceForest(dataclasses.replace(forest, input_dtype=xdt), [0])
    finally:
        del os.environ["TI_FORCE_LAYOUT"]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1000000)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--forests", default="lgb,hgb")
    p.add_argument("--layouts", default="crecord,explicit")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "cat_records_bench.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch
    from kfserving_amd.forest import OUT_MARGIN, OUT_PREDICT, TI_F32, TI_F64
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device")
    sh = torch.cuda.current_stream().cuda_stream
    n = a.rows
    lines = []
    for name in a.forests.split(","):
        forest, rows = {"lgb": lgb_forest, "hgb": hgb_forest}[name]()
        X = rows(n)
        F = X.shape[1]
        for xdt, npdt, tdt in ((TI_F32, np.float32, torch.float32), (TI_F64, np.float64, torch.float64)):
            devs = {k: create(forest, k, xdt) for k in a.layouts.split(",")}
            info = {k: d.info() for k, d in devs.items()}
            if any(v["layout"] != {"crecord": 11, "explicit": 1}[k] for k, v in info.items()):
                raise SystemExit("%s: layouts %s" % (name, {k: v["layout"] for k, v in info.items()}))
            Xd = torch.from_numpy(X.astype(npdt)).to("cuda:0")
            acc = torch.float64 if forest.accum_dtype == TI_F64 else torch.float32
            out = {k: torch.empty(n * forest.n_groups, dtype=acc, device="cuda:0") for k in devs}

            def run(k, kind=OUT_PREDICT):
                devs[k].predict_device(Xd.data_ptr(), xdt, n, F, F, kind, out[k].data_ptr(),
                                       out[k].numel(), stream=sh)
            for k in devs:
                run(k, OUT_MARGIN)
            torch.cuda.synchronize()
            if len(devs) == 2 and not torch.equal(out["crecord"], out["explicit"]):
                raise SystemExit("%s: the layouts' margins differ: nothing to time" % name)

            def window(k, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run(k)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / reps
            reps = {}
            for k in devs:
                for _ in range(WARMUP):
                    run(k)
                reps[k] = max(1, min(2000, int(250.0 / max(window(k, 1), 1e-3))))
            ms = {k: [] for k in devs}
            for _ in range(a.rounds):
                for k in devs:        # alternating: both layouts see the same drift
                    ms[k].append(window(k, reps[k]))
            rec = {"forest": name, "rows": n, "x": "float32" if xdt == TI_F32 else "float64",
                   "trees": forest.n_trees, "max_depth": int(forest.depths().max()),
                   "rounds": a.rounds, "bit_identical_margins": len(devs) == 2}
            if "crecord" in devs:
                rec.update(stages=info["crecord"]["n_stages"], tree_ilp=info["crecord"]["tree_ilp"])
            for k in devs:
                med = statistics.median(ms[k])
                rec[k] = {"reps": reps[k], "ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]),
                          "spread": (max(ms[k]) - min(ms[k])) / med, "rows_per_s": n / (med * 1e-3)}
                devs[k].close()
            if len(devs) == 2:
                rec["explicit_over_crecord"] = rec["explicit"]["ms_median"] / rec["crecord"]["ms_median"]
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
