"""What linear leaves cost a LightGBM forest on the device.

Workload: C3's shape (1000 leaf-wise trees x 255 leaves x 100 features, rows
resident on one GPU) with lightgbm_format.add_linear_leaves on the C3
generator's trees (0..4 terms a leaf, every 5th tree constant).  Timed
device-resident and event-timed, as bench.py times its device loop, for
float32 and float64 X:

  linear        the linear forest, TI_OUTPUT_PREDICT: the forest's walk for the
                leaf ids, then linear_leaf_kernel, a row block at a time
  const         the same trees with the linear keys stripped: one walk kernel,
                what the forest cost before linear leaves existed (the yardstick)
  leaf_only     TI_OUTPUT_LEAF of the linear forest: pass 1 alone over the
                whole batch, so pass 2's share is linear - leaf_only
  linear_256mb / linear_1024mb / linear_4096mb
                linear under TI_OPT_LINEAR_SCRATCH_MB = 256, 1024 (the default),
                4096: the cap on one row block's leaf-id scratch
  linear_feat_hbm
                linear under TI_LINEAR_FEAT_LDS=0: pass 2 reads the features from
                the row in HBM / L2 instead of an LDS image (tiles of 256 rows)

The configurations alternate within each of --rounds rounds; the median,
minimum and maximum over rounds are kept.  Before anything is timed the
device's raw scores of a 4,096-row sample are compared bit for bit (NaN equal
to NaN) with the CPU evaluator tests/linear_eval.py; no rate is printed if
they differ.

One JSON line per configuration and input type is appended to --out and printed.

Usage: python scripts/bench_lgb_linear.py [--rows N] [--steps K] [--warmup W]
                                          [--rounds R] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TI_DEV_KNOBS", "1")    # TI_LINEAR_FEAT_LDS is a developer knob

N_TREES, N_LEAVES, N_FEAT = 1000, 255, 100
MAX_TERMS, CONST_EVERY = 4, 5
SCRATCH_MB = (256, 1024, 4096)
SAMPLE = 4096


def make_models():
    """(linear forest, constant forest, the linear model's text)."""
    from kfserving_amd.formats import lightgbm_format as lf
    trees = lf.synthetic_leafwise_trees(N_TREES, N_LEAVES, N_FEAT, seed=0)
    lf.add_linear_leaves(trees, N_FEAT, seed=1, max_terms=MAX_TERMS, const_tree_every=CONST_EVERY)
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, tr in (("linear", trees), ("const", lf.strip_linear_leaves(trees))):
            path = os.path.join(tmp, name + ".txt")
            lf.write_lightgbm_text(path, tr, N_FEAT, "binary sigmoid:1")
            with open(path) as fh:
                out.append(fh.read())
    return lf.parse_lightgbm_text(out[0]), lf.parse_lightgbm_text(out[1]), out[0]


def time_calls(dev, X, xdt, kind, out, steps, warmup):
    """Event time per call, ms (the launch gaps of a back-to-back loop are
    inside it, as in bench.py's device loop)."""
    import torch
    stream = torch.cuda.current_stream()
    rows, cols = X.shape

    def call():
        dev.predict_device(X.data_ptr(), xdt, rows, cols, cols, kind, out.data_ptr(),
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


def check_sample(dev, text, dtype):
    """Device raw scores of a seeded sample against the CPU evaluator."""
    from kfserving_amd.forest import OUT_MARGIN
    from tests import linear_eval
    rng = np.random.default_rng(3)
    X = rng.standard_normal((SAMPLE, N_FEAT))
    X[rng.random(X.shape) < 0.01] = np.nan
    X = X.astype(dtype)
    want, fell = linear_eval.raw_scores(text, X)
    got = dev.predict(X, OUT_MARGIN)
    return bool(linear_eval.same_bits(got, want[:, 0])), float(fell.mean())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1 << 20)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lgb_linear_bench.jsonl"))
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lgb_linear.py needs a GPU: nothing is timed on the CPU")
    from kfserving_amd.engine import OPT_LINEAR_SCRATCH_MB, DeviceForest
    from kfserving_amd.forest import OUT_LEAF, OUT_PREDICT, TI_F32, TI_F64

    lin_forest, const_forest, text = make_models()
    device = torch.cuda.current_device()
    lin = DeviceForest(lin_forest, [device])
    const = DeviceForest(const_forest, [device])
    n_terms = int(lin_forest.lin_feature.shape[0])

    lines = []
    for dtype, tdt, xdt in ((np.float32, torch.float32, TI_F32), (np.float64, torch.float64, TI_F64)):
        same, fell = check_sample(lin, text, dtype)
        if not same:
            raise SystemExit(f"{np.dtype(dtype).name}: the device's raw scores differ from the CPU "
                             "evaluator on the sample; nothing timed")
        g = torch.Generator(device="cuda")
        g.manual_seed(11)
        X = torch.randn((a.rows, N_FEAT), generator=g, device="cuda", dtype=tdt)
        score = torch.empty(a.rows, dtype=torch.float64, device="cuda")
        leaves = torch.empty((a.rows, N_TREES), dtype=torch.int32, device="cuda")
        # (name, forest handle, output kind, output buffer, scratch cap or None)
        configs = [("linear", lin, OUT_PREDICT, score, 1024), ("const", const, OUT_PREDICT, score, None),
                   ("leaf_only", lin, OUT_LEAF, leaves, None)]
        configs += [(f"linear_{mb}mb", lin, OUT_PREDICT, score, mb) for mb in SCRATCH_MB]
        configs += [("linear_feat_hbm", lin, OUT_PREDICT, score, 1024)]
        ms = {c[0]: [] for c in configs}
        for _ in range(a.rounds):
            for name, dev, kind, out, mb in configs:
                if mb is not None:
                    dev.set_option(OPT_LINEAR_SCRATCH_MB, mb)
                if name == "linear_feat_hbm":
                    os.environ["TI_LINEAR_FEAT_LDS"] = "0"
                try:
                    ms[name].append(time_calls(dev, X, xdt, kind, out, a.steps, a.warmup))
                finally:
                    os.environ.pop("TI_LINEAR_FEAT_LDS", None)
        lin.set_option(OPT_LINEAR_SCRATCH_MB, 1024)
        med = {k: statistics.median(v) for k, v in ms.items()}
        for name, dev, kind, out, mb in configs:
            info = dev.info()
            t = ms[name]
            line = {"bench": "lgb_linear", "config": name, "x_dtype": np.dtype(dtype).name,
                    "layout": info["layout"], "bottom": info["bottom"], "linear": info["linear"],
                    "trees": N_TREES, "leaves": N_LEAVES, "features": N_FEAT, "rows": a.rows,
                    "max_terms": MAX_TERMS, "const_tree_every": CONST_EVERY, "linear_terms": n_terms,
                    "scratch_mb": mb,
                    "tile_rows": 256 if name == "linear_feat_hbm" else lin.linear_tile_rows(dtype),
                    "ms_median": round(med[name], 4), "ms_min": round(min(t), 4),
                    "ms_max": round(max(t), 4), "rows_per_s": round(a.rows / (med[name] * 1e-3), 1),
                    "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
                    "sample_rows": SAMPLE, "sample_equals_cpu_evaluator": same,
                    "sample_fallback_share": round(fell, 4),
                    "device": torch.cuda.get_device_name(0)}
            if name == "linear":
                line["linear_over_const"] = round(med["linear"] / med["const"], 3)
                line["pass2_ms"] = round(med["linear"] - med["leaf_only"], 4)
                line["pass2_share"] = round((med["linear"] - med["leaf_only"]) / med["linear"], 3)
            lines.append(line)
        del X, score, leaves
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for line in lines:
            s = json.dumps(line)
            fh.write(s + "\n")
            print(s, flush=True)
    lin.close()
    const.close()


if __name__ == "__main__":
    main()
