"""Approximate (Saabas) contributions (TI_OUTPUT_CONTRIB_APPROX) on the C2
model: rows/s of ti_predict_device on resident rows, and beside them, in the
same process, the leaf ids alone (TI_OUTPUT_LEAF, which is pass 1 of the
approximate contributions) and the TreeSHAP contributions (TI_OUTPUT_CONTRIB),
so both ratios are on record.  Then the C2-shaped model with
XGBoost categorical splits, which TreeSHAP refuses: leaf ids and approximate
contributions.

Each (model, batch size) is warmed up, then timed in alternating rounds (leaf,
approx, contrib, leaf, ...), one device-event window of at least a quarter of
a second a round; a line reports the median and the spread of the rounds.
Pass 1 is the leaf-id launch; pass 2 is reported as the approximate call minus
the leaf-id call of the same round (the two passes are stream-ordered and do
not overlap, so the difference is approx_contrib_kernel plus the scratch's
stream-ordered allocation).  TI_OCC=1 makes the library print pass 2's VGPRs
and workgroups per CU once; the line goes into every record.

Usage: python scripts/bench_approx_contrib.py [--rows 4096,100000,1000000]
           [--cat-rows 100000] [--rounds 3] [--out profiles/approx_contrib_bench.jsonl]
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TI_DEV_KNOBS"] = "1"
os.environ["TI_OCC"] = "1"
WARMUP = 2


def categorical_c2():
    """The C2 trees with half the splits on features 0, 3 and 7 categorical
    (XGBoost's rule, 70 categories), through the JSON loader."""
    import bench
    from kfserving_amd.formats import xgboost_format as xf
    trees, ti = xf.synthetic_complete_trees(bench.N_TREES, bench.DEPTH, bench.N_FEAT, seed=0)
    xf.add_categorical_splits(trees, [0, 3, 7], 70, seed=8)
    doc = xf.json_model_doc(trees, ti, bench.N_FEAT, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    return xf.parse_xgboost_bytes(json.dumps(doc).encode())


def terms_per_row(forest):
    """Mean distinct features on a root-to-leaf path, summed over the trees
    (leaves weighted equally): pass 2's terms a row, from the arrays."""
    total = 0.0
    for t in range(forest.n_trees):
        b = int(forest.tree_offset[t])
        stack, n, leaves = [(0, frozenset())], 0, 0
        while stack:
            v, feats = stack.pop()
            g = b + v
            if forest.feature[g] < 0:
                n += len(feats)
                leaves += 1
                continue
            feats = feats | {int(forest.feature[g])}
            stack += [(int(forest.left[g]), feats), (int(forest.right[g]), feats)]
        total += n / leaves
    return total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="4096,100000,1000000")
    p.add_argument("--cat-rows", default="100000")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "approx_contrib_bench.jsonl"))
    a = p.parse_args()
    import torch
    import bench
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_LEAF, TI_F32
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device")
    sh = torch.cuda.current_stream().cuda_stream
    names = {OUT_LEAF: "leaf", OUT_CONTRIB_APPROX: "approx", OUT_CONTRIB: "contrib"}
    lines = []
    models = [("c2", bench.build_model()[2], a.rows, (OUT_LEAF, OUT_CONTRIB_APPROX, OUT_CONTRIB)),
              ("c2-categorical", categorical_c2(), a.cat_rows, (OUT_LEAF, OUT_CONTRIB_APPROX))]
    for model, forest, rows_arg, kinds in models:
        dev = DeviceForest(forest, [0])
        F = forest.n_features
        shape = {"model": model, "trees": forest.n_trees, "features": F,
                 "terms_per_row": terms_per_row(forest)}
        occ = {}
        for n in [int(x) for x in rows_arg.split(",") if x]:
            X = bench.device_normal(n, F, 5, "cuda:0")
            if model == "c2-categorical":       # category codes in the categorical columns
                X[:, [0, 3, 7]] = torch.floor(torch.abs(X[:, [0, 3, 7]]) * 30.0)
            outs = {k: torch.empty(n * forest.output_width(k),
                                   dtype=torch.int32 if k == OUT_LEAF else torch.float32, device="cuda")
                    for k in kinds}

            def run(kind):
                dev.predict_device(X.data_ptr(), TI_F32, n, F, F, kind, outs[kind].data_ptr(),
                                   outs[kind].numel(), stream=sh)
            if not occ:   # the library's occupancy line goes to the C stderr: catch it once
                with tempfile.TemporaryFile() as tf:
                    saved = os.dup(2)
                    os.dup2(tf.fileno(), 2)
                    try:
                        run(OUT_CONTRIB_APPROX)
                        torch.cuda.synchronize()
                    finally:
                        os.dup2(saved, 2)
                        os.close(saved)
                    tf.seek(0)
                    text = tf.read().decode("utf-8", "replace")
                sys.stderr.write(text)
                for m in re.finditer(r"block (\d+) lds (\d+) B: (-?\d+) workgroups/CU "
                                     r"\((-?\d+) waves/SIMD\), (\d+) VGPRs", text):
                    if int(m.group(1)) == 64:   # pass 2 (the walks have tiles of 256 or 512 rows)
                        occ = {"pass2_lds_bytes": int(m.group(2)), "pass2_workgroups_per_cu": int(m.group(3)),
                               "pass2_vgprs": int(m.group(5))}
            reps = {}
            for kind in kinds:
                for _ in range(WARMUP):         # first use: tables, code objects
                    run(kind)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(kind)
                e1.record()
                torch.cuda.synchronize()
                reps[kind] = max(1, min(500, int(250.0 / max(e0.elapsed_time(e1), 1e-3))))
            ms = {k: [] for k in kinds}
            for _ in range(a.rounds):
                for kind in kinds:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps[kind]):
                        run(kind)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[kind].append(e0.elapsed_time(e1) / reps[kind])
            rec = {"rows": n, "rounds": a.rounds, "warmup_calls": WARMUP, **shape, **occ}
            for kind in kinds:
                med = statistics.median(ms[kind])
                rec[names[kind]] = {"reps": reps[kind], "ms_median": med, "ms_min": min(ms[kind]),
                                    "ms_max": max(ms[kind]), "rows_per_s": n / (med * 1e-3)}
            p2 = [x - y for x, y in zip(ms[OUT_CONTRIB_APPROX], ms[OUT_LEAF])]
            rec["pass1_ms"] = rec["leaf"]["ms_median"]
            rec["pass2_ms"] = statistics.median(p2)
            rec["pass2_ms_min"], rec["pass2_ms_max"] = min(p2), max(p2)
            rec["pass2_ns_per_term"] = rec["pass2_ms"] * 1e6 / (n * shape["terms_per_row"])
            rec["approx_over_leaf_time"] = rec["approx"]["ms_median"] / rec["leaf"]["ms_median"]
            if OUT_CONTRIB in kinds:
                rec["approx_over_contrib_rate"] = rec["approx"]["rows_per_s"] / rec["contrib"]["rows_per_s"]
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            del X, outs
        dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
