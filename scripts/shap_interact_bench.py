"""SHAP interaction values (TI_OUTPUT_INTERACT) on the C2 model: rows/s of
ti_predict_device at a few batch sizes, and beside each the plain
contributions (TI_OUTPUT_CONTRIB) of the same rows in the same process, so
the ratio is on record.

Each batch size is warmed up, then timed in alternating rounds (interactions,
contributions, interactions, ...), one device-event window a round; a line
reports the median and the spread (min, max) of the rounds.  The script sets
TI_OCC=1 with TI_DEV_KNOBS=1, which makes the library print the interaction
kernel's VGPRs and workgroups per CU (the runtime's occupancy calculator) to
stderr once; that line is caught and goes into every record.  The LDS per
workgroup is computed from the launch shape (K_SHAP_LDS_W // (F + 1)
conditioned features x (F + 1) columns x 64 lanes of the path-arithmetic
type) and checked against the line.

Usage: python scripts/shap_interact_bench.py [--rows 256,4096,16384] [--rounds 5]
           [--out profiles/shap_interact_bench.jsonl]
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
K_SHAP_LDS_W = 128          # kShapLdsW, kfserving_amd/csrc/treeinfer_shap.h
WARMUP = 3


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="256,4096,16384")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_interact_bench.jsonl"))
    a = p.parse_args()
    import torch
    import bench
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_CONTRIB, OUT_INTERACT, TI_F32
    _, _, forest = bench.build_model()
    dev = DeviceForest(forest, [0])
    F = forest.n_features
    cpb = K_SHAP_LDS_W // (F + 1)
    mt_bytes = 4 if forest.accum_dtype == TI_F32 else 8     # the path arithmetic's type
    shape = {"trees": forest.n_trees, "features": F, "conditioned_features_per_block": cpb,
             "blocks_per_group": -(-F // cpb),
             "lds_bytes_per_workgroup": min(cpb, F) * (F + 1) * 64 * mt_bytes}
    # the library's occupancy line goes to the C stderr: catch it around the first launch
    X0 = bench.device_normal(64, bench.N_FEAT, 5, "cuda:0")
    o0 = torch.empty(64 * forest.output_width(OUT_INTERACT), dtype=torch.float32, device="cuda")
    with tempfile.TemporaryFile() as tf:
        saved = os.dup(2)
        os.dup2(tf.fileno(), 2)
        try:
            dev.predict_device(X0.data_ptr(), TI_F32, 64, bench.N_FEAT, bench.N_FEAT, OUT_INTERACT,
                               o0.data_ptr(), o0.numel(),
                               stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        text = tf.read().decode("utf-8", "replace")
    sys.stderr.write(text)
    m = re.search(r"lds (\d+) B: (-?\d+) workgroups/CU \((-?\d+) waves/SIMD\), (\d+) VGPRs", text)
    if m:
        assert int(m.group(1)) == shape["lds_bytes_per_workgroup"], (m.group(0), shape)
        shape.update({"workgroups_per_cu": int(m.group(2)), "waves_per_simd": int(m.group(3)),
                      "vgprs": int(m.group(4))})
    sh = torch.cuda.current_stream().cuda_stream
    lines = []
    for n in [int(x) for x in a.rows.split(",")]:
        X = bench.device_normal(n, bench.N_FEAT, 5, "cuda:0")
        outs = {k: torch.empty(n * forest.output_width(k), dtype=torch.float32, device="cuda")
                for k in (OUT_INTERACT, OUT_CONTRIB)}

        def run(kind):
            dev.predict_device(X.data_ptr(), TI_F32, n, bench.N_FEAT, bench.N_FEAT, kind,
                               outs[kind].data_ptr(), outs[kind].numel(), stream=sh)
        # reps per round: a window of about a quarter second at the least
        reps = {}
        for kind in (OUT_INTERACT, OUT_CONTRIB):
            for _ in range(WARMUP):       # first use: path tables, coefficient table, code objects
                run(kind)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kind)
            e1.record()
            torch.cuda.synchronize()
            reps[kind] = max(1, min(200, int(250.0 / max(e0.elapsed_time(e1), 1e-3))))
        ms = {OUT_INTERACT: [], OUT_CONTRIB: []}
        for _ in range(a.rounds):
            for kind in (OUT_INTERACT, OUT_CONTRIB):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps[kind]):
                    run(kind)
                e1.record()
                torch.cuda.synchronize()
                ms[kind].append(e0.elapsed_time(e1) / reps[kind])
        rec = {"rows": n, "rounds": a.rounds, "warmup_calls": WARMUP, **shape}
        for kind, name in ((OUT_INTERACT, "interact"), (OUT_CONTRIB, "contrib")):
            med = statistics.median(ms[kind])
            rec[name] = {"reps": reps[kind], "ms_median": med, "ms_min": min(ms[kind]),
                         "ms_max": max(ms[kind]), "rows_per_s": n / (med * 1e-3),
                         "rows_per_s_min": n / (max(ms[kind]) * 1e-3),
                         "rows_per_s_max": n / (min(ms[kind]) * 1e-3)}
        rec["contrib_over_interact"] = rec["contrib"]["rows_per_s"] / rec["interact"]["rows_per_s"]
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    dev.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
