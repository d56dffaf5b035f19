"""The oblivious-tree walk (layout 12) beside the layout the library would
otherwise pick for the same expanded CatBoost forest.

Three seeded CatBoost documents (catboost_format.json_model_doc, 28 features,
64 borders a feature): 1,000 trees of depth 6, 1,000 of depth 8, 500 of depth
10.  Each is created twice in this process -- under TI_FORCE_LAYOUT=oblivious,
and unforced, which while layout 12 is no default is the choice of a library
without it ("parent": the binned heap, layout 3, at depths 6 and 8; a record
layout at depth 10; the script stops if that comes out as layout 12) -- and,
at depth 10, a third time on the float explicit kernel (layout 1).  All are
timed on the same resident float32 rows, PREDICT output.

Device-event windows of at least a quarter of a second each, the layouts
alternating round by round; a line per forest with each layout's median,
minimum and maximum and the spread (max - min) / median of its rounds goes to
stdout and to --out.  The margins of the layouts are compared bit for bit
before anything is timed.

Usage: python scripts/bench_oblivious.py [--rows 1000000] [--rounds 7]
           [--out profiles/oblivious_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["TI_DEV_KNOBS"] = "1"
WARMUP = 2
FEATURES = 28
FORESTS = (("d6", 1000, 6), ("d8", 1000, 8), ("d10", 500, 10))


def create(forest, env):
    from kfserving_amd.engine import DeviceForest
    os.environ.update(env)
    try:
        return DeviceForest(forest, [0])
    finally:
        for k in env:
            del os.environ[k]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1000000)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "oblivious_bench.jsonl"))
    a = p.parse_args()
    import numpy as np
    import torch
    from kfserving_amd.forest import OUT_MARGIN, OUT_PREDICT, TI_F32
    from kfserving_amd.formats import catboost_format as cf
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device")
    sh = torch.cuda.current_stream().cuda_stream
    n = a.rows
    rng = np.random.default_rng(3)
    X = rng.standard_normal((n, FEATURES)).astype(np.float32)
    X[rng.random(X.shape) < 0.001] = np.nan    # about one tile in four holds a NaN
    Xd = torch.from_numpy(X).to("cuda:0")
    lines = []
    for name, trees, depth in FORESTS:
        forest = cf.forest_from_catboost_doc(
            cf.json_model_doc(trees, depth, FEATURES, loss="Logloss", seed=depth, borders=64))
        envs = {"oblivious": {"TI_FORCE_LAYOUT": "oblivious"}, "parent": {}}
        if depth > 8:
            envs["explicit"] = {"TI_FORCE_LAYOUT": "explicit"}
        devs = {k: create(forest, env) for k, env in envs.items()}
        info = {k: d.info() for k, d in devs.items()}
        if info["oblivious"]["layout"] != 12 or info["parent"]["layout"] == 12:
            raise SystemExit("%s: layouts %s" % (name, {k: v["layout"] for k, v in info.items()}))
        out = {k: torch.empty(n, dtype=torch.float64, device="cuda:0") for k in devs}

        def run(k, kind=OUT_PREDICT):
            devs[k].predict_device(Xd.data_ptr(), TI_F32, n, FEATURES, FEATURES, kind,
                                   out[k].data_ptr(), out[k].numel(), stream=sh)
        for k in devs:
            run(k, OUT_MARGIN)
        torch.cuda.synchronize()
        if any(not torch.equal(out["oblivious"], out[k]) for k in devs):
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
            for k in devs:        # alternating: the layouts see the same drift
                ms[k].append(window(k, reps[k]))
        rec = {"forest": name, "rows": n, "x": "float32", "trees": trees, "depth": depth,
               "features": FEATURES, "rounds": a.rounds, "bit_identical_margins": True,
               "stages": info["oblivious"]["n_stages"],
               "layouts": {k: v["layout"] for k, v in info.items()}}
        for k in devs:
            med = statistics.median(ms[k])
            rec[k] = {"reps": reps[k], "ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]),
                      "spread": (max(ms[k]) - min(ms[k])) / med, "rows_per_s": n / (med * 1e-3)}
            devs[k].close()
        for k in devs:
            if k != "oblivious":
                rec[k + "_over_oblivious"] = rec[k]["ms_median"] / rec["oblivious"]["ms_median"]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
