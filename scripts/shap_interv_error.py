"""The scaled error of the GPU's interventional contributions
(TI_OUTPUT_CONTRIB_INTERV) against the brute-force float64 reference
tests/shap_interv_eval.py, on the cases of
tests/test_gpu_shap_interventional.py with float32 and float64 rows: one JSON
line a (case, row type), then the maximum per output type and the bound it
gives (x 4), which the test asserts.

Usage: python scripts/shap_interv_error.py [--out profiles/shap_interv_error.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TI_DEV_KNOBS", "1")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_interv_error.jsonl"))
    a = p.parse_args()
    import numpy as np
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import OUT_CONTRIB_INTERV
    from tests import shap_interact_cases as ic
    from tests import test_gpu_shap_interventional as tc
    lines, worst = [], {}
    for name, n, B in tc.CASES:
        f, X, Z, want = tc.case(name, n, B)
        dev = DeviceForest(f, [0])
        dev.set_background(Z)
        for xdt in (np.float32, np.float64):
            got = ic.predict(dev, X.astype(xdt), OUT_CONTRIB_INTERV)
            rec = {"case": name, "rows": n, "B": B, "x": np.dtype(xdt).name, "out": got.dtype.name,
                   "max_scaled_error": tc.scaled_error(got, want)}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            worst[got.dtype.name] = max(worst.get(got.dtype.name, 0.0), rec["max_scaled_error"])
        dev.close()
    for out, err in sorted(worst.items()):
        rec = {"out": out, "max_scaled_error": err, "bound": 4 * err}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
