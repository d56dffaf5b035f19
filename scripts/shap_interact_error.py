"""The scaled error of the GPU's SHAP interaction values (TI_OUTPUT_INTERACT)
against the float64 reference tests/shap_interact_eval.py, on the cases of
tests/shap_interact_cases.py with float32 and float64 rows: one JSON line a
(case, row type, path arithmetic), then the maximum per path arithmetic and
the bound it gives (x 4, rounded up to a power of ten), which
tests/test_gpu_shap_interact.py asserts.

float32-accumulator forests are measured twice: with their float32 path
arithmetic and, under the developer knob TI_SHAP_F64=1, with float64.

Usage: python scripts/shap_interact_error.py [--out profiles/shap_interact_error.jsonl]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TI_DEV_KNOBS", "1")


def bound_of(err):
    return 10.0 ** math.ceil(math.log10(4 * err)) if err > 0 else 0.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_interact_error.jsonl"))
    a = p.parse_args()
    import numpy as np
    from kfserving_amd.engine import DeviceForest
    from kfserving_amd.forest import TI_F32
    from tests import shap_interact_cases as ic
    from tests import shap_interact_eval as si
    lines, worst = [], {}
    for name in ic.PARITY:
        f, X = ic.case(name)
        want = ic.want(name)
        maths = ["float32", "float64-forced"] if f.accum_dtype == TI_F32 else ["float64"]
        for math_ in maths:
            if math_ == "float64-forced":
                os.environ["TI_SHAP_F64"] = "1"
            else:
                os.environ.pop("TI_SHAP_F64", None)
            dev = DeviceForest(f, [0])
            for xdt in (np.float32, np.float64):
                got = ic.matrices(f, ic.predict(dev, X.astype(xdt)))
                err = si.scaled_error(got, want)
                sym = si.scaled_error(got, np.swapaxes(got.astype(np.float64), 2, 3))
                rec = {"case": name, "x": np.dtype(xdt).name, "path_arithmetic": math_,
                       "out": got.dtype.name, "rows": int(X.shape[0]), "max_scaled_error": err,
                       "max_scaled_asymmetry": sym}
                lines.append(rec)
                print(json.dumps(rec), flush=True)
                worst[math_] = max(worst.get(math_, 0.0), err)
            dev.close()
    os.environ.pop("TI_SHAP_F64", None)
    for math_, err in sorted(worst.items()):
        rec = {"path_arithmetic": math_, "max_scaled_error": err, "bound": bound_of(err)}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
