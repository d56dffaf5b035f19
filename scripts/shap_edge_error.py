"""The scaled error of the GPU's contributions, approximate contributions and
interaction values on the edge cases of tests/shap_edge_cases.py (rows on
split thresholds, special values, paths of 8/9, 16/17 and 32/33 elements,
widths 128/129) against their float64 references: one JSON line a (case, row
type, output, kernel form), then the maximum per (output, path arithmetic,
MAXN).  tests/test_gpu_shap_edges.py asserts the bounds of
shap_edge_cases.bound on the same cases.

float32 forests are also measured with float64 path arithmetic (the developer
knob TI_SHAP_F64=1), which separates the kernel's rounding from the output's.

Usage: python scripts/shap_edge_error.py [--out profiles/shap_edge_error.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TI_DEV_KNOBS", "1")

KNOBS = ("TI_SHAP_GENERIC", "TI_SHAP_SLICES", "TI_SHAP_F64")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "shap_edge_error.jsonl"))
    a = p.parse_args()
    import numpy as np
    from kfserving_amd.engine import OPT_SHAP_TABLE_ROWS, DeviceForest
    from kfserving_amd.forest import OUT_CONTRIB, OUT_CONTRIB_APPROX
    from tests import saabas_eval as sa
    from tests import shap_edge_cases as ec
    from tests import shap_interact_cases as ic
    from tests import shap_interact_eval as si

    def forms(name):
        out = []
        if ec.takes_register_kernel(name):
            if ec.max_unique(name) <= 8:
                out.append("table")
            out.append("arith")
            if ec.is_f32(name) and ec.maxn(name) in (8, 16):
                out.append("arith-f64-forced")
            if name == "xgb-d8":
                out += ["arith-slices2", "arith-slices3"]
        return out + ["generic"]

    lines, worst = [], {}

    def note(rec, key):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        worst[key] = max(worst.get(key, 0.0), rec["max_scaled_error"])

    for name in ec.CASES:
        f = ec.forest(name)
        # float32 forests keep float32 path arithmetic on paths of <= 16 elements
        # (kShapF32MaxN, treeinfer_shap.h); the approximate pass stores float32 deltas
        math_ = "float32" if ec.is_f32(name) and ec.maxn(name) in (8, 16) else "float64"
        store_ = "float32" if ec.is_f32(name) else "float64"
        dev = DeviceForest(f, [0])
        for variant in ec.XDTYPES:
            X = ec.rows(name, variant)
            base = {"case": name, "x": variant, "max_unique": ec.max_unique(name), "maxn": ec.maxn(name),
                    "width": ec.width(name), "rows": int(X.shape[0])}
            for form in forms(name):
                for k in KNOBS:
                    os.environ.pop(k, None)
                dev.set_option(OPT_SHAP_TABLE_ROWS, 1 << 30 if form == "table" else 0)
                if form == "generic":
                    os.environ["TI_SHAP_GENERIC"] = "1"
                if "slices" in form:
                    os.environ["TI_SHAP_SLICES"] = form[-1]
                if form.endswith("f64-forced"):
                    os.environ["TI_SHAP_F64"] = "1"
                got = ic.predict(dev, X, OUT_CONTRIB)
                m = "float64-forced" if form.endswith("f64-forced") else \
                    "float64" if form == "generic" else math_
                note(dict(base, output="contrib", kernel=form, path_arithmetic=m,
                          bound=ec.bound(name),
                          max_scaled_error=sa.scaled_error(got, ec.want_contrib(name, variant))),
                     ("contrib", m, ec.maxn(name) if form != "generic" else 0))
            for k in KNOBS:
                os.environ.pop(k, None)
            got = ic.predict(dev, X, OUT_CONTRIB_APPROX)
            note(dict(base, output="approx", kernel="approx", path_arithmetic=store_, bound=ec.bound(name),
                      max_scaled_error=sa.scaled_error(got, ec.want_approx(name, variant))),
                 ("approx", store_, 0))
            if ec.takes_interactions(name):
                for forced in ([False, True] if math_ == "float32" else [False]):
                    if forced:
                        os.environ["TI_SHAP_F64"] = "1"
                    got = ic.matrices(f, ic.predict(dev, X[:ec.INTERACT_ROWS]))
                    os.environ.pop("TI_SHAP_F64", None)
                    m = "float64-forced" if forced else math_
                    g64 = got.astype(np.float64)
                    note(dict(base, output="interact", kernel="interact", path_arithmetic=m,
                              rows=ec.INTERACT_ROWS, bound=ec.bound(name, "interact"),
                              max_scaled_error=si.scaled_error(got, ec.want_interact(name, variant)),
                              max_scaled_asymmetry=si.scaled_error(g64, np.swapaxes(g64, 2, 3))),
                         ("interact", m, ec.maxn(name)))
        dev.close()
    for (output, m, maxn), err in sorted(worst.items()):
        rec = {"output": output, "path_arithmetic": m, "maxn": maxn, "max_scaled_error": err}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
