"""Repeated calls on group-part forests in a process that never imports torch:
`python -m tests.group_parts_child`, started by
tests/test_gpu_group_parts.py::test_process_without_torch.

Under pytest, tests/conftest.py imports torch first, so libtreeinfer binds to
the HIP runtime PyTorch bundles.  A serving worker (xgbserver, lgbserver,
sklearnserver) imports no torch and gets the system's libamdhip64, a different
release: the wrong contributions DESIGN.md recorded on these forests showed
under that runtime alone, and so did wrong leaf ids, margins and labels of the
other cases and wrong contributions of a 16-group forest with no group part
on a process's second and third handle.  Scenarios: the 17-group forest's
contributions (table at its default, off, on), the kinds interleaved, margins,
predictions and leaf ids of every case, contributions of k20-sliced (also with
TI_SHAP_SLICES=2) and k33-generic with approximate contributions between, and
k16-one-part on three successive handles.  One line a scenario, "ok" or where the first wrong
call went wrong; exit status 1 if any scenario is wrong."""
import os
import sys

os.environ.setdefault("TI_DEV_KNOBS", "1")

import numpy as np

from kfserving_amd.engine import OPT_SHAP_TABLE_ROWS, DeviceForest
from kfserving_amd.forest import (OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_INTERACT, OUT_LEAF,
                                  OUT_MARGIN, OUT_PREDICT)
from tests import group_parts_cases as gp
from tests import shap_interact_cases as ic

NAMES = {OUT_MARGIN: "margin", OUT_PREDICT: "predict", OUT_LEAF: "leaf", OUT_CONTRIB: "contrib",
         OUT_CONTRIB_APPROX: "approx", OUT_INTERACT: "interact"}


def scenario(tag, name, calls, table_rows=None, xdtype=np.float32):
    """calls: (kind, rows, seed) in order on one handle; the first wrong call ends it."""
    f = gp.case(name).forest
    dev = DeviceForest(f, [0])
    verdict = "ok"
    try:
        if table_rows is not None:
            dev.set_option(OPT_SHAP_TABLE_ROWS, table_rows)
        for i, (kind, n, seed) in enumerate(calls):
            got = ic.predict(dev, gp.batch(name, n, seed).astype(xdtype), kind)
            bad = gp.wrong_elements(f, kind, got, gp.want(name, kind, n, seed))
            if bad.any():
                verdict = (f"WRONG call {i} of {len(calls)} ({NAMES[kind]}, {n} rows): "
                           f"{gp.describe_wrong(f, kind, bad)}")
                break
    finally:
        dev.close()
    print(f"{name} {tag}: {verdict}", flush=True)
    return verdict == "ok"


def main():
    ok = True
    k17 = "k17-design"
    seq17 = gp.sequence(k17)
    # DESIGN's record: the same batch six times, the table at its default
    # (built on the first call), and the other kinds and sizes before it
    for tag, seq in (("6 rows x 6, same batch", (gp.K17_6[0],) * 6), ("6 rows x 6", gp.K17_6),
                     ("70 rows x 6, same batch", (gp.K17_70[0],) * 6), ("70 rows x 6", gp.K17_70),
                     ("sizes", seq17)):
        for tab, table_rows in (("default table", None), ("table off", 0), ("table on", 1 << 30)):
            for xd in (np.float32, np.float64):
                ok &= scenario(f"contrib, {tag}, {tab}, {np.dtype(xd).name}", k17,
                               [(OUT_CONTRIB, n, s) for n, s in seq], table_rows, xd)
    ok &= scenario("margin, then contrib 70 rows x 6, table off", k17,
                   [(OUT_MARGIN,) + gp.K17_70[0]] + [(OUT_CONTRIB, n, s) for n, s in gp.K17_70], 0)
    small = [s for s in seq17 if s[0] <= 70]
    cycle = [OUT_MARGIN, OUT_CONTRIB, OUT_LEAF, OUT_INTERACT, OUT_PREDICT, OUT_CONTRIB_APPROX, OUT_CONTRIB]
    ok &= scenario("kinds interleaved", k17,
                   [(k,) + small[(i + 2) % len(small)] for i, k in enumerate(cycle * 2)])
    # margins, predictions and leaf ids of the other cases (cheap references)
    for name in ("k20-sliced", "k20-softmax", "k33-generic", "lgb-k18-f64", "sk-k20-vector"):
        seq = gp.sequence(name)
        for kind in (OUT_MARGIN, OUT_PREDICT, OUT_LEAF):
            ok &= scenario(f"{NAMES[kind]}, sizes", name, [(kind, n, s) for n, s in seq])
        mixed = [(k,) + seq[i % len(seq)] for i, k in enumerate([OUT_MARGIN, OUT_LEAF, OUT_PREDICT] * 4)]
        ok &= scenario("margin, leaf, predict interleaved", name, mixed, xdtype=np.float64)
    # contributions beyond k17-design: path slices and their partials (forced
    # to 2 as well), the generic kernel's accumulator, and the approximate
    # pass's leaf ids, each with the other kinds between
    for name in ("k20-sliced", "k33-generic"):
        seq = gp.sequence(name)
        ok &= scenario("contrib, sizes, default table", name, [(OUT_CONTRIB, n, s) for n, s in seq])
        mixed = [OUT_MARGIN, OUT_CONTRIB, OUT_LEAF, OUT_CONTRIB_APPROX, OUT_CONTRIB, OUT_PREDICT]
        ok &= scenario("contrib, approx and the rest interleaved", name,
                       [(k,) + seq[i % len(seq)] for i, k in enumerate(mixed * 2)], xdtype=np.float64)
    os.environ["TI_SHAP_SLICES"] = "2"
    try:
        ok &= scenario("contrib, sizes, TI_SHAP_SLICES=2, table off", "k20-sliced",
                       [(OUT_CONTRIB, n, s) for n, s in gp.sequence("k20-sliced")], 0)
    finally:
        del os.environ["TI_SHAP_SLICES"]
    # no group part at all: 16 groups, three handles one after another (the
    # second and third were the wrong ones)
    seq = gp.sequence("k16-one-part")
    mixed = [OUT_MARGIN, OUT_CONTRIB, OUT_LEAF, OUT_PREDICT, OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_LEAF,
             OUT_CONTRIB]
    for handle in range(3):
        ok &= scenario(f"kinds interleaved, handle {handle} of the process", "k16-one-part",
                       [(k,) + seq[i % len(seq)] for i, k in enumerate(mixed * 2)],
                       xdtype=np.float32 if handle % 2 else np.float64)
    assert "torch" not in sys.modules
    with open("/proc/self/maps") as fh:
        libs = sorted({line.split()[-1] for line in fh if "libamdhip64" in line})
    print("HIP runtime:", ", ".join(libs), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
