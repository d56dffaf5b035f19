"""The TreeSHAP kernels on the edge cases of tests/shap_edge_cases.py: rows on
split thresholds and next to them, NaN, both zeros, the values LightGBM's zero
map folds, +-inf and +-FLT_MAX, on paths of exactly 8/9, 16/17 and 32/33
merged elements and on output widths 128/129 -- contributions in every kernel
form a case can take (coefficient table, extend / unwind arithmetic, generic
kernel, forced path slices), interactions, approximate contributions, and
float64 rows between two float32 values.  tests/test_shap_edge_cases.py shows
on the CPU that a wrong element test moves these references by more than 100 x
the bounds used here.

Bounds (shap_edge_cases.bound; scaled error = |got - want| / max(largest
|want| of the row, 1)): float64 forests 1e-9, their interactions 1e-14 on
paths of at most 20 elements and 1e-9 on longer ones; float32 forests 1e-6,
or 4 x the error of the float32 restatement of xgboost's own TreeShap on that
case rounded up to a power of ten where that is larger, never more than 1e-5.
scripts/shap_edge_error.py measures the device's errors
(profiles/shap_edge_error.jsonl).

These tests found float32 path arithmetic wrong by 1.5e-2 (contributions) and
4.3e-2 (interactions) on the 32-element XGBoost chains, and by 1.8e-6 on the
17-element ones (profiles/shap_edge_error_before.jsonl); float32 forests with
paths of more than 16 elements now take float64 path arithmetic
(kShapF32MaxN, treeinfer_shap.h) and measure 5.7e-8."""
import numpy as np
import pytest

from kfserving_amd.engine import OPT_SHAP_TABLE_ROWS, DeviceForest, TreeInferError
from kfserving_amd.forest import OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_LEAF, OUT_MARGIN, TI_F32
from oracle import xgb_ref
from tests import canon_eval
from tests import saabas_eval as sa
from tests import shap_cat_eval as sc
from tests import shap_edge_cases as ec
from tests import shap_interact_cases as ic
from tests import shap_interact_eval as si

pytestmark = pytest.mark.gpu

KNOBS = ("TI_SHAP_GENERIC", "TI_SHAP_SLICES", "TI_SHAP_F64")


def forms(name):
    """The contributions kernel forms a case can take, in the order they run:
    first the handle as it is created (no knob, the default table limit)."""
    out = ["default"]
    if ec.takes_register_kernel(name):
        if ec.max_unique(name) <= 8:
            out.append("table")
        out.append("arith")
        if name == "xgb-d8":
            out += ["table-slices2", "arith-slices2", "table-slices3", "arith-slices3"]
    return out + ["generic"]


def set_form(dev, form, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if form == "default":
        return
    dev.set_option(OPT_SHAP_TABLE_ROWS, 1 << 30 if form.startswith("table") else 0)
    if form == "generic":
        monkeypatch.setenv("TI_SHAP_GENERIC", "1")
    if "slices" in form:
        monkeypatch.setenv("TI_SHAP_SLICES", form[-1])


def _stride(X, variant):
    return X.shape[1] + ec.STRIDE_PAD if variant.endswith("-stride") else None


def _sums_to_margin(f, contrib, margin, what):
    """Each row's columns sum to the device's own margin of the same buffer,
    with the tolerances of tests/test_gpu_shap.py test_efficiency_at_scale: the
    merged elements decide as the walk does on the same values."""
    c = contrib.astype(np.float64).reshape(len(contrib), f.n_groups, -1)
    m = margin.astype(np.float64).reshape(len(contrib), f.n_groups)
    tol = 2e-4 if f.accum_dtype == TI_F32 else 1e-9
    np.testing.assert_allclose(c.sum(axis=2), m, rtol=tol, atol=tol, err_msg=what)


@pytest.mark.parametrize("variant", ec.VARIANTS)
@pytest.mark.parametrize("name", ec.CASES)
def test_contributions(name, variant, monkeypatch):
    f = ec.forest(name)
    X = ec.rows(name, variant)
    want = ec.want_contrib(name, variant)
    stride = _stride(X, variant)
    dev = DeviceForest(f, [0])
    margin = ic.predict(dev, X, OUT_MARGIN, stride=stride)
    got = {}
    try:
        for form in forms(name):
            set_form(dev, form, monkeypatch)
            out = ic.predict(dev, X, OUT_CONTRIB, stride=stride)
            got[form] = out
            what = f"{name} {variant} {form}"
            err = sa.scaled_error(out, want)
            print(f"{what}: max scaled error {err:.3g} (bound {ec.bound(name):g})")
            assert out.shape == want.shape
            assert out.dtype == (np.float32 if ec.is_f32(name) else np.float64)
            again = ic.predict(dev, X, OUT_CONTRIB, stride=stride)
            assert np.array_equal(out, again), f"{what}: two calls differ"
            assert err <= ec.bound(name), f"{what}: max scaled error {err:.3g}"
            _sums_to_margin(f, out, margin, what)
            if form.startswith("table"):
                assert dev.info()["shap_table"] == 1, what
        # the table holds the floats the arithmetic computes
        for tab in [k for k in got if k.startswith("table")]:
            assert np.array_equal(got[tab], got[tab.replace("table", "arith")]), tab
        if "table" in got:
            assert np.array_equal(got["default"], got["table"])     # 96 rows: under the default limit
        else:
            assert dev.info()["shap_table"] == 0      # never possible, never built
            if ec.takes_register_kernel(name):
                assert np.array_equal(got["default"], got["arith"])
            else:                                     # W = 129, 33 elements: generic without the knob
                assert np.array_equal(got["default"], got["generic"])
    finally:
        dev.close()


@pytest.mark.parametrize("variant", ec.VARIANTS)
@pytest.mark.parametrize("name", ec.CASES)
def test_approximate_contributions(name, variant):
    """The walk decides them, so they take the contributions' bounds."""
    f = ec.forest(name)
    X = ec.rows(name, variant)
    stride = _stride(X, variant)
    dev = DeviceForest(f, [0])
    try:
        got = ic.predict(dev, X, OUT_CONTRIB_APPROX, stride=stride)
        err = sa.scaled_error(got, ec.want_approx(name, variant))
        print(f"{name} {variant}: max scaled error {err:.3g} (bound {ec.bound(name):g})")
        assert err <= ec.bound(name)
        assert np.array_equal(got, ic.predict(dev, X, OUT_CONTRIB_APPROX, stride=stride))
        _sums_to_margin(f, got, ic.predict(dev, X, OUT_MARGIN, stride=stride), f"{name} {variant}")
    finally:
        dev.close()


@pytest.mark.parametrize("variant", ec.XDTYPES)
@pytest.mark.parametrize("name", [n for n in ec.CASES if ec.takes_interactions(n)])
def test_interactions(name, variant):
    """The first 8 rows against the reference; on all 96 the rows of each
    matrix sum to the device's own contributions and the matrix is symmetric."""
    f = ec.forest(name)
    X = ec.rows(name, variant)
    F, K = f.n_features, f.n_groups
    bound = ec.bound(name, "interact")
    dev = DeviceForest(f, [0])
    try:
        raw = ic.predict(dev, X)
        assert np.array_equal(raw, ic.predict(dev, X)), "two calls differ"
        m = ic.matrices(f, raw)
        err = si.scaled_error(m[:ec.INTERACT_ROWS], ec.want_interact(name, variant))
        c = ic.predict(dev, X, OUT_CONTRIB).astype(np.float64).reshape(len(X), K, F + 1)
        m64 = m.astype(np.float64)
        rows_err = si.scaled_error(m64.sum(axis=3), c)
        sym_err = si.scaled_error(m64, np.swapaxes(m64, 2, 3))
        print(f"{name} {variant}: max scaled error {err:.3g}, row sums vs contributions {rows_err:.3g}, "
              f"asymmetry {sym_err:.3g} (bound {bound:g})")
        assert err <= bound
        assert rows_err <= bound
        assert sym_err <= bound
        assert np.array_equal(m64[:, :, F, F], c[:, :, F])
        assert not m[:, :, F, :F].any() and not m[:, :, :F, F].any()
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["xgb-chain-33", "lgb-chain-33"])
def test_interactions_of_33_element_paths_stay_unsupported(name):
    dev = DeviceForest(ec.forest(name), [0])
    try:
        with pytest.raises(TreeInferError, match="32 unique features") as e:
            ic.predict(dev, ec.rows(name, "x32"))
        assert e.value.code == -4
        assert ic.predict(dev, ec.rows(name, "x32"), OUT_MARGIN).shape == (ec.ROWS, 1)
    finally:
        dev.close()


def test_float64_rows_between_two_float32(monkeypatch):
    """include/treeinfer.h: float64 inputs compare in float64.  A float64 value
    strictly between a canonical threshold of a float32 forest and the float32
    above it turns right, in the walk (leaf ids, margins) and in the merged
    elements of TreeSHAP alike."""
    name = "xgb-d8"
    f = ec.forest(name)
    X = ec.between_rows(name)
    trees, ti = ec.xgb_d8_raw()
    ref = xgb_ref.from_raw_trees(trees, ti, 10, 0, 0.5, "binary:logistic")
    want = sc.contributions(f, X)
    dev = DeviceForest(f, [0])
    try:
        leaf = ic.predict(dev, X, OUT_LEAF)
        assert np.array_equal(leaf, canon_eval.predict(f, X, OUT_LEAF))
        margin = ic.predict(dev, X, OUT_MARGIN)
        # the float32 nearest to each of these values is the split value itself,
        # which turns right under xgboost's x < s too
        assert np.array_equal(margin[:, 0], xgb_ref.predict(ref, X.astype(np.float32), output_margin=True))
        for form in forms(name):
            set_form(dev, form, monkeypatch)
            got = ic.predict(dev, X, OUT_CONTRIB)
            err = sa.scaled_error(got, want)
            print(f"between, {form}: max scaled error {err:.3g} (bound {ec.bound(name):g})")
            assert err <= ec.bound(name), form
            _sums_to_margin(f, got, margin, form)
    finally:
        dev.close()


def test_reach():
    """The cases land on every MAXN instantiation on both sides of each limit,
    the table is built at exactly 8 elements and not at 9, and the output
    widths are 128 and 129."""
    assert {n: ec.maxn(f"lgb-chain-{n}") for n in ec.CHAINS_LGB} == {8: 8, 9: 16, 16: 16, 17: 32, 32: 32,
                                                                     33: 0}
    assert {n: ec.maxn(f"xgb-chain-{n}") for n in ec.CHAINS_XGB} == {9: 16, 16: 16, 17: 32, 32: 32, 33: 0}
    assert ec.max_unique("xgb-d8") == 8 and ec.maxn("xgb-d8") == 8
    for name, built in (("lgb-chain-8", 1), ("xgb-d8", 1), ("w128", 1), ("lgb-chain-9", 0),
                        ("xgb-chain-9", 0), ("w129", 0)):
        dev = DeviceForest(ec.forest(name), [0])
        try:
            dev.set_option(OPT_SHAP_TABLE_ROWS, 1 << 30)
            ic.predict(dev, ec.rows(name, "x32"), OUT_CONTRIB)
            info = dev.info()
            assert info["shap_table"] == built, (name, info)
            assert (info["shap_table_bytes"] > 0) == bool(built)
        finally:
            dev.close()
    assert ec.forest("w128").output_width(OUT_CONTRIB) == 128
    assert ec.forest("w129").output_width(OUT_CONTRIB) == 129
