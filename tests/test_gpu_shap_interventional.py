"""Interventional TreeSHAP on the GPU (TI_OUTPUT_CONTRIB_INTERV) against the
brute-force definition tests/shap_interv_eval.py.  Cases are (forest, request
rows, background rows); 65 crosses the 64-lane z block.  Error: |got - want| /
max(max |want| of the row, 1), as tests/test_gpu_shap.py.
scripts/shap_interv_error.py measured its maximum over CASES below
(profiles/shap_interv_error.jsonl): 3.36e-8 for float32 forests (the rounding
of the float32 output and bias margins; the arithmetic is float64), 7.78e-16
for float64.  The bound is 4 x that (1.35e-7 and 3.2e-15), below the 1e-6 and
1e-9 that TI_OUTPUT_CONTRIB holds."""
import dataclasses
import functools

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import OUT_CONTRIB_INTERV, OUT_MARGIN, TI_F32, TI_F64
from kfserving_amd.formats import lightgbm_format as lf
from tests import shap_cat_eval as sc
from tests import shap_interact_cases as ic
from tests import shap_interv_eval as iv
from tests.shap_interact_eval import scaled_error
from tests.test_gpu_shap_interact import _refused as refused_forest

pytestmark = pytest.mark.gpu

MEASURED = {TI_F64: 7.78e-16, TI_F32: 3.36e-8}
BOUND = {k: 4 * v for k, v in MEASURED.items()}


def sum_bound(f, got):
    # |sum(phi) + bias - margin| of a float32 forest at its worst: W outputs rounded once, two
    # margins (the row's, the bias's) summed in float32 over T leaves, all within `scale`
    leaves = np.abs(f.leaf_value).max(axis=1)
    scale = max(sum(leaves[f.tree_slice(t)].max() for t in range(f.n_trees)), np.abs(got).max())
    return (got.shape[-1] + 2 * f.n_trees) * 2.0 ** -24 * scale


FORESTS = {
    "xgb-f32": lambda: ic.xgb(10, 3, 8, seed=1),               # float32, LW == 1, K == 1
    "xgb-k3": lambda: ic.xgb(9, 3, 6, seed=2, K=3),            # three groups of scalar leaves
    "lgb-zero-map": lambda: sc.lgb_cat_forest(8, 15, 7, seed=3),   # float64, zero / NaN missing
    "lgb-categorical": lambda: sc.lgb_cat_forest(6, 15, 6, seed=5, cat_features=(0, 3),
                                                 n_categories=70),
    "sk-vector-averaged": ic.sk_vector_forest,                 # vector leaves, divisor 5
    "deep-repeats": lambda: sc.forest_of_trees(lf.synthetic_leafwise_trees(5, 31, 4, seed=23), 4),
    "no-covers": lambda: dataclasses.replace(ic.xgb(6, 4, 5, seed=9), cover=None),
    "xgb-k17-parts": lambda: ic.xgb(17, 2, 5, seed=6, K=17),   # > 16 groups: two group parts
}


def rows(f, n, seed):
    X = sc.rows(f, n, seed=seed, n_categories=70).astype(np.float32).astype(np.float64)
    if f.library == "sklearn":
        X[np.isnan(X)] = 0.25               # sklearn trees: no missing values
    if f.lgb_zero_map:
        X[0, 0] = 1e-36
    return X


CASES = [("xgb-f32", 65, 65), ("xgb-f32", 1, 1), ("xgb-k3", 1, 3), ("xgb-k3", 65, 1),
         ("lgb-zero-map", 65, 3), ("lgb-zero-map", 1, 65), ("lgb-categorical", 1, 65),
         ("lgb-categorical", 65, 3), ("sk-vector-averaged", 65, 65), ("deep-repeats", 65, 65),
         ("no-covers", 1, 65), ("xgb-k17-parts", 65, 3)]


@functools.lru_cache(maxsize=None)
def case(name, n, B):
    f = FORESTS[name]()
    X, Z = rows(f, n, seed=11), rows(f, B, seed=12)
    want = iv.contributions(f, X, Z)
    want.setflags(write=False)
    return f, X, Z, want


@pytest.mark.parametrize("xdtype", [np.float32, np.float64], ids=["x32", "x64"])
@pytest.mark.parametrize("name,n,B", CASES)
def test_matches_brute_force(name, n, B, xdtype):
    f, X, Z, want = case(name, n, B)
    dev = DeviceForest(f, [0])
    dev.set_background(Z)
    got = ic.predict(dev, X.astype(xdtype), OUT_CONTRIB_INTERV)
    err = scaled_error(got, want)
    print(f"{name} rows {n} B {B} {np.dtype(xdtype).name}: max scaled error {err:.3g}")
    assert got.shape == want.shape and got.dtype == dev.forest.output_dtype(OUT_CONTRIB_INTERV)
    assert err <= BOUND[f.accum_dtype]
    assert np.array_equal(got, ic.predict(dev, X.astype(xdtype), OUT_CONTRIB_INTERV))


def test_chain_of_32_features_closed_forms():
    """32 distinct features on a path, the limit.  Z = x: all zero.  Z differing
    in the one feature j that changes the leaf: phi_j = f(x) - f(z) alone."""
    f = sc.forest_of_trees(ic.chain_trees(1, 32, seed=44), 32, objective="regression")
    dev = DeviceForest(f, [0])
    x = np.full((1, 32), 5.0)               # right at every split: the deepest leaf
    dev.set_background(x)
    got = ic.predict(dev, x, OUT_CONTRIB_INTERV)
    fx = ic.predict(dev, x, OUT_MARGIN)[0, 0]
    assert not got[0, :32].any() and got[0, 32] == fx
    root = int(f.feature[0])                # z turns left at the root: its first leaf
    z = np.where(np.arange(32) == root, -5.0, x)
    dev.set_background(z)
    got = ic.predict(dev, x, OUT_CONTRIB_INTERV)
    fz = ic.predict(dev, z, OUT_MARGIN)[0, 0]
    want = np.zeros(33)
    want[root], want[32] = fx - fz, fz
    assert scaled_error(got, want[None, :]) <= BOUND[TI_F64]


def test_identities_c2_shape(monkeypatch):
    """500 x depth 8, 28 features, B = 100: efficiency, same bits twice, 1 against 7 slices."""
    f = ic.xgb(500, 8, 28, seed=21)
    X, Z = (sc.rows(f, n, seed=n, n_categories=0).astype(np.float32) for n in (65, 100))
    dev = DeviceForest(f, [0])
    dev.set_background(Z)
    got = ic.predict(dev, X, OUT_CONTRIB_INTERV)
    assert np.array_equal(got, ic.predict(dev, X, OUT_CONTRIB_INTERV))
    total = got.astype(np.float64).sum(axis=1, keepdims=True)
    assert np.abs(total - ic.predict(dev, X, OUT_MARGIN)).max() <= sum_bound(f, got)
    by_slices = {}
    for s in (1, 7):
        monkeypatch.setenv("TI_SHAP_SLICES", str(s))
        by_slices[s] = ic.predict(dev, X[:3], OUT_CONTRIB_INTERV)
    assert scaled_error(by_slices[7], by_slices[1].astype(np.float64)) <= BOUND[TI_F32]


@pytest.mark.parametrize("which,message", [
    ("xgboost-categorical", "XGBoost's rule"), ("linear-leaves", "linear leaves"),
    ("too-many-features", "n_groups"), ("path-too-long", "32 unique features")])
def test_refusals(which, message):
    """The interaction tests' refused forests: -4 from both entry points; margins still served."""
    f, _ = refused_forest(which)
    X = np.random.default_rng(5).integers(0, 5, size=(3, f.n_features)).astype(np.float64)
    dev = DeviceForest(f, [0])
    for call in (lambda: dev.set_background(X), lambda: dev.predict(X, OUT_CONTRIB_INTERV)):
        with pytest.raises(TreeInferError, match=message) as e:
            call()
        assert e.value.code == -4
        assert dev.predict(X, OUT_MARGIN).shape[0] == 3


def test_background_state():
    """No background: -1; a second one replaces the first; clearing restores -1."""
    f, X, Z, want = case("xgb-f32", 1, 1)
    dev = DeviceForest(f, [0])
    assert dev.output_shape(OUT_CONTRIB_INTERV, 5) == (5 * 9, TI_F32)
    with pytest.raises(TreeInferError, match="background") as e:
        dev.predict(X, OUT_CONTRIB_INTERV)
    assert e.value.code == -1
    dev.set_background(rows(f, 3, seed=99))
    dev.set_background(Z)
    assert scaled_error(dev.predict(X, OUT_CONTRIB_INTERV), want) <= BOUND[TI_F32]
    dev.set_background(None)
    with pytest.raises(TreeInferError, match="background") as e:
        dev.predict(X, OUT_CONTRIB_INTERV)
    assert e.value.code == -1


@pytest.mark.parametrize("K", [1, 3])
def test_plugin_explain(K):
    from kfserving_amd.xgbserver import XGBoostModel
    f = ic.xgb(9, 3, 4, seed=51, K=K if K > 1 else 0)
    Z = np.random.default_rng(1).standard_normal((5, 4)).astype(np.float32)
    model = XGBoostModel("m", "", 1, booster=f, background=Z)
    inst = [[6.8, 2.8, -4.8, 1.4], [-6.0, 3.4, 4.5, -1.6]]
    got = np.asarray(model.explain({"instances": inst, "interventional": True})["explanations"])
    assert got.shape == ((2, K, 5) if K > 1 else (2, 5))
    X = model.request_matrix({"instances": inst})
    margin = model.predict_matrix(X, OUT_MARGIN).reshape(2, -1)
    assert np.abs(got.reshape(2, -1, 5).sum(axis=2) - margin).max() <= sum_bound(f, got)
    assert scaled_error(got.reshape(2, -1), iv.contributions(f, X, Z)) <= BOUND[TI_F32]
    with pytest.raises(Exception, match="Failed to explain"):
        model.explain({"instances": inst, "interventional": True, "approx_contribs": True})
    with pytest.raises(Exception, match="Failed to explain.*background"):
        XGBoostModel("m", "", 1, booster=f).explain({"instances": inst, "interventional": True})
