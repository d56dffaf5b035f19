"""SHAP interaction values on the GPU (TI_OUTPUT_INTERACT, xgboost's
pred_interactions) against tests/shap_interact_eval.py, the float64
conditioned recursion pinned by the brute-force Shapley interaction index
(tests/test_shap_interact_eval.py); plus the identities (rows sum to the
contributions, the matrix to the margin, symmetry, determinism) on a forest
the Python reference cannot reach, the refusals, and the plugin's route.

Bounds.  The scaled error is |got - want| / max(max |want| of the row, 1), as
in tests/test_gpu_shap.py.  scripts/shap_interact_error.py measured its
maximum over the cases of tests/shap_interact_cases.py, float32 and float64
rows (profiles/shap_interact_error.jsonl):

    float64 path arithmetic (LightGBM, sklearn forests)   7.8e-16  ->  bound 1e-14
    float32 path arithmetic (XGBoost forests)             2.9e-8   ->  bound 1e-6
    (float32 forests with float64 forced, TI_SHAP_F64=1:  2.9e-8: the float32
     output's rounding, so the forests keep their float32 path arithmetic)

and each bound is that maximum times 4, rounded up to a power of ten; both are
under the 1e-5 the project's goal allows."""
import dataclasses
import json

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import (NODE_CAT_XGB, OUT_CONTRIB, OUT_INTERACT, OUT_MARGIN, TI_F32,
                                  TI_F64)
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from tests import shap_cat_eval as sc
from tests import shap_interact_cases as ic
from tests import shap_interact_eval as si

pytestmark = pytest.mark.gpu

MEASURED = {TI_F64: 7.8e-16, TI_F32: 2.9e-8}     # max scaled error, by path arithmetic
BOUND = {TI_F64: 1e-14, TI_F32: 1e-6}            # 4 x MEASURED, rounded up to a power of ten


def _check(f, got, want, what=""):
    err = si.scaled_error(got, want)
    print(f"{what}: max scaled error {err:.3g} (bound {BOUND[f.accum_dtype]:g})")
    assert got.shape == want.shape
    assert err <= BOUND[f.accum_dtype], f"{what}: max scaled error {err:.3g}"


def test_hand_computed_matrix():
    """x0 <= 0 ? (x1 <= 0 ? 1 : -2) : 4 with covers 8 -> (4 -> (2, 2), 4), row
    (-1, -1).  With v(S) the cover-weighted expectation given the features in
    S: v() = 1.75, v(0) = -0.5, v(1) = 2.5, v(01) = 1, so
      Phi[0][1] = (v(01) - v(0) - v(1) + v()) / 2          =  0.375
      phi_0 = ((v(0) - v()) + (v(01) - v(1))) / 2 = -1.875,  Phi[0][0] = -2.25
      phi_1 = ((v(1) - v()) + (v(01) - v(0))) / 2 =  1.125,  Phi[1][1] =  0.75
    and the bias is v().  Every figure is a dyadic fraction: exact on the GPU."""
    f = ic.hand_tree()
    want = np.array([[-2.25, 0.375, 0.0], [0.375, 0.75, 0.0], [0.0, 0.0, 1.75]])
    dev = DeviceForest(f, [0])
    for X in (np.array([[-1.0, -1.0]]), np.array([[-1.0, -1.0]], np.float32)):
        got = ic.predict(dev, X)
        assert got.dtype == np.float64 and got.shape == (1, 9)
        assert np.array_equal(got.reshape(3, 3), want), got
    # row (-1, 1), the leaf -2: v(01) = -2, v(1) = (-2 + 4) / 2 = 1, so
    # Phi[0][1] = (-2 + 0.5 - 1 + 1.75) / 2 = -0.375, phi_0 = -2.625, phi_1 = -1.125
    got = ic.predict(dev, np.array([[-1.0, 1.0]])).reshape(3, 3)
    assert np.array_equal(got, [[-2.25, -0.375, 0.0], [-0.375, -0.75, 0.0], [0.0, 0.0, 1.75]]), got


@pytest.mark.parametrize("xdtype", [np.float32, np.float64], ids=["x32", "x64"])
@pytest.mark.parametrize("name", [n for n in ic.PARITY if n != "geometry"])
def test_matches_reference(name, xdtype):
    f, X = ic.case(name)
    dev = DeviceForest(f, [0])
    got = ic.matrices(f, ic.predict(dev, X.astype(xdtype)))
    assert got.dtype == (np.float32 if f.accum_dtype == TI_F32 else np.float64)
    _check(f, got, ic.want(name), f"{name} {np.dtype(xdtype).name}")
    if name == "unused-feature-short-rows":
        assert X.shape[1] < f.n_features
        assert not got[:, :, 6, :].any() and not got[:, :, :, 6].any()   # no tree reads feature 6
        assert got[:, :, 5, :].any()                                     # read as NaN, still a player
    if name == "xgb-k17-parts":
        assert dev.info()["n_groups"] == 17
        # a handle's later calls too (the parts write into one output in turn)
        for _ in range(2):
            assert np.array_equal(ic.matrices(f, ic.predict(dev, X.astype(xdtype))), got)


def test_every_path_length_instantiation():
    """The kernel is instantiated for paths of <= 8, <= 16 and <= 32 elements;
    the cases land on all three."""
    longest = {n: sc.path_element_kinds(ic.case(n)[0])["max_unique"]
               for n in ("lgb-missing", "chain12", "chain20")}
    assert longest["lgb-missing"] <= 8 < longest["chain12"] <= 16 < longest["chain20"] <= 32, longest
    # 20 conditioned features, 128 // 21 = 6 a block: three full blocks and one of two
    assert ic.case("chain20")[0].n_features == 20


@pytest.mark.parametrize("rows", [1, 63, 65, 130])
def test_row_counts(rows):
    f, X = ic.case("geometry")
    got = ic.matrices(f, ic.predict(DeviceForest(f, [0]), X[:rows]))
    _check(f, got, ic.want("geometry")[:rows], f"{rows} rows")


@pytest.mark.parametrize("slices", [2, 3])
def test_path_slices(slices, monkeypatch):
    """TI_SHAP_SLICES (a developer knob) cuts the 150 paths into slices whose
    partials the finishing kernel sums in slice order."""
    f, X = ic.case("lgb-missing")
    dev = DeviceForest(f, [0])
    one = ic.predict(dev, X)
    monkeypatch.setenv("TI_SHAP_SLICES", str(slices))
    got = ic.predict(dev, X)
    _check(f, ic.matrices(f, got), ic.want("lgb-missing"), f"{slices} slices")
    assert np.array_equal(got, ic.predict(dev, X))           # the order is fixed
    assert si.scaled_error(got.reshape(ic.want("lgb-missing").shape),
                           ic.matrices(f, one).astype(np.float64)) <= BOUND[TI_F64]


@pytest.mark.parametrize("kind", ["xgb-f32", "lgb-f64"])
def test_identities_at_scale(kind):
    """50 trees of depth 6 (or 63 leaves), 512 rows, 28 features in 7 blocks
    of 4 conditioned features, more than 512 paths (several slices)."""
    if kind == "xgb-f32":
        f = ic.xgb(50, 6, 28, seed=31)
    else:
        f = sc.lgb_cat_forest(50, 63, 28, seed=32, cat_features=(2, 9), n_categories=40)
    X = sc.rows(f, 512, seed=33, n_categories=40).astype(np.float32)
    F, K = f.n_features, f.n_groups
    dev = DeviceForest(f, [0])
    raw = ic.predict(dev, X)
    assert np.array_equal(raw, ic.predict(dev, X)), "two calls differ"
    m = ic.matrices(f, raw).astype(np.float64)
    c = ic.predict(dev, X, OUT_CONTRIB).astype(np.float64).reshape(512, K, F + 1)
    bound = BOUND[f.accum_dtype]
    rows_err = si.scaled_error(m.sum(axis=3), c)
    sym_err = si.scaled_error(m, np.swapaxes(m, 2, 3))
    print(f"{kind}: row sums vs contributions {rows_err:.3g}, symmetry {sym_err:.3g} (bound {bound:g})")
    assert rows_err <= bound
    assert sym_err <= bound
    assert np.array_equal(m[:, :, F, F], c[:, :, F])
    assert not m[:, :, F, :F].any() and not m[:, :, :F, F].any()
    # the total against the margin: the efficiency bound of the contributions
    # themselves (tests/test_gpu_shap.py), whose sum the matrix's sum is
    margin = ic.predict(dev, X, OUT_MARGIN).astype(np.float64).reshape(512, K)
    tol = 2e-4 if f.accum_dtype == TI_F32 else 1e-9
    np.testing.assert_allclose(m.sum(axis=(2, 3)), margin, rtol=tol, atol=tol)


def test_float32_forest_with_float64_path_arithmetic(monkeypatch):
    """TI_SHAP_F64=1 (a developer knob, the A/B of the accuracy measurement):
    a float32 forest's interactions in float64 path arithmetic, on the first
    and on later calls of a handle, for both row types."""
    f, X = ic.case("xgb-f32")
    monkeypatch.setenv("TI_SHAP_F64", "1")
    dev = DeviceForest(f, [0])
    for _ in range(3):
        for xdtype in (np.float32, np.float64):
            got = ic.matrices(f, ic.predict(dev, X.astype(xdtype)))
            _check(f, got, ic.want("xgb-f32"), f"float64 forced, {np.dtype(xdtype).name}")


def _c2_shape():
    f = ic.xgb(50, 6, 28, seed=31)
    return f, sc.rows(f, 700, seed=34, n_categories=0).astype(np.float32)


@pytest.mark.parametrize("registered", [0, 1], ids=["pinned-chunks", "registered"])
def test_host_pipeline_chunks_by_the_output_row(registered, monkeypatch):
    """TI_CHUNK_MB=1: a 28-feature float32 forest's output row is 29 * 29 * 4 =
    3,364 B against 112 B of input, so a chunk is 256 rows and 700 rows take
    three chunks on the two lanes (two streams sharing the replica's
    scratch); the same matrices as the single launch, bit for bit."""
    from kfserving_amd.engine import OPT_HOST_REGISTER
    f, X = _c2_shape()
    dev = DeviceForest(f, [0])
    want = ic.predict(dev, X)
    monkeypatch.setenv("TI_CHUNK_MB", "1")
    dev.set_option(OPT_HOST_REGISTER, registered)
    for _ in range(2):
        assert np.array_equal(ic.predict(dev, X), want)
    c = ic.predict(dev, X, OUT_CONTRIB).astype(np.float64).reshape(700, 1, 29)
    assert si.scaled_error(ic.matrices(f, want).astype(np.float64).sum(axis=3), c) <= BOUND[TI_F32]


def test_row_blocks_when_the_partials_are_bounded(monkeypatch):
    """TI_SHAP_PART_MB=1 (a developer knob) bounds the partials at 1 MiB: one
    slice of a row is 28 * 29 * 8 = 6,496 B, so the batch runs in blocks of
    128 rows (5 full and a short one), slices dropped first; same matrices."""
    f, X = _c2_shape()
    dev = DeviceForest(f, [0])
    want = ic.predict(dev, X)
    monkeypatch.setenv("TI_SHAP_PART_MB", "1")
    got = ic.predict(dev, X)
    # one slice instead of several: the sums differ in their order, not by more
    assert si.scaled_error(got, want.astype(np.float64)) <= BOUND[TI_F32]
    assert np.array_equal(got, ic.predict(dev, X))
    c = ic.predict(dev, X, OUT_CONTRIB).astype(np.float64).reshape(700, 1, 29)
    assert si.scaled_error(ic.matrices(f, got).astype(np.float64).sum(axis=3), c) <= BOUND[TI_F32]


def _xgb_rule_forest():
    trees, ti = xf.synthetic_complete_trees(6, 3, 8, seed=7)
    xf.add_categorical_splits(trees, [0, 3], 70, seed=8)
    doc = xf.json_model_doc(trees, ti, 8, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    return xf.parse_xgboost_bytes(json.dumps(doc).encode())


def _refused(which):
    if which == "no-covers":
        return dataclasses.replace(ic.xgb(4, 3, 5, seed=9), cover=None), "covers"
    if which == "xgboost-categorical":
        f = _xgb_rule_forest()
        assert np.any(f.flags & NODE_CAT_XGB)
        return f, "XGBoost's rule"
    if which == "linear-leaves":
        trees = lf.synthetic_leafwise_trees(4, 7, 4, seed=41)
        lf.add_linear_leaves(trees, 4, seed=42, max_terms=3)
        f = sc.forest_of_trees(trees, 4)
        assert f.has_linear
        return f, "linear leaves"
    if which == "too-many-features":          # 128 + 1 columns a matrix row
        return sc.forest_of_trees(lf.synthetic_leafwise_trees(2, 7, 128, seed=43), 128), "n_features"
    if which == "path-too-long":              # 33 distinct features on a path
        return sc.forest_of_trees(ic.chain_trees(1, 33, seed=44), 33), "32 unique features"
    raise KeyError(which)


@pytest.mark.parametrize("which", ["no-covers", "xgboost-categorical", "linear-leaves",
                                   "too-many-features", "path-too-long"])
def test_refusals(which):
    f, message = _refused(which)
    X = np.random.default_rng(5).integers(0, 5, size=(3, f.n_features)).astype(np.float64)
    dev = DeviceForest(f, [0])
    try:
        with pytest.raises(TreeInferError, match=message) as e:
            dev.predict(X, OUT_INTERACT)
        assert e.value.code == -4
        assert dev.predict(X, OUT_MARGIN).shape == (3,)      # the handle still serves
    finally:
        dev.close()


def test_output_shape():
    f, _ = ic.case("xgb-k3")
    dev = DeviceForest(f, [0])
    assert dev.output_shape(OUT_INTERACT, 5) == (5 * 3 * 9 * 9, TI_F32)
    assert f.output_width(OUT_INTERACT) == 3 * 9 * 9
    f, _ = ic.case("lgb-missing")
    assert DeviceForest(f, [0]).output_shape(OUT_INTERACT, 2) == (2 * 11 * 11, TI_F64)


@pytest.mark.parametrize("K", [1, 3])
def test_plugin_explain(K):
    """`"pred_interactions": true` answers matrices whose rows sum to the
    contributions the same route answers without it."""
    from kfserving_amd.xgbserver import XGBoostModel
    f = ic.xgb(9, 3, 4, seed=51, K=K if K > 1 else 0)
    model = XGBoostModel("m", "", 1, booster=f)
    rows = [[6.8, 2.8, -4.8, 1.4], [-6.0, 3.4, 4.5, -1.6]]
    plain = np.asarray(model.explain({"instances": rows})["explanations"])
    assert plain.shape == ((2, K, 5) if K > 1 else (2, 5))
    also = np.asarray(model.explain({"instances": rows, "pred_interactions": False})["explanations"])
    assert np.array_equal(plain, also)
    got = np.asarray(model.explain({"instances": rows, "pred_interactions": True})["explanations"])
    assert got.shape == ((2, K, 5, 5) if K > 1 else (2, 5, 5))
    want = si.interactions(f, model.request_matrix({"instances": rows}).astype(np.float64))
    _check(f, got.reshape(want.shape), want, f"explain K={K}")
    assert si.scaled_error(got.sum(axis=-1), plain) <= BOUND[TI_F32]
