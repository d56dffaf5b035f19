"""sklearn HistGradientBoosting on the device, held to sklearn itself: the
models of tests/hgb_cases through DeviceForest against est._raw_predict (bit
for bit), est.predict and a walk of the estimator's own nodes, on the default
layout and every layout that can be forced onto them (TI_FORCE_LAYOUT, as
tests/test_gpu_parity.py forces them).  These are the library-backed forests
with float64 input, leaf-wise trees, per-node NaN flags, infinite thresholds
and categorical splits."""
import os

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import (OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_LEAF, OUT_MARGIN,
                                  OUT_PREDICT, T_EXP)
from tests import hgb_cases as hc
from tests import saabas_eval as sa
from tests import shap_cat_eval as sc

pytestmark = pytest.mark.gpu

RTOL = 1e-5           # the project's standing bound on transformed outputs (T_EXP here)
CONTRIB_TOL = 1e-9    # the float64 bound of tests/test_gpu_shap_categorical.py / test_gpu_approx_contrib.py
BATCHES = (1, 63, 257, 1000)      # across the 64- and 256-row tiles
LAYOUT_ID = {"": None, "explicit": 1, "rexplicit": 6, "lexplicit": 7, "hexplicit": 8,
             "texplicit": 9, "cheap": 10}
# a forced record layout that does not fit a forest leaves it on another of them
RECORD = (6, 7, 8, 9)


def _dev(forest, layout=""):
    old = os.environ.get("TI_FORCE_LAYOUT")
    if layout:
        os.environ["TI_FORCE_LAYOUT"] = layout
    else:
        os.environ.pop("TI_FORCE_LAYOUT", None)
    try:
        return DeviceForest(forest, [0])
    finally:
        if old is None:
            os.environ.pop("TI_FORCE_LAYOUT", None)
        else:
            os.environ["TI_FORCE_LAYOUT"] = old


def _engine_rows(name, X):
    """The rows as the serving layer hands them to the engine (non-integer
    values on categorical columns made NaN; everything else as it is)."""
    return hc.served(name).request_matrix({"instances": np.asarray(X)})


def _parity(name, dev):
    est, f = hc.fitted(name), hc.forest(name)
    X = hc.rows()
    Xe = _engine_rows(name, X)
    raw, pred, leaf = hc.reference(name)
    K = f.n_groups
    for n in BATCHES:
        margin = dev.predict(Xe[:n], OUT_MARGIN).reshape(n, K)
        assert np.array_equal(margin, raw[:n]), (name, n, "margin")
        out = dev.predict(Xe[:n], OUT_PREDICT)
        if f.meta["classes"] is not None:
            assert np.array_equal(np.asarray(est.classes_).take(out.astype(np.int64)), pred[:n]), \
                (name, n, "labels")
        elif f.transform == T_EXP:
            np.testing.assert_allclose(out, pred[:n], rtol=RTOL, atol=0)
        else:
            assert np.array_equal(out, pred[:n]), (name, n, "predict")
        assert np.array_equal(dev.predict(Xe[:n], OUT_LEAF), leaf[:n]), (name, n, "leaf")


# ------------------------------------------------------------------- parity
@pytest.mark.parametrize("layout", ["", "explicit", "rexplicit", "lexplicit", "hexplicit",
                                    "texplicit"])
@pytest.mark.parametrize("name", hc.NUMERICAL)
def test_numerical_models_every_layout(name, layout):
    dev = _dev(hc.forest(name), layout)
    try:
        got = dev.info()["layout"]
        print(f"{name} TI_FORCE_LAYOUT={layout or '(none)'}: layout {got}")
        if layout == "explicit":
            assert got == 1
        elif layout:
            assert got == LAYOUT_ID[layout] or got in RECORD     # accepted, or another record layout
        _parity(name, dev)
    finally:
        dev.close()


@pytest.mark.parametrize("layout", ["", "explicit"])
@pytest.mark.parametrize("name", hc.CATEGORICAL)
def test_categorical_models(name, layout):
    dev = _dev(hc.forest(name), layout)
    try:
        got = dev.info()["layout"]
        print(f"{name} TI_FORCE_LAYOUT={layout or '(none)'}: layout {got}")
        assert got in (1, 10) if not layout else got == 1
        _parity(name, dev)
    finally:
        dev.close()


def test_categorical_heap_takes_the_depth_limited_model():
    """max_depth = 6: the categorical heap (layout 10) where it accepts the
    forest -- by default for XGBoost-rule forests, and forced."""
    f = hc.forest("reg-cat-d6")
    assert f.depths().max() <= 8
    ran = []
    for layout in ("", "cheap"):
        dev = _dev(f, layout)
        try:
            ran.append(dev.info()["layout"])
            _parity("reg-cat-d6", dev)
        finally:
            dev.close()
    print("layouts:", ran)
    assert 10 in ran, ran


def test_non_integer_rows_through_the_serving_layer():
    for name in ("reg-cat", "multi-cat", "reg-num"):
        f = hc.forest(name)
        X = hc.rows(300, 6, True)
        raw, _, leaf = hc.reference(name, 300, 6, True)
        dev = _dev(f)
        try:
            Xe = _engine_rows(name, X)
            assert np.array_equal(dev.predict(Xe, OUT_MARGIN).reshape(raw.shape), raw)
            assert np.array_equal(dev.predict(Xe, OUT_LEAF), leaf)
        finally:
            dev.close()


def test_float32_input_is_widened_exactly():
    """float32 rows reach the float64 forest as float32 (engine.prepare_input)
    and must read as the float64 sklearn converts them to."""
    for name in ("reg-num", "reg-cat"):
        X32 = np.clip(hc.rows(257, 7), -1e30, 1e30).astype(np.float32)      # NaN stays
        want = hc.fitted(name)._raw_predict(X32)
        dev = _dev(hc.forest(name))
        try:
            assert np.array_equal(dev.predict(X32, OUT_MARGIN).reshape(want.shape), want)
        finally:
            dev.close()


def test_large_categories_run_on_the_explicit_kernel():
    """A set that reaches category 2^24 - 1 (a 2 MiB bitset) fits no heap
    record; the forest loads and agrees with sklearn."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    rng = np.random.default_rng(3)
    cats = np.array([0.0, 5.0, 70000.0, 2.0 ** 24 - 1])
    X = np.stack([rng.standard_normal(400), rng.choice(cats, size=400)], axis=1)
    y = X[:, 0] + (X[:, 1] > 10) * 2.0 + (X[:, 1] > 1e6)
    est = HistGradientBoostingRegressor(max_iter=3, max_depth=4, categorical_features=[1],
                                        random_state=0).fit(X, y)
    f = forest_from_sklearn(est)
    assert f.has_categorical
    Xt = np.stack([rng.standard_normal(300),
                   rng.choice(np.append(cats, [1.0, 69999.0, 2.0 ** 24, np.nan]), size=300)], axis=1)
    dev = _dev(f)
    try:
        print("layout", dev.info()["layout"], "largest bitset", int(f.cat_nwords.max()), "words")
        assert np.array_equal(dev.predict(Xt, OUT_MARGIN), est._raw_predict(Xt)[:, 0])
    finally:
        dev.close()


# ------------------------------------------------------------- contributions
ROWS = 130      # two full 64-row blocks and a ragged one


def _margins(dev, f, X):
    return dev.predict(X, OUT_MARGIN).reshape(X.shape[0], f.n_groups)


@pytest.mark.parametrize("name", ["reg-num", "multi-num"])
def test_treeshap_contributions_of_numerical_models(name):
    f = hc.forest(name)
    rows = 70       # a full 64-row block and a ragged one: the reference is Python
    X = np.asarray(hc.rows(rows, 8))
    want = sc.contributions(f, X)
    dev = _dev(f)
    try:
        got = dev.predict(X, OUT_CONTRIB)
        err = sa.scaled_error(got, want)
        minus = np.isneginf(X).any(axis=1)
        print(f"{name}: max scaled error {err:.3g} (bound {CONTRIB_TOL:g}); rows with -inf "
              f"{sa.scaled_error(got[minus], want[minus]):.3g}, without "
              f"{sa.scaled_error(got[~minus], want[~minus]):.3g}")
        assert got.shape == want.shape and err <= CONTRIB_TOL
        total = got.reshape(rows, f.n_groups, f.n_features + 1).sum(axis=2)
        np.testing.assert_allclose(total, _margins(dev, f, X), rtol=CONTRIB_TOL, atol=CONTRIB_TOL)
        assert np.array_equal(_margins(dev, f, X), hc.fitted(name)._raw_predict(X))
    finally:
        dev.close()


def test_treeshap_follows_infinite_values():
    """-inf turns left at every threshold and +inf right at every finite one:
    a path element with no lower bound must take -inf (it did not: its bound
    was -inf itself under a strict compare), and `x <= +inf` sends +inf left."""
    f = hc.forest("multi-num")
    assert np.isposinf(f.threshold).any()
    rng = np.random.default_rng(12)
    X = rng.standard_normal((64, hc.F))
    X[rng.random(X.shape) < 0.3] = -np.inf
    X[rng.random(X.shape) < 0.2] = np.inf
    X[:2] = [[-np.inf] * hc.F, [np.inf] * hc.F]
    want = sc.contributions(f, X)
    dev = _dev(f)
    try:
        got = dev.predict(X, OUT_CONTRIB)
        err = sa.scaled_error(got, want)
        print(f"max scaled error {err:.3g} (bound {CONTRIB_TOL:g})")
        assert err <= CONTRIB_TOL
        total = got.reshape(64, f.n_groups, f.n_features + 1).sum(axis=2)
        np.testing.assert_allclose(total, hc.fitted("multi-num")._raw_predict(X),
                                   rtol=CONTRIB_TOL, atol=CONTRIB_TOL)
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["reg-cat", "multi-cat"])
def test_approximate_contributions_of_categorical_models(name):
    f = hc.forest(name)
    X = np.asarray(hc.rows(ROWS, 8))
    want = sa.contributions(f, X)
    dev = _dev(f)
    try:
        got = dev.predict(X, OUT_CONTRIB_APPROX)
        err = sa.scaled_error(got, want)
        print(f"{name}: max scaled error {err:.3g} (bound {CONTRIB_TOL:g})")
        assert got.shape == want.shape and err <= CONTRIB_TOL
        total = got.reshape(ROWS, f.n_groups, f.n_features + 1).sum(axis=2)
        np.testing.assert_allclose(total, _margins(dev, f, X), rtol=CONTRIB_TOL, atol=CONTRIB_TOL)
        assert np.array_equal(_margins(dev, f, X), hc.fitted(name)._raw_predict(X))
        # TreeSHAP of XGBoost-rule categorical nodes stays refused
        with pytest.raises(TreeInferError):
            dev.predict(X, OUT_CONTRIB)
    finally:
        dev.close()


# -------------------------------------------------------------------- serving
def test_sklearnserver_loads_a_joblib_file(tmp_path):
    import joblib
    from kfserving_amd.sklearnserver import SKLearnModel
    est = hc.fitted("multi-cat")
    joblib.dump(est, str(tmp_path / "model.joblib"))
    model = SKLearnModel("hgb", str(tmp_path))
    assert model.load()
    X = np.concatenate([hc.rows(200, 5), hc.rows(100, 6, True)])
    want = est.predict(X)
    keep = X.copy()
    assert model.predict({"instances": X.tolist()})["predictions"] == want.tolist()
    assert np.array_equal(model.predict_tensor(X), want)
    assert np.array_equal(X, keep, equal_nan=True)        # the caller's rows are untouched
    raw = est._raw_predict(X[:7])
    exp = np.asarray(model.explain({"instances": X[:7].tolist(), "approx_contribs": True})
                     ["explanations"])
    assert exp.shape == (7, 3, hc.F + 1)
    np.testing.assert_allclose(exp.sum(axis=2), raw, rtol=CONTRIB_TOL, atol=CONTRIB_TOL)
    with pytest.raises(Exception, match="infinity"):
        model.predict({"instances": [[0.0, float("inf"), 0.0, 0.0, 0.0, 0.0]]})
    with pytest.raises(Exception, match="X has 5 features, but ColumnTransformer is expecting 6"):
        model.predict({"instances": [[0.0] * 5]})
    # a regressor with the log link, served end to end
    reg = hc.fitted("poisson-num")
    os.makedirs(str(tmp_path / "reg"))
    joblib.dump(reg, str(tmp_path / "reg" / "model.joblib"))
    rmodel = SKLearnModel("hgb-reg", str(tmp_path / "reg"))
    assert rmodel.load()
    got = np.asarray(rmodel.predict({"instances": X.tolist()})["predictions"])
    np.testing.assert_allclose(got, reg.predict(X), rtol=RTOL, atol=0)
