"""sklearn HistGradientBoosting -> canonical forest, held to sklearn itself on
the CPU: the forest of forest_from_hist_gradient_boosting evaluated by
tests/canon_eval (the ABI's semantics in numpy) must give est._raw_predict's
margins bit for bit, est.predict's answers, and the leaf a walk of the
estimator's own nodes reaches.  SKLearnModel's request checks are held to the
errors sklearn raises on the same input."""
import copy

import numpy as np
import pytest

from kfserving_amd.forest import (NODE_CAT_XGB, NODE_CATEGORICAL, NODE_NAN_LEFT, OUT_LEAF,
                                  OUT_MARGIN, OUT_PREDICT, T_ARGMAX, T_EXP, T_HINGE, T_IDENTITY,
                                  TI_F64)
from kfserving_amd.formats.sklearn_format import (forest_from_hist_gradient_boosting,
                                                  forest_from_sklearn)
from tests import canon_eval
from tests import hgb_cases as hc

ALL = list(hc.MODELS)


def _labels(f, out):
    classes = f.meta["classes"]
    return out if classes is None else np.asarray(classes).take(out.astype(np.int64))


def _margin(f, X):
    return canon_eval.predict(f, X, OUT_MARGIN).reshape(X.shape[0], f.n_groups)


# ------------------------------------------------------------------- the forest
@pytest.mark.parametrize("name", ALL)
def test_canonical_fields(name):
    est, f = hc.fitted(name), hc.forest(name)
    kind, loss, categorical, _ = hc.MODELS[name]
    K = {"reg": 1, "clf2": 1, "clf3": 3}[kind]
    assert f.accum_dtype == TI_F64 and f.input_dtype == TI_F64
    assert f.base_first and not f.lgb_zero_map and f.leaf_width == 1 and f.average_divisor == 1.0
    assert f.n_features == hc.F and f.n_groups == K and f.n_trees == hc.MAX_ITER * K
    assert np.array_equal(f.tree_group, np.tile(np.arange(K), hc.MAX_ITER))   # iteration-major
    assert np.array_equal(f.base_margin, est._baseline_prediction[0])
    want_t = {"reg": T_EXP if loss == "poisson" else T_IDENTITY, "clf2": T_HINGE,
              "clf3": T_ARGMAX}[kind]
    assert f.transform == want_t
    assert f.has_categorical == categorical
    if kind == "reg":
        assert f.meta["classes"] is None
    else:
        assert np.array_equal(f.meta["classes"], est.classes_)
    # node fields of the first tree against the estimator's own record array
    nd = est._predictors[0][0].nodes
    s = f.tree_slice(0)
    leaf = nd["is_leaf"] != 0
    assert np.array_equal(f.feature[s] < 0, leaf)
    assert np.array_equal(f.leaf_value[s][leaf, 0], nd["value"][leaf])
    assert np.array_equal(f.cover[s], nd["count"].astype(np.float64))
    assert np.array_equal(f.leaf_id[s], np.arange(nd.shape[0]))
    num = ~leaf & (nd["is_categorical"] == 0)
    assert np.array_equal(f.threshold[s][num], nd["num_threshold"][num])
    assert np.array_equal((f.flags[s][num] & NODE_NAN_LEFT) != 0, nd["missing_go_to_left"][num] != 0)
    f.validate()


def test_models_cover_what_the_tests_claim():
    """Both values of missing_go_to_left on numerical and on categorical
    nodes, categorical features behind the estimator's permutation, an
    infinite threshold somewhere, and trees deeper than the heap layouts take."""
    for name in hc.CATEGORICAL:
        one, zero = hc.categorical_orientations(hc.fitted(name))
        print(f"{name}: categorical nodes with missing_go_to_left=1: {one}, =0 (swapped): {zero}")
        assert one > 0 and zero > 0, name
        f = hc.forest(name)
        cat = (f.flags & NODE_CATEGORICAL) != 0
        assert np.all((f.flags[cat] & (NODE_CAT_XGB | NODE_NAN_LEFT)) == (NODE_CAT_XGB | NODE_NAN_LEFT))
        assert set(np.unique(f.feature[cat])) <= set(hc.CAT_COLS)
        assert not set(np.unique(f.feature[(f.feature >= 0) & ~cat])) & set(hc.CAT_COLS)
        est = hc.fitted(name)
        assert est._preprocessor is not None and list(np.flatnonzero(est.is_categorical_)) == [1, 4]
    for name in hc.NUMERICAL:
        f = hc.forest(name)
        internal = f.feature >= 0
        nan_left = (f.flags[internal] & NODE_NAN_LEFT) != 0
        assert nan_left.any() and (~nan_left).any(), name
    assert any(np.isposinf(hc.forest(n).threshold).any() for n in ALL)
    depth = {n: int(hc.forest(n).depths().max()) for n in ALL}
    print(depth)
    assert max(depth[n] for n in hc.NUMERICAL) > 8 and max(depth[n] for n in hc.CATEGORICAL) > 8
    assert hc.forest("reg-num-d6").depths().max() <= 6 and hc.forest("reg-cat-d6").depths().max() <= 6


@pytest.mark.parametrize("name", ALL)
def test_bit_exact_against_sklearn(name):
    """Integer-valued rows straight into the forest."""
    f = hc.forest(name)
    X = hc.rows()
    raw, pred, leaf = hc.reference(name)
    assert np.array_equal(_margin(f, X), raw)
    got = _labels(f, canon_eval.predict(f, X, OUT_PREDICT))
    assert np.array_equal(got, pred)
    assert np.array_equal(canon_eval.predict(f, X, OUT_LEAF), leaf)
    assert len(np.unique(raw)) > 50       # the rows spread over the leaves


@pytest.mark.parametrize("name", ALL)
def test_non_integer_rows_through_the_request_matrix(name):
    """3.5 on a categorical column is an unknown category to sklearn and
    category 3 to the canonical rule: request_matrix makes it NaN, in a copy."""
    f, model = hc.forest(name), hc.served(name)
    X = hc.rows(300, 6, True)
    raw, pred, leaf = hc.reference(name, 300, 6, True)
    keep = X.copy()
    Xe = model.request_matrix({"instances": np.asarray(X)})
    assert np.array_equal(X, keep, equal_nan=True)
    assert Xe.dtype == np.float64
    assert np.array_equal(_margin(f, Xe), raw)
    assert np.array_equal(_labels(f, canon_eval.predict(f, Xe, OUT_PREDICT)), pred)
    assert np.array_equal(canon_eval.predict(f, Xe, OUT_LEAF), leaf)
    if hc.MODELS[name][2]:
        assert Xe is not X and np.isnan(Xe[:, list(hc.CAT_COLS)]).sum() > \
            np.isnan(X[:, list(hc.CAT_COLS)]).sum()
        # and the gap is real: unprepared rows differ somewhere
        assert not np.array_equal(_margin(f, X), raw)
    else:
        assert np.array_equal(Xe, X, equal_nan=True)


def test_float32_input_is_widened_exactly():
    """A float32 matrix is what sklearn converts to float64."""
    f = hc.forest("reg-cat")
    X32 = np.clip(hc.rows(200, 7), -1e30, 1e30).astype(np.float32)      # NaN stays
    want = hc.fitted("reg-cat")._raw_predict(X32)
    assert np.array_equal(_margin(f, X32.astype(np.float64)), want)


def test_largest_category_is_accepted():
    """Categories up to 2^24 - 1 load: the cap is the rule's own, no layout's."""
    from sklearn.ensemble import HistGradientBoostingRegressor
    rng = np.random.default_rng(3)
    cats = np.array([0.0, 5.0, 70000.0, 2.0 ** 24 - 1])
    X = np.stack([rng.standard_normal(400), rng.choice(cats, size=400)], axis=1)
    y = X[:, 0] + (X[:, 1] > 10) * 2.0 + (X[:, 1] > 1e6)
    est = HistGradientBoostingRegressor(max_iter=3, categorical_features=[1], random_state=0).fit(X, y)
    f = forest_from_sklearn(est)
    assert f.has_categorical and f.cat_nwords.max() <= (1 << 24) // 32
    Xt = np.stack([rng.standard_normal(64), rng.choice(np.append(cats, [1.0, 2.0 ** 24, np.nan]),
                                                       size=64)], axis=1)
    assert np.array_equal(_margin(f, Xt), est._raw_predict(Xt))


# -------------------------------------------------------------------- refusals
def _fit_with_categories(values):
    from sklearn.ensemble import HistGradientBoostingRegressor
    rng = np.random.default_rng(4)
    X = np.stack([rng.standard_normal(300), rng.choice(np.asarray(values, dtype=np.float64), 300)],
                 axis=1)
    return HistGradientBoostingRegressor(max_iter=2, categorical_features=[1],
                                         random_state=0).fit(X, X[:, 0] + X[:, 1] % 2)


@pytest.mark.parametrize("values,message", [
    ([0, 1, -2, 3], r"categorical feature 1: negative category -2"),
    ([0, 1, 2.5, 3], r"categorical feature 1: non-integer category 2\.5"),
    ([0, 1, 2.0 ** 24, 3], r"categorical feature 1: category 1\.67772e\+07 >= 2\^24"),
])
def test_refused_categories(values, message):
    with pytest.raises(ValueError, match=message):
        forest_from_sklearn(_fit_with_categories(values))


def test_refused_string_categories():
    """String categories, as a DataFrame's: nothing numeric to put in a bitset."""
    est = copy.deepcopy(hc.fitted("reg-cat"))
    enc = est._preprocessor.named_transformers_["encoder"]
    enc.categories_[1] = np.array(["a", "b", "c"], dtype=object)
    with pytest.raises(ValueError, match=r"categorical feature 4: categories of dtype object are "
                                         r"not numeric"):
        forest_from_sklearn(est)


@pytest.mark.parametrize("attr", ["_predictors", "_baseline_prediction", "_preprocessor",
                                  "_bin_mapper", "is_categorical_"])
def test_refused_without_the_private_attributes(attr):
    """A pickle of another sklearn version: a TypeError naming what is missing."""
    est = copy.deepcopy(hc.fitted("reg-cat"))
    delattr(est, attr)
    with pytest.raises(TypeError, match=r"lacks the private attributes of sklearn 1\.7.*" + attr):
        forest_from_hist_gradient_boosting(est)


def test_other_estimators_still_refused():
    from sklearn.linear_model import LinearRegression
    with pytest.raises(TypeError, match="not a supported tree ensemble"):
        forest_from_sklearn(LinearRegression())


# -------------------------------------------------------------- request checks
def _both(name, X):
    """(sklearn's error, ours) on the same input."""
    with pytest.raises(Exception) as theirs:
        hc.fitted(name).predict(X)
    with pytest.raises(Exception) as ours:
        hc.served(name).request_matrix({"instances": X})
    return theirs.value, ours.value


BAD = {
    "1-D": np.zeros(hc.F),
    "narrow": np.zeros((2, hc.F - 1)),
    "wide": np.zeros((2, hc.F + 2)),
    "3-D": np.zeros((2, 2, hc.F)),
}


@pytest.mark.parametrize("what", list(BAD))
@pytest.mark.parametrize("name", ["reg-num", "multi-cat"])
def test_shape_errors_are_sklearns(name, what):
    theirs, ours = _both(name, BAD[what])
    print(f"sklearn: {theirs}\nours:    {ours}")
    assert type(ours) is type(theirs) is ValueError
    assert str(theirs).startswith(str(ours))      # sklearn's 1-D message goes on with the array


def test_infinity_on_a_categorical_column_is_rejected_as_the_encoder_does():
    for v in (np.inf, -np.inf):
        X = np.array(hc.rows(8, 9))
        X[3, 4] = v
        theirs, ours = _both("binary-cat", X)
        assert type(ours) is type(theirs) is ValueError and str(ours) == str(theirs)
        # a number to the model without categorical features
        assert hc.served("binary-num").request_matrix({"instances": X}) is not None
        hc.fitted("binary-num").predict(X)


def test_what_sklearn_lets_through_passes():
    """NaN, infinity on numerical columns and float64 beyond float32."""
    X = np.array(hc.rows(16, 10))
    X[0, 0], X[1, 2], X[2, 3], X[3, 5] = np.nan, np.inf, -np.inf, 1e300
    for name in ("reg-num", "reg-cat"):
        hc.fitted(name).predict(X)
        got = hc.served(name).request_matrix({"instances": X.tolist()})
        assert got.dtype == np.float64 and got.shape == X.shape
        assert got[3, 5] == 1e300 and np.isposinf(got[1, 2]) and np.isnan(got[0, 0])


def test_no_native_route():
    """HGB forests are answered by the application route."""
    for name in ("reg-num", "reg-cat", "multi-num"):
        m = hc.served(name)
        assert m.native_v1_transform is None and m.native_v2_transform is None
