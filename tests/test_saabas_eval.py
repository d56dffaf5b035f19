"""tests/saabas_eval.py, the float64 reference of the approximate (Saabas)
contributions, pinned by a hand-computed tree, by TreeSHAP on stumps (where
the two attributions coincide) and by the efficiency property on forests of
every split rule; plus the Python plumbing of the kind (``output_width``, the
``:explain`` route's ``"approx_contribs"`` key)."""
import dataclasses
import json

import numpy as np
import pytest

from kfserving_amd.forest import (NODE_CAT_XGB, NODE_CATEGORICAL, OUT_CONTRIB, OUT_CONTRIB_APPROX,
                                  OUT_INTERACT, OUT_MARGIN, TI_F64)
from kfserving_amd.formats import xgboost_format as xf
from oracle import shap_ref
from tests import canon_eval
from tests import saabas_eval as sa
from tests import shap_cat_eval as sc
from tests import shap_interact_cases as ic


def test_hand_computed_tree():
    """x0 <= 0 ? (x1 <= 0 ? 1 : -2) : 4 with covers 8 -> (4 -> (2, 2), 4): the
    left subtree's mean is (1 * 2 - 2 * 2) / 4 = -0.5, the root's
    (-0.5 * 4 + 4 * 4) / 8 = 1.75."""
    f = ic.hand_tree()
    X = np.array([[-1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 1.0]])
    want = np.array([[-2.25, 1.5, 1.75], [-2.25, -1.5, 1.75], [2.25, 0.0, 1.75], [2.25, 0.0, 1.75]])
    assert np.array_equal(sa.contributions(f, X), want)
    assert np.array_equal(sa.node_means(f)[:2, 0], [1.75, -0.5])


def test_equals_treeshap_on_stumps():
    trees, ti = xf.synthetic_complete_trees(12, 1, 6, seed=61)
    f = xf.forest_from_raw_trees(trees, ti, 6, 0, 0.5, "binary:logistic")
    assert np.all(f.depths() == 1)
    X = sc.rows(f, 40, seed=62, n_categories=0)
    want = shap_ref.contributions(f, X)
    assert sa.scaled_error(sa.contributions(f, X), want) <= 1e-12


def _xgb_rule_forest():
    trees, ti = xf.synthetic_complete_trees(6, 3, 8, seed=7)
    xf.add_categorical_splits(trees, [0, 3], 70, seed=8)
    doc = xf.json_model_doc(trees, ti, 8, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    return xf.parse_xgboost_bytes(json.dumps(doc).encode())


@pytest.mark.parametrize("which", ["xgboost-categorical", "lightgbm-categorical", "sklearn-vector"])
def test_rows_sum_to_the_margin(which):
    if which == "xgboost-categorical":
        f = _xgb_rule_forest()
        assert np.any(f.flags & NODE_CAT_XGB)
        X = sc.rows(f, 60, seed=63, n_categories=70)
    elif which == "lightgbm-categorical":
        f = sc.lgb_cat_forest(8, 15, 8, seed=5, cat_features=(0, 3), n_categories=70)
        assert np.any(f.flags & NODE_CATEGORICAL) and f.lgb_zero_map
        X = sc.rows(f, 60, seed=64, n_categories=70)
        assert np.isnan(X).any() and (X == 0).any()
    else:
        f = ic.sk_vector_forest()
        assert f.leaf_width == f.n_groups == 3 and f.average_divisor > 1
        X = sc.rows(f, 60, seed=65, n_categories=0)
        X[np.isnan(X)] = 0.25
    got = sa.contributions(f, X).reshape(60, f.n_groups, f.n_features + 1)
    # the margin summed in float64 whatever the forest's own accumulator is
    margin = canon_eval.predict(dataclasses.replace(f, accum_dtype=TI_F64), X, OUT_MARGIN)
    margin = np.asarray(margin, dtype=np.float64).reshape(60, f.n_groups)
    scale = np.maximum(np.abs(got).max(axis=2), 1.0)
    assert (np.abs(got.sum(axis=2) - margin) / scale).max() <= 1e-12


def test_output_width():
    f = ic.xgb(9, 3, 8, seed=2, K=3)
    assert f.output_width(OUT_CONTRIB_APPROX) == f.output_width(OUT_CONTRIB) == 3 * 9
    assert OUT_CONTRIB_APPROX == 5


@pytest.mark.parametrize("K", [1, 3])
def test_explain_route_keys(K):
    """`"approx_contribs": true` asks the device for OUT_CONTRIB_APPROX and is
    shaped as the plain request; with `"pred_interactions": true` it is an
    error naming both keys."""
    from kfserving_amd.xgbserver import XGBoostModel
    f = ic.xgb(3 * max(K, 1), 2, 4, seed=51, K=K if K > 1 else 0)
    model = XGBoostModel("m", "", 1, booster=f)
    kinds = []

    def predict_matrix(X, kind):
        kinds.append(kind)
        w = f.output_width(kind)
        return np.arange(X.shape[0] * w, dtype=np.float32).reshape(X.shape[0], w)
    model.predict_matrix = predict_matrix
    rows = [[6.8, 2.8, -4.8, 1.4], [-6.0, 3.4, 4.5, -1.6]]
    shape = (2, K, 5) if K > 1 else (2, 5)
    got = np.asarray(model.explain({"instances": rows, "approx_contribs": True})["explanations"])
    assert got.shape == shape and kinds == [OUT_CONTRIB_APPROX]
    assert np.array_equal(got.ravel(), np.arange(got.size))
    for req in ({"instances": rows}, {"instances": rows, "approx_contribs": False},
                {"instances": rows, "approx_contribs": 1}):
        assert np.asarray(model.explain(req)["explanations"]).shape == shape
    assert kinds[1:] == [OUT_CONTRIB] * 3
    model.explain({"instances": rows, "pred_interactions": True, "approx_contribs": False})
    assert kinds[-1] == OUT_INTERACT
    n = len(kinds)
    with pytest.raises(Exception, match="approx_contribs.*pred_interactions"):
        model.explain({"instances": rows, "approx_contribs": True, "pred_interactions": True})
    assert len(kinds) == n
