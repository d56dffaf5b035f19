"""Pin tests/shap_cat_eval.py, the CPU reference of the GPU's contributions on
forests with LightGBM categorical splits: its recursion equals the brute-force
Shapley values of the same path-dependent value function on forests small
enough to enumerate, it equals oracle/shap_ref.contributions exactly where
that one answers (no categorical node), and sum(phi) + bias == margin."""
import functools

import numpy as np
import pytest

from kfserving_amd.forest import OUT_MARGIN
from oracle import shap_ref
from tests import canon_eval
from tests import shap_cat_eval as sc


@functools.lru_cache(maxsize=None)
def _forest(seed):
    return sc.lgb_cat_forest(12, 31, 6, seed, cat_features=(0, 3), n_categories=70)


@pytest.mark.parametrize("seed", [31, 32])
def test_recursion_equals_brute_force_shapley(seed):
    f = _forest(seed)
    kinds = sc.path_element_kinds(f)
    # the merged-element cases the device builder has to get right are in here
    assert kinds["paths"] == 12 * 31
    assert min(kinds["num+cat"], kinds["cat-LL"], kinds["cat-RR"], kinds["cat-LR"]) > 0, kinds
    X = sc.rows(f, 24, seed=seed + 5, n_categories=70)
    got = sc.contributions(f, X)
    for r in range(X.shape[0]):
        want = sc.brute_force(f, X[r])
        assert np.abs(got[r] - want).max() <= 1e-12, (r, np.abs(got[r] - want).max())


@pytest.mark.parametrize("K", [1, 3])
def test_equals_shap_ref_without_categorical_nodes(K):
    f = sc.lgb_cat_forest(9, 15, 7, seed=33, K=K)
    assert not f.has_categorical
    X = sc.rows(f, 20, seed=34, n_categories=0)
    assert np.array_equal(sc.contributions(f, X), shap_ref.contributions(f, X))


@pytest.mark.parametrize("K", [1, 3])
def test_efficiency(K):
    f = sc.lgb_cat_forest(9, 15, 8, seed=35, cat_features=(1, 4), n_categories=70, K=K,
                          edge_frac=0.25, root_trees=2)
    X = sc.rows(f, 40, seed=36, n_categories=70)
    c = sc.contributions(f, X).reshape(X.shape[0], K, f.n_features + 1)
    margin = canon_eval.predict(f, X, OUT_MARGIN).reshape(X.shape[0], K)
    scale = np.maximum(np.abs(c).max(axis=(1, 2)), 1.0)[:, None]
    assert (np.abs(c.sum(axis=2) - margin) / scale).max() <= 1e-12
