"""Pin tests/shap_interact_eval.py, the CPU reference of the GPU's SHAP
interaction values: its conditioned recursion equals the brute-force Shapley
interaction index of the same path-dependent value function (1e-12, the bound
of tests/test_shap_cat_eval.py) on forests small enough to enumerate --
numerical splits with LightGBM's zero / NaN missing types, a feature repeated
on a path, LightGBM categorical splits, three output groups -- its rows sum to
the contributions and its matrices to the margin.  Also here, needing no GPU:
the tree-sharded mode refuses the kind by name."""
import functools

import numpy as np
import pytest

from kfserving_amd.forest import OUT_INTERACT, OUT_MARGIN
from tests import canon_eval
from tests import shap_cat_eval as sc
from tests import shap_interact_eval as si

BOUND = 1e-12


@functools.lru_cache(maxsize=None)
def _case(name):
    """(forest, rows).  Leaf-wise trees of 15 leaves on at most 6 features
    repeat features on their paths; the generator draws all three missing
    types."""
    if name == "numerical":
        f = sc.lgb_cat_forest(4, 15, 5, seed=41)
        return f, sc.rows(f, 6, seed=42, n_categories=0)
    if name == "categorical":
        f = sc.lgb_cat_forest(4, 15, 6, seed=43, cat_features=(0, 3), n_categories=70)
        return f, sc.rows(f, 8, seed=44, n_categories=70)
    if name == "multiclass":
        f = sc.lgb_cat_forest(6, 9, 4, seed=45, K=3)
        return f, sc.rows(f, 5, seed=46, n_categories=0)
    raise KeyError(name)


CASES = ["numerical", "categorical", "multiclass"]


def test_cases_cover_what_they_claim():
    f, X = _case("numerical")
    assert not f.has_categorical and f.n_features <= 6
    assert sc.path_element_kinds(f)["max_unique"] < 6       # 14 splits on 5 features: repeats
    assert f.lgb_zero_map and np.isnan(X).any() and (X == 0).any()
    f, _ = _case("categorical")
    kinds = sc.path_element_kinds(f)
    assert f.has_categorical and f.n_features <= 6 and kinds["num+cat"] > 0, kinds
    f, _ = _case("multiclass")
    assert f.n_groups == 3 and f.n_features <= 6


@pytest.mark.parametrize("name", CASES)
def test_recursion_equals_brute_force_interaction_index(name):
    f, X = _case(name)
    got = si.interactions(f, X)
    assert got.shape == (X.shape[0], f.n_groups, f.n_features + 1, f.n_features + 1)
    for r in range(X.shape[0]):
        want = si.brute_force(f, X[r])
        assert np.abs(got[r] - want).max() <= BOUND, (r, np.abs(got[r] - want).max())


@pytest.mark.parametrize("name", CASES)
def test_unconditioned_recursion_is_the_contributions(name):
    f, X = _case(name)
    assert np.abs(si.contributions(f, X) - sc.contributions(f, X)).max() <= BOUND


@pytest.mark.parametrize("name", CASES)
def test_row_sums_total_and_symmetry(name):
    f, X = _case(name)
    F, K = f.n_features, f.n_groups
    m = si.interactions(f, X)
    c = sc.contributions(f, X).reshape(X.shape[0], K, F + 1)
    scale = np.maximum(np.abs(c).max(axis=(1, 2)), 1.0)[:, None]
    assert (np.abs(m.sum(axis=3) - c).max(axis=2) / scale).max() <= BOUND
    margin = canon_eval.predict(f, X, OUT_MARGIN).reshape(X.shape[0], K)
    assert (np.abs(m.sum(axis=(2, 3)) - margin) / scale).max() <= BOUND
    assert (np.abs(m - np.swapaxes(m, 2, 3)).max(axis=(2, 3)) / scale).max() <= BOUND
    # the bias row and column hold the bias alone
    assert np.array_equal(m[:, :, F, F], c[:, :, F])
    assert not m[:, :, F, :F].any() and not m[:, :, :F, F].any()


def test_tree_shard_refuses_interactions_by_name():
    """TreeShardedForest.predict used to send an unknown kind down the margin
    path; the refusal comes before anything touches a device or a process
    group."""
    from kfserving_amd.tree_shard import TreeShardedForest
    shard = TreeShardedForest.__new__(TreeShardedForest)
    with pytest.raises(ValueError, match="OUT_INTERACT"):
        shard.predict(None, OUT_INTERACT)
