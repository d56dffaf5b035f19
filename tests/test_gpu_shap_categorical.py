"""TreeSHAP contributions (TI_OUTPUT_CONTRIB) of forests with LightGBM
categorical splits, on the GPU, against tests/shap_cat_eval.py (a float64
recursion on the tree, pinned by brute-force Shapley values in
tests/test_shap_cat_eval.py).

Tolerance: the project's own for float64-accumulating forests
(tests/test_gpu_shap.py): 1e-9 of the row's largest contribution (at least 1).
float32 rows are read as the same doubles.  Every parity case runs with the
coefficient table forced (TI_OPT_SHAP_TABLE_ROWS huge) and with the extend /
unwind arithmetic (0), on 130 rows: two full 64-row blocks and a ragged one.
"""
import dataclasses
import functools
import json

import numpy as np
import pytest

from kfserving_amd.engine import OPT_SHAP_TABLE_ROWS, DeviceForest, TreeInferError
from kfserving_amd.forest import (NODE_CAT_XGB, NODE_CATEGORICAL, OUT_CONTRIB, OUT_MARGIN,
                                  OUT_PREDICT)
from kfserving_amd.formats import xgboost_format as xf
from tests import shap_cat_eval as sc

pytestmark = pytest.mark.gpu

ROWS = 130
TOL = 1e-9


# ------------------------------------------------------------------ forests
def _chain_tree(rng, order, cat_feats, n_categories):
    """A 20-deep chain in LightGBM's arrays: internal node i splits feature
    order[i] and has one leaf child and node i + 1 on a random side; the
    features of ``cat_feats`` split on random category sets."""
    n_int = len(order)
    left = np.zeros(n_int, dtype=np.int64)
    right = np.zeros(n_int, dtype=np.int64)
    thr = rng.standard_normal(n_int)
    dt = (rng.integers(0, 2, size=n_int) << 1) | (rng.integers(0, 3, size=n_int) << 2)
    bounds, words = [0], []
    for i in range(n_int):
        nxt = i + 1 if i + 1 < n_int else ~n_int        # the last node owns leaves n_int - 1, n_int
        if rng.random() < 0.5:
            left[i], right[i] = nxt, ~i
        else:
            left[i], right[i] = ~i, nxt
        if order[i] in cat_feats:
            members = np.nonzero(rng.random(n_categories) < 0.5)[0]
            nw = int(members.max()) // 32 + 1
            bits = [0] * nw
            for m in members:
                bits[m // 32] |= 1 << (m % 32)
            thr[i] = len(bounds) - 1
            dt[i] = 1
            words += bits
            bounds.append(bounds[-1] + nw)
    leaf_count = rng.integers(1, 40, size=n_int + 1)
    internal_count = np.zeros(n_int, dtype=np.int64)

    def count(c):
        if c < 0:
            return int(leaf_count[~c])
        internal_count[c] = count(int(left[c])) + count(int(right[c]))
        return int(internal_count[c])
    count(0)
    return {"split_feature": np.asarray(order), "threshold": thr, "decision_type": dt,
            "left_child": left, "right_child": right,
            "leaf_value": rng.uniform(-0.05, 0.05, size=n_int + 1),
            "leaf_count": leaf_count, "internal_count": internal_count,
            "cat_boundaries": np.asarray(bounds), "cat_threshold": np.asarray(words)}


def _hand_tree():
    """node 0: x0 in {1, 33} ? node 1 : C;  node 1: x1 <= 0.5 ? node 2 : D;
    node 2: x0 in {33, 40} ? A : B.   Counts A 10, B 30, C 40, D 20."""
    return {"split_feature": np.array([0, 1, 0]), "threshold": np.array([0.0, 0.5, 1.0]),
            "decision_type": np.array([1, 0, 1]),
            "left_child": np.array([1, 2, ~0]), "right_child": np.array([~2, ~3, ~1]),
            "leaf_value": np.array([8.0, -4.0, 2.0, 5.0]),
            "leaf_count": np.array([10, 30, 40, 20]), "internal_count": np.array([100, 60, 40]),
            # {1, 33} = words 2, 2;  {33, 40} = words 0, 2 + 256
            "cat_boundaries": np.array([0, 2, 4]), "cat_threshold": np.array([2, 2, 0, 258])}


def _disjoint_tree():
    """node 0: x1 <= 0.5 ? node 1 : D;  node 1: x0 in {1, 2} ? node 2 : C;
    node 2: x0 in {5, 6} ? A : B.  No value reaches A: its element for
    feature 0 allows nothing."""
    return {"split_feature": np.array([1, 0, 0]), "threshold": np.array([0.5, 0.0, 1.0]),
            "decision_type": np.array([0, 1, 1]),
            "left_child": np.array([1, 2, ~0]), "right_child": np.array([~3, ~2, ~1]),
            "leaf_value": np.array([9.0, -4.0, 2.0, 5.0]),
            "leaf_count": np.array([5, 35, 40, 20]), "internal_count": np.array([100, 80, 40]),
            "cat_boundaries": np.array([0, 1, 2]), "cat_threshold": np.array([6, 96])}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(forest, float64 rows, categories per categorical feature)."""
    if name == "two-slices":     # 620 paths, up to 9 unique features a path
        nc = 300
        f = sc.lgb_cat_forest(20, 31, 12, 52, cat_features=(0, 3, 7), n_categories=nc,
                              edge_frac=0.25, root_trees=4)
    elif name == "table":        # every path <= 8 unique features
        nc = 70
        f = sc.lgb_cat_forest(12, 31, 6, 41, cat_features=(0, 3), n_categories=nc)
    elif name == "chains":       # two 20-deep chains over 20 distinct features
        nc = 100
        rng = np.random.default_rng(61)
        trees = [_chain_tree(rng, list(rng.permutation(20)), {2, 5, 11, 17}, nc)
                 for _ in range(2)]
        f = sc.forest_of_trees(trees, 20)
    elif name == "wide":         # W = 3 * 51 = 153 > 128 accumulators: contrib_kernel
        nc = 300
        f = sc.lgb_cat_forest(9, 15, 50, 43, cat_features=(1, 4, 40), n_categories=nc, K=3)
    elif name == "groups17":     # K = 17: parts of 16 groups and 1
        # two trees a group (nine trees would leave groups 9..16 without any,
        # which ti_forest_create refuses)
        nc = 70
        f = sc.lgb_cat_forest(34, 15, 7, 44, cat_features=(1, 4), n_categories=nc, K=17)
    elif name == "disjoint":
        nc = 10
        f = sc.forest_of_trees([_disjoint_tree()], 2)
    else:
        raise KeyError(name)
    return f, sc.rows(f, ROWS, seed=71, n_categories=nc), nc


@functools.lru_cache(maxsize=None)
def _want(name, dtype):
    """The reference for the case's rows as the device reads them in `dtype`
    (float32 differs from float64 only where a value is no float32)."""
    f, X, _ = _case(name)
    if dtype == "f64":
        want = sc.contributions(f, X)
    else:
        X32 = X.astype(np.float32).astype(np.float64)
        want = _want(name, "f64").copy()
        diff = np.nonzero(~((X32 == X) | (np.isnan(X32) & np.isnan(X))).all(axis=1))[0]
        if diff.size:
            want[diff] = sc.contributions(f, X32[diff])
    want.setflags(write=False)
    return want


def _scaled_error(got, want):
    assert got.shape == want.shape
    scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), 1.0)
    return float((np.abs(got.astype(np.float64) - want) / scale).max())


def _run(f, X, kernel):
    dev = DeviceForest(f, [0])
    try:
        dev.set_option(OPT_SHAP_TABLE_ROWS, 1 << 30 if kernel == "table" else 0)
        return dev.predict(X, OUT_CONTRIB), dev.info()
    finally:
        dev.close()


def _parity(name, dtype, kernel):
    f, X, _ = _case(name)
    Xd = X.astype(np.float32) if dtype == "f32" else X
    got, info = _run(f, Xd, kernel)
    err = _scaled_error(got, _want(name, dtype))
    print(f"{name} {dtype} {kernel}: max scaled error {err:.3g}")
    assert err <= TOL, err
    return got, info


# -------------------------------------------------------------------- cases
@pytest.mark.parametrize("kernel", ["table", "arith"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_slices_sixteen_elements(dtype, kernel):
    """620 paths (two path slices), paths of up to 9 unique features
    (MAXN = 16, past the table's 8), and every kind of merged element."""
    f, X, nc = _case("two-slices")
    kinds = sc.path_element_kinds(f)
    assert kinds["paths"] == 620 and 8 < kinds["max_unique"] <= 16, kinds
    assert min(kinds["num+cat"], kinds["cat-LL"], kinds["cat-RR"], kinds["cat-LR"]) > 0, kinds
    cat = (f.feature >= 0) & ((f.flags & NODE_CATEGORICAL) != 0)
    nw = int(f.cat_nwords[cat].max())
    for c in sc.cat_columns(f):      # the edge values of the rule are in the rows
        for v in (-1.0, -0.5, 31.0, 32.0, 32.0 * nw - 1, 32.0 * nw, 2147483647.0):
            assert np.any(X[:, c] == v), (c, v)
        assert np.any((X[:, c] == 0) & np.signbit(X[:, c]))
    _parity("two-slices", dtype, kernel)


def test_table_serves_short_paths_bit_identically():
    f, X, _ = _case("table")
    assert sc.path_element_kinds(f)["max_unique"] <= 8
    tab, info = _parity("table", "f64", "table")
    assert info["shap_table"] == 1 and info["shap_table_bytes"] > 0, info
    arith, info = _parity("table", "f64", "arith")
    assert info["shap_table"] == 0, info
    assert np.array_equal(tab, arith)


@pytest.mark.parametrize("kernel", ["table", "arith"])
def test_chains_of_twenty_features(kernel):
    """Paths of 20 unique features: MAXN = 32."""
    f, _, _ = _case("chains")
    assert sc.path_element_kinds(f)["max_unique"] == 20
    _parity("chains", "f64", kernel)


@pytest.mark.parametrize("kernel", ["table", "arith"])
def test_wide_output_takes_the_generic_kernel(kernel):
    f, _, _ = _case("wide")
    assert f.n_groups * (f.n_features + 1) > 128
    _parity("wide", "f64", kernel)


@pytest.mark.parametrize("kernel", ["table", "arith"])
def test_seventeen_groups_in_parts(kernel):
    f, _, _ = _case("groups17")
    assert f.n_groups == 17
    got, _ = _parity("groups17", "f64", kernel)
    assert got.shape == (ROWS, 17 * 8)


@pytest.mark.parametrize("kernel", ["table", "arith"])
def test_hand_computed(kernel):
    """The tree of _hand_tree.  With E the cover-weighted means
    E[node 2] = (10 * 8 + 30 * -4) / 40 = -1,  E[node 1] = (40 * -1 + 20 * 5) / 60 = 1,
    E[root] = (60 * 1 + 40 * 2) / 100 = 1.4 = v({}), and x1 = 0.25 (left at node 1):
      v({1}) = (60 * E[node 2] + 40 * 2) / 100 = 0.2
      x0 = 1  (in {1, 33}, not in {33, 40}: B):  v({0}) = (40 * -4 + 20 * 5) / 60 = -1, v({0,1}) = -4
      x0 = 33 (in both: A):                      v({0}) = (40 * 8 + 20 * 5) / 60 = 7,   v({0,1}) = 8
      x0 = 40, 64, NaN, -3 (right at the root: C): v({0}) = v({0,1}) = 2
    phi0 = ((v({0}) - v({})) + (v({0,1}) - v({1}))) / 2,
    phi1 = ((v({1}) - v({})) + (v({0,1}) - v({0}))) / 2.
    With x1 = 0.75 (right at node 1: D) and x0 = 33: v({1}) = (60 * 5 + 40 * 2) / 100 = 3.8,
    v({0}) = 7, v({0,1}) = 5."""
    f = sc.forest_of_trees([_hand_tree()], 2)
    X = np.array([[1.0, 0.25], [33.0, 0.25], [40.0, 0.25], [64.0, 0.25], [np.nan, 0.25],
                  [-3.0, 0.25], [33.0, 0.75]])
    want = np.array([[-3.3, -2.1, 1.4], [6.7, -0.1, 1.4], [1.2, -0.6, 1.4], [1.2, -0.6, 1.4],
                     [1.2, -0.6, 1.4], [1.2, -0.6, 1.4], [3.4, 0.2, 1.4]])
    Xp = np.tile(X, (19, 1))[:ROWS]
    got, _ = _run(f, Xp, kernel)
    assert _scaled_error(got, np.tile(want, (19, 1))[:ROWS]) <= TOL
    assert _scaled_error(sc.contributions(f, X), want) <= 1e-12     # and the helper agrees


@pytest.mark.parametrize("kernel", ["table", "arith"])
def test_element_that_allows_nothing(kernel):
    """Left turns on {1, 2} and then on {5, 6}: no row follows that path."""
    f, X, _ = _case("disjoint")
    assert np.all(sc.decisions(f, X)[:, 1] & sc.decisions(f, X)[:, 2] == 0)
    _parity("disjoint", "f64", kernel)


def test_efficiency_at_4096_rows():
    """sum(phi) + bias == margin where the helper cannot reach."""
    f, _, nc = _case("two-slices")
    X = sc.rows(f, 4096, seed=72, n_categories=nc)
    dev = DeviceForest(f, [0])
    try:
        c = dev.predict(X, OUT_CONTRIB).reshape(len(X), f.n_groups, -1)
        m = dev.predict(X, OUT_MARGIN).reshape(len(X), f.n_groups)
    finally:
        dev.close()
    scale = np.maximum(np.abs(c).max(axis=(1, 2)), 1.0)[:, None]
    assert (np.abs(c.sum(axis=2) - m) / scale).max() <= TOL


def test_tree_subsets_sum_to_the_whole():
    """Two tree_subset halves (bitsets kept whole, per-node arrays cut): their
    contributions add up to the forest's, bias included."""
    f, X, _ = _case("two-slices")
    whole, _ = _run(f, X, "arith")
    acc = np.zeros_like(whole)
    for r, (a, b) in enumerate(((0, 9), (9, 20))):
        sub = f.tree_subset(a, b, keep_base=r == 0)
        assert sub.cat_bits is f.cat_bits or np.array_equal(sub.cat_bits, f.cat_bits)
        part, _ = _run(sub, X, "arith")
        acc += part
    assert _scaled_error(acc, whole) <= TOL
    assert _scaled_error(whole, _want("two-slices", "f64")) <= TOL


def test_tables_are_counted_and_freed():
    """Contributions grow device_bytes by the path tables plus the two new
    arrays (a {first, nwords} per element and the sets' words); create /
    explain / close cycles give the memory back (the bound of
    tests/test_gpu_forest_memory.py: eight cycles may hold less than four
    forests)."""
    import torch
    nc = 300
    f = sc.lgb_cat_forest(300, 63, 12, 45, cat_features=(0, 3, 7), n_categories=nc)
    X = sc.rows(f, 700, seed=73, n_categories=nc)
    n_paths = 300 * 63
    n_elems = n_cat_elems = 0        # unique (categorically split) features per path, summed
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        stack = [(0, frozenset(), frozenset())]
        while stack:
            v, feats, cats = stack.pop()
            g = b + v
            if f.feature[g] < 0:
                n_elems += len(feats)
                n_cat_elems += len(cats)
                continue
            feats = feats | {int(f.feature[g])}
            if f.flags[g] & NODE_CATEGORICAL:
                cats = cats | {int(f.feature[g])}
            stack += [(int(f.left[g]), feats, cats), (int(f.right[g]), feats, cats)]
    path_tables = n_paths * 24 + n_elems * 32 + n_paths * 8 + f.n_groups * 8
    refs = n_elems * 8

    def cycle():
        dev = DeviceForest(f, [0])
        try:
            dev.set_option(OPT_SHAP_TABLE_ROWS, 0)     # no coefficient table: the path tables alone
            dev.predict(X, OUT_MARGIN)
            before = dev.info()["device_bytes"]
            dev.predict(X, OUT_CONTRIB)
            return before, dev.info()["device_bytes"]
        finally:
            dev.close()
    before, after = cycle()
    words = after - before - path_tables - refs
    print(f"predict only {before} B, path tables {path_tables} B, refs {refs} B, sets {words} B")
    # a categorical element holds between one word and the longest bitset
    assert n_cat_elems > 1000
    assert 4 * n_cat_elems <= words <= 4 * n_cat_elems * ((nc - 1) // 32 + 1), (before, after,
                                                                              words)
    assert words % 4 == 0
    assert after >= 1 << 20
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(8):
        assert cycle() == (before, after)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info(0)[0] < 4 * after


def _xgb_rule_forest():
    trees, ti = xf.synthetic_complete_trees(30, 5, 8, seed=7)
    xf.add_categorical_splits(trees, [0, 3], 70, seed=8)
    doc = xf.json_model_doc(trees, ti, 8, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    return xf.parse_xgboost_bytes(json.dumps(doc).encode())


@pytest.mark.parametrize("which", ["mixed", "xgboost"])
def test_xgboost_rule_stays_refused(which):
    if which == "xgboost":
        f = _xgb_rule_forest()
        assert np.any(f.flags & NODE_CAT_XGB)
    else:
        f, _, _ = _case("table")
        flags = f.flags.copy()
        cat = np.nonzero((f.feature >= 0) & ((flags & NODE_CATEGORICAL) != 0))[0]
        flags[cat[::2]] |= np.uint8(NODE_CAT_XGB)
        f = dataclasses.replace(f, flags=flags)
        assert not np.all(flags[cat] & NODE_CAT_XGB)
    assert f.cover is not None
    X = np.random.default_rng(5).integers(0, 70, size=(8, f.n_features)).astype(np.float64)
    dev = DeviceForest(f, [0])
    try:
        with pytest.raises(TreeInferError, match="categorical") as e:
            dev.predict(X, OUT_CONTRIB)
        assert e.value.code == -4
        assert "XGBoost" in str(e.value)
        assert dev.predict(X, OUT_MARGIN).shape == (8,)     # the handle still serves
    finally:
        dev.close()


def test_lightgbm_plugin_explains():
    from kfserving_amd.formats import lightgbm_format as lf
    from kfserving_amd.lgbserver import LightGBMModel
    names = ["age", "colour", "height", "weight"]
    trees = lf.synthetic_leafwise_trees(10, 15, 4, seed=81)
    lf.add_categorical_splits(trees, [1], 40, seed=82)
    f = sc.forest_of_trees(trees, 4, feature_names=names, objective="regression")
    assert f.feature_names == names and f.has_categorical
    X = sc.rows(f, 20, seed=83, n_categories=40)
    model = LightGBMModel("m", "", 1, booster=f)
    req = {"inputs": [{n: [None if np.isnan(v) else float(v) for v in X[:, j]]
                       for j, n in enumerate(names)}]}
    got = np.asarray(model.explain(req)["explanations"])
    assert got.shape == (20, 5)
    assert _scaled_error(got, sc.contributions(f, X)) <= TOL
    raw = np.asarray(model.predict(req)["predictions"])
    assert f.transform == 0
    np.testing.assert_allclose(got.sum(axis=1), raw, rtol=0, atol=1e-9)
    assert model.device_forest().predict(X, OUT_PREDICT).shape == (20,)
