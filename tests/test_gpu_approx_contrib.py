"""Approximate (Saabas) contributions on the GPU (TI_OUTPUT_CONTRIB_APPROX,
xgboost's approx_contribs) against tests/saabas_eval.py, the float64 node-by-
node restatement pinned by tests/test_saabas_eval.py; plus the identities
(TreeSHAP on stumps, rows sum to the margin, determinism), the plumbing (row
blocks, the host pipeline, tree shards, device memory), the refusals and the
plugin's route.

Bounds.  The scaled error is |got - want| / max(max |want| of the row, 1), as
in tests/test_gpu_shap.py.

    float64 forests (LightGBM, sklearn): 1e-9, the project's bound for
        contributions (tests/test_gpu_shap.py).
    float32 forests (XGBoost): the deltas are stored as float32, summed in
        float64 accumulators and rounded once to the float32 output.  The
        largest scaled error of the parity cases below against the float64
        helper, float32 and float64 rows, is MEASURED (2.9e-8, the 17-group
        forest: the float32 output's own rounding of a bias near 0.5); BOUND
        is 4 x MEASURED rounded up to a power of ten, 1e-6, under the 1e-5 the
        project's goal allows.  The float64 forests measured 8.4e-17.
"""
import dataclasses
import json

import numpy as np
import pytest

from kfserving_amd.engine import OPT_HOST_REGISTER, DeviceForest, TreeInferError
from kfserving_amd.forest import (NODE_CAT_XGB, OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_MARGIN, TI_F32,
                                  TI_F64)
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from kfserving_amd.formats.sklearn_format import forest_from_tree_arrays
from tests import saabas_eval as sa
from tests import shap_cat_eval as sc
from tests import shap_interact_cases as ic

pytestmark = pytest.mark.gpu

MEASURED = {TI_F32: 2.9e-8, TI_F64: 8.4e-17}   # max scaled error over the cases of this file
BOUND = {TI_F64: 1e-9, TI_F32: 1e-6}           # TI_F32: 4 x MEASURED, rounded up to a power of ten
ROWS = 130                                  # two full 64-row blocks and a ragged one


def _check(f, got, want, what=""):
    err = sa.scaled_error(got, want)
    print(f"{what}: max scaled error {err:.3g} (bound {BOUND[f.accum_dtype]:g})")
    assert got.shape == want.shape
    assert got.dtype == (np.float32 if f.accum_dtype == TI_F32 else np.float64)
    assert err <= BOUND[f.accum_dtype], f"{what}: max scaled error {err:.3g}"


def _approx(dev, X):
    return ic.predict(dev, X, OUT_CONTRIB_APPROX)


def _xgb_rule_forest():
    trees, ti = xf.synthetic_complete_trees(6, 3, 8, seed=7)
    xf.add_categorical_splits(trees, [0, 3], 70, seed=8)
    doc = xf.json_model_doc(trees, ti, 8, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    return xf.parse_xgboost_bytes(json.dumps(doc).encode())


def _repeats_a_feature(f):
    """Whether some root-to-leaf path splits twice on one feature."""
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        stack = [(0, ())]
        while stack:
            v, feats = stack.pop()
            g = b + v
            if f.feature[g] < 0:
                if len(set(feats)) < len(feats):
                    return True
                continue
            feats = feats + (int(f.feature[g]),)
            stack += [(int(f.left[g]), feats), (int(f.right[g]), feats)]
    return False


def _with_single_leaf_tree():
    """Five depth-3 XGBoost trees with a tree that is one leaf in the middle."""
    trees, _ = xf.synthetic_complete_trees(5, 3, 6, seed=71)
    z = np.full(1, -1, dtype=np.int32)
    trees.insert(2, {"cleft": z, "cright": z.copy(), "sindex": np.zeros(1, dtype=np.uint32),
                     "value": np.array([0.375], dtype=np.float32),
                     "sum_hess": np.array([7.0], dtype=np.float32)})
    return xf.forest_from_raw_trees(trees, np.zeros(6, dtype=np.int32), 6, 0, 0.5, "binary:logistic")


def _vector_forest(K=3):
    """Four hand-built sklearn-shaped trees with K-class vector leaves,
    averaged: two splits each on 5 features, covers from the leaves up."""
    rng = np.random.default_rng(72 + K)
    trees = []
    for _ in range(4):
        leaf_cover = rng.integers(1, 30, size=3).astype(np.float64)
        cover = np.array([leaf_cover.sum(), leaf_cover[0] + leaf_cover[1], leaf_cover[2],
                          leaf_cover[0], leaf_cover[1]])
        value = np.zeros((5, 1, K))
        value[[2, 3, 4], 0, :] = rng.dirichlet(np.ones(K), size=3)
        trees.append({"children_left": np.array([1, 3, -1, -1, -1]),
                      "children_right": np.array([2, 4, -1, -1, -1]),
                      "feature": np.array([rng.integers(0, 5), rng.integers(0, 5), -2, -2, -2]),
                      "threshold": np.array([rng.normal(), rng.normal(), -2.0, -2.0, -2.0]),
                      "missing_go_to_left": rng.integers(0, 2, size=5).astype(np.uint8),
                      "value": value, "cover": cover})
    return forest_from_tree_arrays(trees, 5, classifier=True, n_classes=K, average=True)


def _rows(f, n, seed, n_categories=0, nan=True):
    X = sc.rows(f, n, seed=seed, n_categories=n_categories)
    if not nan:
        X[np.isnan(X)] = 0.25
    return X.astype(np.float32).astype(np.float64)


def _case(name):
    """(forest, rows: float64 values that float32 holds exactly)."""
    if name in ("xgb40", "xgb40-nan"):            # 40 trees cross the 32-tree id chunk
        trees, ti = xf.synthetic_complete_trees(40, 5, 8, seed=70)
        f = xf.forest_from_raw_trees(trees, ti, 8, 0, 0.5, "binary:logistic")
        return f, _rows(f, ROWS, 80, nan=name == "xgb40-nan")
    if name == "xgb-categorical":
        f = _xgb_rule_forest()
        return f, _rows(f, ROWS, 81, n_categories=70)
    if name == "lgb-categorical":
        f = sc.lgb_cat_forest(20, 31, 12, 52, cat_features=(0, 3, 7), n_categories=300)
        return f, _rows(f, ROWS, 82, n_categories=300)
    if name == "chain33":                         # 33 distinct features on one path
        f = sc.forest_of_trees(ic.chain_trees(1, 33, seed=44), 33)
        return f, _rows(f, ROWS, 83)
    if name == "repeated-feature":                # 14 splits a tree on 3 features
        f = sc.forest_of_trees(lf.synthetic_leafwise_trees(6, 15, 3, seed=73), 3)
        return f, _rows(f, ROWS, 84)
    if name == "single-leaf-tree":
        f = _with_single_leaf_tree()
        return f, _rows(f, ROWS, 85)
    if name == "xgb-k3":
        f = ic.xgb(9, 3, 8, seed=2, K=3)
        return f, _rows(f, ROWS, 86)
    if name == "vector-k3-averaged":
        f = _vector_forest()
        return f, _rows(f, ROWS, 87, nan=False)
    if name == "wide-k3-f300":                    # 903 columns: four column tiles
        f = ic.xgb(9, 4, 300, seed=74, K=3)
        return f, _rows(f, ROWS, 88)
    if name == "vector-k17-parts":                # two group parts, each holding every tree
        f = _vector_forest(17)
        return f, _rows(f, ROWS, 93, nan=False)
    raise KeyError(name)


PARITY = ["xgb40", "xgb40-nan", "xgb-categorical", "lgb-categorical", "chain33", "repeated-feature",
          "single-leaf-tree", "xgb-k3", "vector-k3-averaged", "wide-k3-f300", "vector-k17-parts"]
_cache = {}


def _case_and_want(name):
    if name not in _cache:
        f, X = _case(name)
        want = sa.contributions(f, X)
        want.setflags(write=False)
        _cache[name] = (f, X, want)
    return _cache[name]


@pytest.mark.parametrize("xdtype", [np.float32, np.float64], ids=["x32", "x64"])
@pytest.mark.parametrize("name", PARITY)
def test_matches_reference(name, xdtype):
    f, X, want = _case_and_want(name)
    dev = DeviceForest(f, [0])
    try:
        _check(f, _approx(dev, X.astype(xdtype)), want, f"{name} {np.dtype(xdtype).name}")
        if name == "xgb40":
            assert not np.isnan(X).any()
        if name == "xgb40-nan":
            assert np.isnan(X).any()
        if name == "xgb-categorical":
            assert np.any(f.flags & NODE_CAT_XGB)
            with pytest.raises(TreeInferError, match="XGBoost") as e:     # TreeSHAP still refuses it
                dev.predict(X, OUT_CONTRIB)
            assert e.value.code == -4
        if name == "chain33":
            assert sc.path_element_kinds(f)["max_unique"] == 33
        if name == "repeated-feature":
            assert _repeats_a_feature(f)
        if name == "single-leaf-tree":
            assert 1 in np.diff(f.tree_offset)
        if name == "vector-k3-averaged":
            assert f.leaf_width == f.n_groups == 3 and f.average_divisor == 4.0
        if name == "wide-k3-f300":
            assert f.output_width(OUT_CONTRIB_APPROX) == 903
        if name == "vector-k17-parts":
            assert f.leaf_width == 17 and dev.info()["n_groups"] == 17
    finally:
        dev.close()


@pytest.mark.parametrize("xdtype", [np.float32, np.float64], ids=["x32", "x64"])
@pytest.mark.parametrize("rows", [70, 6])
def test_seventeen_groups_repeated_calls(rows, xdtype):
    """K = 17: two group parts, each writing its columns of the one output.  Six
    calls on one handle, every one equal to the reference."""
    f = ic.xgb(17, 2, 5, seed=6, K=17)
    X = _rows(f, rows, 89)
    want = sa.contributions(f, X)
    dev = DeviceForest(f, [0])
    try:
        assert dev.info()["n_groups"] == 17
        for call in range(6):
            _check(f, _approx(dev, X.astype(xdtype)), want, f"k17 {rows} rows, call {call}")
    finally:
        dev.close()


def test_stumps_equal_treeshap():
    """On depth-1 trees Saabas' attribution is Shapley's."""
    trees, ti = xf.synthetic_complete_trees(40, 1, 6, seed=61)
    f32 = xf.forest_from_raw_trees(trees, ti, 6, 0, 0.5, "binary:logistic")
    f64 = sc.forest_of_trees(lf.synthetic_leafwise_trees(40, 2, 6, seed=75), 6)
    for f in (f32, f64):
        assert np.all(f.depths() == 1)
        X = _rows(f, ROWS, 90)
        dev = DeviceForest(f, [0])
        try:
            got = _approx(dev, X)
            shap = ic.predict(dev, X, OUT_CONTRIB)
        finally:
            dev.close()
        _check(f, got, shap.astype(np.float64), "stumps against TI_OUTPUT_CONTRIB")


@pytest.mark.parametrize("kind", ["xgb-f32", "lgb-f64"])
def test_rows_sum_to_the_margin_and_calls_repeat(kind):
    """4,096 rows of a forest the Python reference does not reach: the columns
    of a row sum to the device's own margin, within the efficiency bound the
    TreeSHAP contributions are held to (tests/test_gpu_shap_interact.py: 2e-4
    where the margin is summed in float32, 1e-9 in float64); two calls return
    the same bits."""
    if kind == "xgb-f32":
        f = ic.xgb(50, 6, 28, seed=31)
    else:
        f = sc.lgb_cat_forest(50, 63, 28, seed=32, cat_features=(2, 9), n_categories=40)
    X = sc.rows(f, 4096, seed=33, n_categories=40).astype(np.float32)
    dev = DeviceForest(f, [0])
    try:
        got = _approx(dev, X)
        assert np.array_equal(got, _approx(dev, X)), "two calls differ"
        margin = ic.predict(dev, X, OUT_MARGIN).astype(np.float64)
    finally:
        dev.close()
    tol = 2e-4 if f.accum_dtype == TI_F32 else 1e-9
    total = got.astype(np.float64).sum(axis=1, keepdims=True)
    print(f"{kind}: largest |row sum - margin| {np.abs(total - margin).max():.3g} (tolerance {tol:g})")
    np.testing.assert_allclose(total, margin, rtol=tol, atol=tol)


@pytest.mark.parametrize("slices", [1, 3])
def test_tree_slices(slices, monkeypatch):
    """A small batch cuts its trees into slices of whole 32-tree id chunks,
    summed in slice order.  130 trees are five chunks: by default 130 rows take
    five slices; TI_APPROX_SLICES (a developer knob) asks for none, or for
    three (two chunks, two chunks, and one of two trees)."""
    trees, ti = xf.synthetic_complete_trees(130, 3, 8, seed=76)
    f = xf.forest_from_raw_trees(trees, ti, 8, 0, 0.5, "binary:logistic")
    X = _rows(f, ROWS, 94)
    want = sa.contributions(f, X)
    dev = DeviceForest(f, [0])
    try:
        auto = _approx(dev, X)
        _check(f, auto, want, "130 trees, default slices")
        monkeypatch.setenv("TI_APPROX_SLICES", str(slices))
        got = _approx(dev, X)
        _check(f, got, want, f"130 trees, {slices} slice(s)")
        assert np.array_equal(got, _approx(dev, X))           # the order is fixed
    finally:
        dev.close()


def test_row_blocks(monkeypatch):
    """TI_APPROX_SCRATCH_MB=0 (a developer knob): the leaf-id scratch holds one
    64-row tile, so 300 rows take five passes over the two kernels."""
    f, _, _ = _case_and_want("lgb-categorical")
    X = _rows(f, 300, 91, n_categories=300)
    dev = DeviceForest(f, [0])
    try:
        one = _approx(dev, X)
        monkeypatch.setenv("TI_APPROX_SCRATCH_MB", "0")
        assert np.array_equal(_approx(dev, X), one)
    finally:
        dev.close()
    _check(f, one, sa.contributions(f, X), "300 rows")


@pytest.mark.parametrize("registered", [0, 1], ids=["pinned-chunks", "registered"])
def test_host_pipeline_chunks_by_the_output_row(registered, monkeypatch):
    """TI_CHUNK_MB=1: the 903-column float32 row is 3,612 B against 1,200 B of
    input, so a chunk is 256 rows and 700 rows take three chunks on the two
    lanes; the same contributions as the single launch, bit for bit."""
    f, _, _ = _case_and_want("wide-k3-f300")
    X = _rows(f, 700, 92).astype(np.float32)
    dev = DeviceForest(f, [0])
    try:
        want = _approx(dev, X)
        monkeypatch.setenv("TI_CHUNK_MB", "1")
        dev.set_option(OPT_HOST_REGISTER, registered)
        for _ in range(2):
            assert np.array_equal(_approx(dev, X), want)
    finally:
        dev.close()
    _check(f, want[:40], sa.contributions(f, X[:40]), "wide, 40 of 700 rows")


def test_tree_subsets_add_up():
    """Two tree shards (kfserving_amd/tree_shard.py), the base margin on the
    first: their outputs add up to the whole forest's."""
    f, X, want = _case_and_want("lgb-categorical")
    h = f.n_trees // 2
    parts = []
    for sub in (f.tree_subset(0, h, keep_base=True), f.tree_subset(h, f.n_trees, keep_base=False)):
        dev = DeviceForest(sub, [0])
        try:
            parts.append(_approx(dev, X))
        finally:
            dev.close()
    _check(f, parts[0] + parts[1], want, "two tree shards")


def test_tables_are_lazy_counted_and_freed():
    """Predict-only serving uploads nothing; the first approximate call grows
    device_bytes by exactly the tables (a leaf-id-indexed record per leaf, a
    16-byte term per distinct feature of each path, leaf_base, bias); create /
    explain / close cycles give the memory back (the bound of
    tests/test_gpu_shap_categorical.py::test_tables_are_counted_and_freed)."""
    import torch
    nc = 300
    f = sc.lgb_cat_forest(300, 63, 12, 45, cat_features=(0, 3, 7), n_categories=nc)
    X = sc.rows(f, 700, seed=73, n_categories=nc)
    n_terms = 0
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        stack = [(0, frozenset())]
        while stack:
            v, feats = stack.pop()
            g = b + v
            if f.feature[g] < 0:
                n_terms += len(feats)
                continue
            feats = feats | {int(f.feature[g])}
            stack += [(int(f.left[g]), feats), (int(f.right[g]), feats)]
    tables = 301 * 8 + 300 * 63 * 8 + n_terms * 16 + 8

    def cycle():
        dev = DeviceForest(f, [0])
        try:
            start = dev.info()["device_bytes"]
            dev.predict(X, OUT_MARGIN)
            before = dev.info()["device_bytes"]
            assert before == start
            _approx(dev, X)
            after = dev.info()["device_bytes"]
            _approx(dev, X)
            assert dev.info()["device_bytes"] == after
            return before, after
        finally:
            dev.close()
    before, after = cycle()
    assert after - before == tables, (before, after, tables)
    assert after >= 1 << 20
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(8):
        assert cycle() == (before, after)
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info(0)[0] < 4 * after


@pytest.mark.parametrize("which", ["no-covers", "linear-leaves"])
def test_refusals(which):
    if which == "no-covers":
        f, message = dataclasses.replace(ic.xgb(4, 3, 5, seed=9), cover=None), "covers"
    else:
        trees = lf.synthetic_leafwise_trees(4, 7, 4, seed=41)
        lf.add_linear_leaves(trees, 4, seed=42, max_terms=3)
        f, message = sc.forest_of_trees(trees, 4), "linear leaves"
        assert f.has_linear
    X = np.random.default_rng(5).integers(0, 5, size=(3, f.n_features)).astype(np.float64)
    dev = DeviceForest(f, [0])
    try:
        with pytest.raises(TreeInferError, match=message) as e:
            dev.predict(X, OUT_CONTRIB_APPROX)
        assert e.value.code == -4
        assert dev.predict(X, OUT_MARGIN).shape == (3,)      # the handle still serves
    finally:
        dev.close()


def test_output_shape():
    f = ic.xgb(9, 3, 8, seed=2, K=3)
    dev = DeviceForest(f, [0])
    assert dev.output_shape(OUT_CONTRIB_APPROX, 5) == (5 * 3 * 9, TI_F32)
    assert dev.output_shape(OUT_CONTRIB_APPROX, 5) == dev.output_shape(OUT_CONTRIB, 5)
    dev.close()
    f, _, _ = _case_and_want("lgb-categorical")
    dev = DeviceForest(f, [0])
    assert dev.output_shape(OUT_CONTRIB_APPROX, 2) == (2 * 13, TI_F64)
    dev.close()


def test_plugin_explains_a_categorical_model():
    """`"approx_contribs": true` on an XGBoost model with categorical splits,
    which the plain request refuses; both keys together are an error."""
    from kfserving_amd.xgbserver import XGBoostModel
    f = _xgb_rule_forest()
    model = XGBoostModel("m", "", 1, booster=f)
    rows = np.random.default_rng(6).integers(0, 70, size=(5, 8)).astype(np.float64).tolist()
    got = np.asarray(model.explain({"instances": rows, "approx_contribs": True})["explanations"])
    assert got.shape == (5, 9)
    want = sa.contributions(f, model.request_matrix({"instances": rows}).astype(np.float64))
    assert sa.scaled_error(got, want) <= BOUND[TI_F32]
    with pytest.raises(Exception, match="XGBoost"):
        model.explain({"instances": rows})
    with pytest.raises(Exception, match="approx_contribs.*pred_interactions"):
        model.explain({"instances": rows, "approx_contribs": True, "pred_interactions": True})
