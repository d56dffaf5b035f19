"""XGBoost categorical splits on the device: the categorical heap (layout 10)
and the explicit kernel (layout 1) against the hand-computed answers and the
scalar restatement of tests/test_xgb_categorical_format.py (``walk_doc``), and
layout 10 under LightGBM's rule against oracle/lgb_ref.

Leaves and margins are compared bit for bit: the kernels add the float32
leaves in tree order, as the restatement does.  Transformed outputs get the
project's RTOL = 1e-5.
"""
import dataclasses
import json
import os

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import OUT_CONTRIB, OUT_LEAF, OUT_MARGIN, OUT_PREDICT, TI_F32, TI_F64
from kfserving_amd.formats import load_lightgbm_model, load_xgboost_model
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from oracle import lgb_ref
from tests.test_xgb_categorical_format import (KA_FILE, KA_LEAF, KA_MARGIN, KA_X, walk_doc)

pytestmark = pytest.mark.gpu

RTOL = 1e-5
CAT_FEATURES = (0, 3, 7)
N_ROWS = 1537            # 256-row tiles: six full tiles and one of one row
LAYOUT_ID = {"": 10, "explicit": 1, "cheap": 10}


def _dev(forest, layout="", dtype=None):
    """The forest on device 0 under TI_FORCE_LAYOUT=layout; dtype float64 makes
    the binding pass X as float64 (an XGBoost forest's input is cast to float32
    otherwise), so the float64 kernels run."""
    if dtype is not None:
        forest = dataclasses.replace(
            forest, input_dtype=TI_F64 if dtype == np.float64 else TI_F32)
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


def _rows(seed, n_features=12, hi=80):
    """The value mix of the issue: categorical columns integers(-5, hi) plus a
    fraction, 5 % NaN, 1 % each of 3e9, 2^24 and -0.5; rows [512, 1024) -- two
    whole tiles -- hold no NaN at all, so the NaN-free walk runs."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N_ROWS, n_features))
    X[rng.random(X.shape) < 0.02] = np.nan        # missing numerical values too
    for j in CAT_FEATURES:
        X[:, j] = rng.integers(-5, hi, size=N_ROWS) + rng.choice([0, 0.5, 0.999], size=N_ROWS)
        X[rng.random(N_ROWS) < 0.05, j] = np.nan
        X[rng.random(N_ROWS) < 0.01, j] = 3e9
        X[rng.random(N_ROWS) < 0.01, j] = 16777216.0
        X[rng.random(N_ROWS) < 0.01, j] = -0.5
    clean = rng.standard_normal((512, n_features))
    for j in CAT_FEATURES:
        clean[:, j] = rng.integers(-5, hi, size=512) + rng.choice([0, 0.5, 0.999], size=512)
    X[512:1024] = clean
    X = X.astype(np.float32)
    assert not np.isnan(X[512:1024]).any() and np.isnan(X[:512]).any()
    return X


def _softmax32(m):
    e = np.exp(m - m.max(axis=1, keepdims=True), dtype=np.float32)
    return e / e.sum(axis=1, keepdims=True, dtype=np.float32)


def _transform(objective, margin):
    if objective == "binary:logistic":
        return (np.float32(1) / (np.float32(1) + np.exp(-margin[:, 0], dtype=np.float32)))
    if objective == "multi:softprob":
        return _softmax32(margin)
    return margin[:, 0]


_CASES = {}


def _case(name):
    """(forest, X, leaf, margin, predict) of a named model: built and walked by
    the restatement once, shared by every layout / dtype of it."""
    if name in _CASES:
        return _CASES[name]
    if name == "deep":
        trees, ti, K, objective = _deep_trees(), np.zeros(12, dtype=np.int32), 0, "binary:logistic"
    else:
        K = {"k1": 0, "k3": 3, "k20": 20}[name]
        objective = "binary:logistic" if K == 0 else "multi:softprob"
        trees, ti = xf.synthetic_complete_trees(150, 6, 12, seed=41 + K, num_class=K)
        xf.add_categorical_splits(trees, list(CAT_FEATURES), 70, seed=42 + K)
    doc = xf.json_model_doc(trees, ti, 12, K, 0.5, objective, version=(2, 0, 0))
    forest = xf.parse_xgboost_bytes(json.dumps(doc).encode())
    assert forest.has_categorical
    X = _rows(seed=50 + K)
    leaf, margin = walk_doc(doc, X)
    _CASES[name] = (forest, X, leaf, margin, _transform(objective, margin))
    return _CASES[name]


def _deep_trees():
    """Twelve depth-10 trees written node by node: a spine of ten splits (every
    other one categorical) with a leaf or a small numerical subtree hanging off
    each; not complete, so only the explicit layout takes them."""
    rng = np.random.default_rng(77)
    trees = []
    for _ in range(12):
        cleft, cright, sindex, value, cats = [], [], [], [], {}

        def new_node():
            cleft.append(-1), cright.append(-1), sindex.append(0), value.append(0.0)
            return len(cleft) - 1

        def leaf():
            n = new_node()
            value[n] = float(np.float32(rng.uniform(-0.05, 0.05)))
            return n

        def split(n, feature, cond, default_left, left, right):
            cleft[n], cright[n] = left, right
            sindex[n] = int(feature) | (int(default_left) << 31)
            value[n] = float(np.float32(cond))

        node = new_node()
        for level in range(10):
            spine_left = bool(rng.integers(0, 2))
            nxt = new_node() if level < 9 else leaf()
            if level % 3 == 1:          # a numerical stump beside the spine
                off = new_node()
                split(off, rng.integers(0, 12), rng.standard_normal(), rng.integers(0, 2),
                      leaf(), leaf())
            else:
                off = leaf()
            if level % 2 == 0:
                f = CAT_FEATURES[int(rng.integers(0, 3))]
                members = np.nonzero(rng.random(70) < 0.5)[0]
                cats[node] = members if members.size else np.array([5])
                cond = 0.0
            else:
                f, cond = int(rng.integers(0, 12)), rng.standard_normal()
            split(node, f, cond, rng.integers(0, 2), nxt if spine_left else off,
                  off if spine_left else nxt)
            node = nxt
        n = len(cleft)
        trees.append({"cleft": np.array(cleft, dtype=np.int32),
                      "cright": np.array(cright, dtype=np.int32),
                      "sindex": np.array(sindex, dtype=np.uint32),
                      "value": np.array(value, dtype=np.float32),
                      "sum_hess": np.ones(n, dtype=np.float32), "cats": cats})
    return trees


def _check(dev, X, leaf, margin, predict):
    assert np.array_equal(dev.predict(X, OUT_LEAF), leaf)
    got = dev.predict(X, OUT_MARGIN)
    assert np.array_equal(got.reshape(margin.shape), margin)
    np.testing.assert_allclose(dev.predict(X, OUT_PREDICT).reshape(predict.shape), predict,
                               rtol=RTOL, atol=0)


# ------------------------------------------------------------ known answers
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["", "explicit"])
def test_known_answers_gpu(golden, dtype, layout):
    f = load_xgboost_model(os.path.join(golden, KA_FILE))
    dev = _dev(f, layout, dtype)
    assert dev.info()["layout"] == LAYOUT_ID[layout]
    X = KA_X.astype(dtype)
    assert np.array_equal(dev.predict(X, OUT_LEAF), KA_LEAF)
    assert np.array_equal(dev.predict(X, OUT_MARGIN), KA_MARGIN)
    assert np.array_equal(dev.predict(X, OUT_PREDICT), KA_MARGIN)   # reg:squarederror
    dev.close()


# -------------------------------------------------------- synthetic parity
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["", "explicit"])
@pytest.mark.parametrize("name", ["k1", "k3", "k20"])
def test_synthetic_parity(name, layout, dtype):
    forest, X, leaf, margin, predict = _case(name)
    dev = _dev(forest, layout, dtype)
    info = dev.info()
    assert info["layout"] == LAYOUT_ID[layout]
    if info["layout"] == 10:
        # more than one LDS stage, so the prefetch / commit hand-over runs
        assert info["n_stages"] >= 2, info
    _check(dev, X.astype(dtype), leaf, margin, predict)
    dev.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_deep_forest_takes_the_explicit_layout(dtype):
    forest, X, leaf, margin, predict = _case("deep")
    assert int(forest.depths().max()) == 10
    dev = _dev(forest, dtype=dtype)
    assert dev.info()["layout"] == 1
    _check(dev, X.astype(dtype), leaf, margin, predict)
    dev.close()


# ------------------------------------------- layout 10 under LightGBM's rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lgb_rule_on_the_categorical_heap(tmp_path, dtype):
    trees = lf.synthetic_leafwise_trees(60, 8, 12, seed=21)
    lf.add_categorical_splits(trees, [0, 3, 7], n_categories=300, seed=22)
    p = str(tmp_path / "model.txt")
    lf.write_lightgbm_text(p, trees, 12, "multiclass num_class:3", num_class=3)
    f = load_lightgbm_model(p)
    assert int(f.depths().max()) <= 7
    m = lgb_ref.read_lgb_text(p)
    rng = np.random.default_rng(23)
    n = N_ROWS
    X = rng.standard_normal((n, 12))
    for j in (0, 3, 7):
        X[:, j] = rng.integers(-5, 320, size=n) + rng.choice([0, 0.5, 0.999], size=n)
        X[rng.random(n) < 0.05, j] = np.nan
        X[rng.random(n) < 0.01, j] = 3e9
    X = X.astype(dtype)
    plain = _dev(f)
    assert plain.info()["layout"] == 1       # LightGBM forests keep the explicit layout
    plain.close()
    dev = _dev(f, "cheap")
    assert dev.info()["layout"] == 10
    Xd = X.astype(np.float64)
    assert np.array_equal(dev.predict(X, OUT_LEAF), lgb_ref.leaf_index(m, Xd))
    assert np.array_equal(dev.predict(X, OUT_MARGIN), lgb_ref.predict(m, Xd, raw_score=True))
    np.testing.assert_allclose(dev.predict(X, OUT_PREDICT), lgb_ref.predict(m, Xd), rtol=RTOL)
    dev.close()


# ------------------------------------------------------------------ plugin
def _one_split_tree(cats=None, default_left=True):
    """Root on feature 0 (x < 0.5, or the category set), leaves 1.0 / 2.0."""
    t = {"cleft": np.array([1, -1, -1], dtype=np.int32),
         "cright": np.array([2, -1, -1], dtype=np.int32),
         "sindex": np.array([(int(default_left) << 31) | 0, 0, 0], dtype=np.uint32),
         "value": np.array([0.5, 1.0, 2.0], dtype=np.float32),
         "sum_hess": np.array([2.0, 1.0, 1.0], dtype=np.float32)}
    if cats is not None:
        t["cats"] = {0: cats}
    return t


@pytest.mark.parametrize("fmt", ["json", "ubj"])
def test_plugin_serves_categorical_model(tmp_path, fmt):
    from kfserving_amd.xgbserver import XGBoostModel
    write = xf.write_json_model if fmt == "json" else xf.write_ubj_model
    cdir, ndir = tmp_path / "cat", tmp_path / "num"
    cdir.mkdir(), ndir.mkdir()
    # categorical: {0} -> right (2.0), anything else valid -> left (1.0), missing -> left
    write(str(cdir / "model.bst"), [_one_split_tree(cats=[0], default_left=True)], [0], 2, 0, 0.0,
          "reg:squarederror", version=(2, 0, 0))
    # numerical: x < 0.5 -> left (1.0), missing -> right (2.0)
    write(str(ndir / "model.bst"), [_one_split_tree(default_left=False)], [0], 2, 0, 0.0,
          "reg:squarederror", version=(2, 0, 0))
    cat = XGBoostModel("cat", str(cdir), 1)
    num = XGBoostModel("num", str(ndir), 1)
    assert cat.load() and num.load()
    rows = [[0, 1.0], [1, 1.0], [0.0, 0.0], [None, 1.0]]
    # category 0 is reached: under the 0.82 list rule the zeros would be missing (1.0)
    assert cat.predict({"instances": rows})["predictions"] == [2.0, 1.0, 2.0, 1.0]
    # the numerical model keeps that rule: 0 is missing -> default right; 1 >= 0.5 -> right
    assert num.predict({"instances": rows[:3]})["predictions"] == [2.0, 2.0, 2.0]
    assert num.predict({"instances": [[0.25, 1.0]]})["predictions"] == [1.0]
    assert cat.native_v1_transform == 0 and num.native_v1_transform == 1
    assert cat.native_v2_transform == 0 and num.native_v2_transform == 0
    # V2 tensors: NaN is missing for both
    T = np.array([[0.0, 1.0], [1.0, 1.0], [np.nan, 1.0]])
    assert cat.predict_tensor(T).tolist() == [2.0, 1.0, 1.0]
    assert num.predict_tensor(T).tolist() == [1.0, 2.0, 2.0]


# ------------------------------------------------------------- contributions
def test_contributions_unsupported_with_a_message():
    forest, X, _, _, _ = _case("k1")
    assert forest.cover is not None
    dev = _dev(forest)
    with pytest.raises(TreeInferError, match="categorical") as e:
        dev.predict(X[:8], OUT_CONTRIB)
    assert e.value.code == -4          # TI_ERR_UNSUPPORTED
    assert dev.predict(X[:8], OUT_MARGIN).shape == (8,)    # the handle still serves
    dev.close()
