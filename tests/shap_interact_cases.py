"""The forests and rows on which the GPU's SHAP interaction values
(TI_OUTPUT_INTERACT) are compared with tests/shap_interact_eval.py: shared by
tests/test_gpu_shap_interact.py and scripts/shap_interact_error.py, which
measures the scaled error the test's bounds are set from.

Every case is at most 8 rows x 17 trees x 21 leaves, so the Python reference
takes a second or two; it is computed once per case and cached.  Rows are
float64 values that float32 holds exactly, so one reference serves the float32
and the float64 input of a case."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from kfserving_amd import engine
from kfserving_amd.forest import OUT_INTERACT, TI_F32, TI_F64
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from tests import shap_cat_eval as sc
from tests import shap_interact_eval as si


def xgb(n_trees, depth, F, seed, K=0):
    trees, ti = xf.synthetic_complete_trees(n_trees, depth, F, seed=seed, num_class=K)
    obj = "multi:softprob" if K else "binary:logistic"
    return xf.forest_from_raw_trees(trees, ti, F, K, 0.5, obj)


def chain_trees(n_trees, n, seed):
    """LightGBM tree dicts, each a chain over a permutation of features
    0..n-1: every split's left child is a leaf, its right child the next
    split, so the deepest two leaves' paths hold n distinct features."""
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(n_trees):
        left = np.array([~i for i in range(n)], dtype=np.int64)
        right = np.array([i + 1 for i in range(n - 1)] + [~n], dtype=np.int64)
        leaf_count = rng.integers(1, 40, size=n + 1).astype(np.int64)
        internal_count = np.array([leaf_count[i:].sum() for i in range(n)], dtype=np.int64)
        trees.append({"split_feature": rng.permutation(n), "threshold": rng.standard_normal(n) * 0.5 + 0.8,
                      "decision_type": (rng.integers(0, 2, size=n) << 1) | (rng.integers(0, 3, size=n) << 2),
                      "left_child": left, "right_child": right,
                      "leaf_value": rng.uniform(-1, 1, size=n + 1),
                      "leaf_count": leaf_count, "internal_count": internal_count})
    return trees


def hand_tree():
    """One depth-2 tree on two features (LightGBM text, float64):
        x0 <= 0 ? (x1 <= 0 ? 1 : -2) : 4     covers 8 -> (4 -> 2, 2), 4"""
    z = np.zeros(2, dtype=np.int64)
    tree = {"split_feature": np.array([0, 1]), "threshold": np.zeros(2), "decision_type": z,
            "left_child": np.array([1, ~0]), "right_child": np.array([~2, ~1]),
            "leaf_value": np.array([1.0, -2.0, 4.0]), "leaf_count": np.array([2, 2, 4]),
            "internal_count": np.array([8, 4])}
    return sc.forest_of_trees([tree], 2, objective="regression")


def sk_vector_forest():
    from sklearn.ensemble import RandomForestClassifier
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 6)).astype(np.float32)
    y = (X[:, 0] > 0).astype(int) + (X[:, 1] > 0.5).astype(int)
    est = RandomForestClassifier(n_estimators=5, max_leaf_nodes=15, random_state=0).fit(X, y)
    return forest_from_sklearn(est)


def _rows(f, n, seed, n_categories=0):
    X = sc.rows(f, n, seed=seed, n_categories=n_categories)
    return X.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(name):
    """(forest, rows [n, n_cols] float64 holding float32 values)."""
    if name == "xgb-f32":                   # float32 forest, paths of <= 3 elements
        f = xgb(10, 3, 10, seed=1)
        return f, _rows(f, 8, 11)
    if name == "lgb-missing":               # zero / NaN / none missing types, repeated features
        f = sc.lgb_cat_forest(10, 15, 10, seed=3)
        return f, _rows(f, 8, 12)
    if name == "lgb-categorical":
        f = sc.lgb_cat_forest(8, 15, 8, seed=5, cat_features=(0, 3), n_categories=70)
        return f, _rows(f, 8, 13, n_categories=70)
    if name == "sk-vector-averaged":        # vector leaves, average_divisor = n_estimators
        f = sk_vector_forest()
        X = _rows(f, 8, 14)
        X[np.isnan(X)] = 0.25               # sklearn trees: no missing values
        return f, X
    if name == "xgb-k3":                    # three groups, scalar leaves
        f = xgb(9, 3, 8, seed=2, K=3)
        return f, _rows(f, 8, 15)
    if name == "xgb-k17-parts":             # > 16 groups: two group parts
        f = xgb(17, 2, 5, seed=6, K=17)
        return f, _rows(f, 6, 16)
    if name == "chain12":                   # paths of 12 elements: MAXN = 16
        f = sc.forest_of_trees(chain_trees(3, 12, seed=21), 12)
        return f, _rows(f, 6, 17)
    if name == "chain20":                   # 20 elements: MAXN = 32; 21 columns -> 6 + 6 + 6 + 2
        f = sc.forest_of_trees(chain_trees(2, 20, seed=22), 20)
        return f, _rows(f, 4, 18)
    if name == "unused-feature-short-rows":
        # feature 6 of 7 is in no tree; the rows have 5 columns, so features 5
        # and 6 read NaN; 14 splits on 6 features repeat features on paths
        f = sc.forest_of_trees(lf.synthetic_leafwise_trees(6, 15, 6, seed=23), 7)
        return f, _rows(f, 8, 19)[:, :5].copy()
    if name == "geometry":                  # 130 rows: two full waves and a ragged one
        f = sc.lgb_cat_forest(3, 7, 4, seed=24)
        return f, _rows(f, 130, 20)
    raise KeyError(name)


PARITY = ["xgb-f32", "lgb-missing", "lgb-categorical", "sk-vector-averaged", "xgb-k3",
          "xgb-k17-parts", "chain12", "chain20", "unused-feature-short-rows", "geometry"]


@functools.lru_cache(maxsize=None)
def want(name):
    f, X = case(name)
    w = si.interactions(f, X)
    w.setflags(write=False)
    return w


def predict(dev, X, kind=OUT_INTERACT, stride=None):
    """ti_predict on X in its own dtype (DeviceForest.predict would convert it
    to the forest's input type), [rows, width].  `stride` > cols passes the
    rows at that pitch, NaN between them."""
    X = np.ascontiguousarray(X)
    assert X.dtype in (np.float32, np.float64)
    rows, cols = X.shape
    if stride is not None:
        wide = np.full((rows, stride), np.nan, dtype=X.dtype)
        wide[:, :cols] = X
        X = wide
    width = dev.forest.output_width(kind)
    out = np.empty(rows * width, dtype=dev.forest.output_dtype(kind))
    xdt = TI_F32 if X.dtype == np.float32 else TI_F64
    engine._check(dev._lib, dev._lib.ti_predict(dev._handle, ctypes.c_void_p(X.ctypes.data), xdt,
                                                rows, cols, stride or cols, kind,
                                                ctypes.c_void_p(out.ctypes.data), out.size))
    return out.reshape(rows, width)


def matrices(f, out):
    n = f.n_features + 1
    return out.reshape(out.shape[0], f.n_groups, n, n)
