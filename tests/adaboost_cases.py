"""Shared by the AdaBoost / tree-quantile tests: the numpy restatement of the
rule (include/treeinfer.h), fitted models, and forests of duplicated trees."""
import functools

import numpy as np

from kfserving_amd.formats.sklearn_format import forest_from_tree_arrays, tree_arrays_from_sklearn

F = 6
# trees requested -> (depth, loss); 300 stops early (35 members are kept)
REGRESSORS = {1: (3, "linear"), 2: (1, "linear"), 50: (5, "linear"), 63: (5, "square"),
              64: (5, "square"), 65: (2, "square"), 129: (6, "exponential"), 300: (3, "linear")}


def rows(n, seed=1, dtype=np.float64):
    X = np.random.default_rng(seed).standard_normal((n, F))
    X[::5] = np.round(X[::5], 1)            # coarse rows reach the same leaves: tied predictions
    return X.astype(np.float32).astype(dtype)


def tree_quantile_rule(V, w, q):
    """V [rows, T] per-tree predictions, w [T], q levels -> [rows, len(q)]."""
    R, T = V.shape
    order = np.lexsort((np.broadcast_to(np.arange(T), V.shape), V))       # by (value, tree)
    cdf = np.cumsum(np.asarray(w, dtype=np.float64)[order], axis=1)       # sequential float64
    at = np.arange(R)
    return np.stack([V[at, order[at, (cdf >= qq * cdf[:, -1:]).argmax(axis=1)]] for qq in q], axis=1)


@functools.lru_cache(maxsize=None)
def regressor(n_trees):
    from sklearn.ensemble import AdaBoostRegressor
    from sklearn.tree import DecisionTreeRegressor
    depth, loss = REGRESSORS[n_trees]
    X = rows(400, seed=7)
    y = 2 * X[:, 0] + np.sin(3 * X[:, 1]) + 0.1 * np.random.default_rng(8).standard_normal(400)
    return AdaBoostRegressor(DecisionTreeRegressor(max_depth=depth), n_estimators=n_trees, loss=loss,
                             random_state=0).fit(X, y)


@functools.lru_cache(maxsize=None)
def classifier(n_classes):
    from sklearn.ensemble import AdaBoostClassifier
    from sklearn.tree import DecisionTreeClassifier
    X = rows(400, seed=9)
    y = np.digitize(X[:, 0] + 0.5 * X[:, 2], np.linspace(-0.6, 0.6, n_classes - 1)) * 10 + 3
    return AdaBoostClassifier(DecisionTreeClassifier(max_depth=2), n_estimators=40,
                              random_state=0).fit(X, y)


@functools.lru_cache(maxsize=None)
def random_forest():
    from sklearn.ensemble import RandomForestRegressor
    X = rows(400, seed=7)
    return RandomForestRegressor(n_estimators=20, max_depth=6, random_state=0).fit(X, X[:, 0] * X[:, 1])


def member_predictions(est, X):
    return np.array([m.predict(X.astype(np.float32)) for m in est.estimators_]).T


def copies_forest(n_trees, weights, scale_period=1):
    """The random forest's 20 trees repeated; copy c's values scaled by 1 + c % scale_period."""
    base = [tree_arrays_from_sklearn(m.tree_) for m in random_forest().estimators_]
    arrays = []
    for t in range(n_trees):
        a = dict(base[t % len(base)])
        a["value"] = a["value"] * (1 + (t // len(base)) % scale_period)
        arrays.append(a)
    f = forest_from_tree_arrays(arrays, F, False, average=False, kind="copies")
    f.tree_weight = None if weights is None else np.asarray(weights, dtype=np.float64)
    return f


def forest_predictions(f, X):
    """[rows, T] leaf values of a forest whose leaf ids are node indexes."""
    from tests import canon_eval
    ids = canon_eval.predict(f, X.astype(np.float32), 2)         # OUT_LEAF
    return f.leaf_value[f.tree_offset[:-1][None, :] + ids, 0]
