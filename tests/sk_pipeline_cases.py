"""Seeded fitted sklearn Pipelines (imputer / scaler steps in front of a small
tree ensemble) shared by tests/test_sk_pipeline_format.py and
tests/test_gpu_sk_pipeline.py, and ``apply_steps``, a numpy restatement of the
pre-step rule of include/treeinfer.h.

The training columns span scales from 1e-3 to 1e6; the last column holds
values around 1e-41 and a single 1.0, so under ``MaxAbsScaler`` (scale 1) and
the cast to float32 it lands in float32's subnormal range.  Every ensemble has
at most 20 trees of depth at most 6."""
import functools

import numpy as np

from kfserving_amd.forest import PRE_ADD, PRE_DIV, PRE_FILL_NAN, PRE_MUL, PRE_SUB

F = 6
SCALES = np.array([1e-3, 1.0, 50.0, 1e3, 1e6, 1e-41])
SHIFTS = np.array([0.0, -3.0, 120.0, 5e3, -2e6, 0.0])
CASES = ("imp-std-rf", "std-minmax-robust-maxabs-et", "std-nomean-dt", "minmax-rfc3", "std-rfc20",
         "imp-std-gb", "std-gb", "passthrough-std-rf", "maxabs-sub-rf")
HAS_IMPUTER = ("imp-std-rf", "imp-std-gb")


def rows(n, seed, nan=False, cols=F):
    """n rows on the training scales (float64); nan: about 4 % of the entries
    and one whole row are NaN, and zeros of both signs appear."""
    rng = np.random.default_rng(seed)
    reps = -(-cols // F)
    X = rng.standard_normal((n, cols)) * np.tile(SCALES, reps)[:cols] + np.tile(SHIFTS, reps)[:cols]
    X[rng.random(X.shape) < 0.03] = 0.0
    X[rng.random(X.shape) < 0.02] = -0.0
    if nan:
        X[rng.random(X.shape) < 0.04] = np.nan
        X[n // 2] = np.nan
    return X


def _train(seed, nan):
    X = rows(500, seed, nan)
    X[7, F - 1] = 1.0                      # MaxAbsScaler's scale of the tiny column
    Z = np.nan_to_num((X - SHIFTS) / SCALES)
    Z[:, F - 1] = np.sign(Z[:, F - 1])
    score = Z[:, 0] - 0.7 * Z[:, 1] + 0.5 * Z[:, 2] * Z[:, 3] + 0.3 * Z[:, 4] + 0.2 * Z[:, F - 1]
    return X, score


@functools.lru_cache(maxsize=None)
def fitted(name):
    from sklearn.ensemble import (ExtraTreesRegressor, GradientBoostingRegressor,
                                  RandomForestClassifier, RandomForestRegressor)
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import MaxAbsScaler, MinMaxScaler, RobustScaler, StandardScaler
    from sklearn.tree import DecisionTreeRegressor
    seed = CASES.index(name) + 11
    X, score = _train(seed, name in HAS_IMPUTER)

    def classes(k):
        edges = np.quantile(score, np.linspace(0, 1, k + 1)[1:-1])
        return np.searchsorted(edges, score) * 3 + 1          # labels 1, 4, 7, ...

    rf = dict(n_estimators=12, max_depth=6, random_state=seed)
    if name == "imp-std-rf":
        steps = [("imp", SimpleImputer(strategy="median")), ("std", StandardScaler()),
                 ("rf", RandomForestRegressor(**rf))]
        y = score
    elif name == "std-minmax-robust-maxabs-et":
        steps = [("std", StandardScaler()), ("mm", MinMaxScaler(feature_range=(-2, 3))),
                 ("rob", RobustScaler()), ("ma", MaxAbsScaler()),
                 ("et", ExtraTreesRegressor(**rf))]
        y = score
    elif name == "std-nomean-dt":
        steps = [("std", StandardScaler(with_mean=False)),
                 ("dt", DecisionTreeRegressor(max_depth=6, random_state=seed))]
        y = score
    elif name == "minmax-rfc3":
        steps = [("mm", MinMaxScaler()), ("rf", RandomForestClassifier(**rf))]
        y = classes(3)
    elif name == "std-rfc20":
        steps = [("std", StandardScaler()),
                 ("rf", RandomForestClassifier(n_estimators=20, max_depth=6, random_state=seed))]
        y = classes(20)
    elif name == "imp-std-gb":
        steps = [("imp", SimpleImputer(strategy="mean")), ("std", StandardScaler()),
                 ("gb", GradientBoostingRegressor(n_estimators=20, max_depth=3, random_state=seed))]
        y = score
    elif name == "std-gb":
        steps = [("std", StandardScaler()),
                 ("gb", GradientBoostingRegressor(n_estimators=20, max_depth=3, random_state=seed))]
        y = score
    elif name == "passthrough-std-rf":
        steps = [("skip", "passthrough"), ("none", None), ("std", StandardScaler()),
                 ("rf", RandomForestRegressor(**rf))]
        y = score
    elif name == "maxabs-sub-rf":
        steps = [("ma", MaxAbsScaler()), ("rf", RandomForestRegressor(**rf))]
        y = score
    else:
        raise KeyError(name)
    return Pipeline(steps).fit(X, y)


@functools.lru_cache(maxsize=None)
def forest(name):
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    return forest_from_sklearn(fitted(name))


def transformed(name, X):
    """sklearn's own transform of the steps in front of the final estimator."""
    return fitted(name)[:-1].transform(X)


def admits_nan(name):
    """Whether Pipeline.predict takes NaN rows (an imputer in the chain, or a
    final estimator that routes NaN itself)."""
    try:
        fitted(name).predict(rows(4, 1, True))
        return True
    except ValueError:
        return False


def batch(name, n, seed):
    """n float64 rows for the case, with NaN where its pipeline admits them."""
    return rows(n, seed, admits_nan(name))


def apply_steps(f, X):
    """The pre-step rule of include/treeinfer.h in numpy: per step a NaN fill
    with the constant cast to X's type, or one float64 operation rounded to
    X's type; then the cast to float32.  X: float32 or float64 [rows, F]."""
    v = np.array(X, copy=True)
    assert v.dtype in (np.float32, np.float64)
    xt = v.dtype
    with np.errstate(all="ignore"):
        for s in range(f.n_pre_steps):
            op, c = int(f.pre_ops[s]), f.pre_consts[s]
            if op == PRE_FILL_NAN:
                v = np.where(np.isnan(v), c.astype(xt), v)
                continue
            w = v.astype(np.float64)
            if op == PRE_SUB:
                w = w - c
            elif op == PRE_DIV:
                w = w / c
            elif op == PRE_MUL:
                w = w * c
            elif op == PRE_ADD:
                w = w + c
            else:
                raise ValueError(op)
            v = w.astype(xt)
        return v.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def wide_forest(n_steps=8, n_features=600, seed=5):
    """A synthetic forest whose constants (n_steps x n_features x 8 bytes)
    exceed the pre-pass's 32 KB LDS budget: a depth-3 tree on 600 columns with
    seeded random ops and constants."""
    import dataclasses
    from sklearn.tree import DecisionTreeRegressor
    from kfserving_amd.forest import TI_F64
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    rng = np.random.default_rng(seed)
    X = rows(80, seed, cols=n_features)
    est = DecisionTreeRegressor(max_depth=3, random_state=0).fit(X.astype(np.float32), X[:, 0])
    ops = np.array([PRE_FILL_NAN, PRE_SUB, PRE_DIV, PRE_MUL, PRE_ADD, PRE_DIV, PRE_SUB, PRE_MUL]
                   [:n_steps], dtype=np.int32)
    consts = rng.standard_normal((n_steps, n_features)) * 3.0
    consts[np.abs(consts) < 0.05] = 0.37
    return dataclasses.replace(forest_from_sklearn(est), pre_ops=ops, pre_consts=consts,
                               input_dtype=TI_F64)
