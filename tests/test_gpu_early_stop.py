"""Prediction early stopping (TI_OUTPUT_EARLY_STOP, ABI 15;
kfserving_amd/csrc/treeinfer_estop.h) against a plain restatement of the rule in
include/treeinfer.h over the leaves tests/canon_eval.py reaches: bit equality of
the margins, 1e-5 on transformed outputs.  25 iterations a forest: R = 10 has two
tests and an unchecked tail, R = 1 seven launches with survivor lists between them."""
import dataclasses
import functools
import os
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import OUT_EARLY_STOP, OUT_MARGIN, TI_F32
from kfserving_amd.formats import lightgbm_format as lf, load_lightgbm_model, xgboost_format as xf
from tests import canon_eval, sk_pipeline_cases

pytestmark = pytest.mark.gpu

ITER, F, ROWS = 25, 9, 1025
RTOL, UNSUPPORTED = 1e-5, -4        # tests/test_gpu_parity.py: transformed outputs; TI_ERR_UNSUPPORTED


def _lgb(K=1, leaves=15, cat=False, linear=False, halves=False, scale=8.0):
    trees = lf.synthetic_leafwise_trees(ITER * K, leaves, F, seed=50 + K + leaves)
    rng = np.random.default_rng(leaves)
    for t in trees:   # leaf values wide enough for rows to part; `halves`: multiples of 0.5
        v = np.asarray(t["leaf_value"]) * scale
        t["leaf_value"] = np.round(v * 2.5) * 0.5 + rng.integers(-1, 2, v.shape) * 0.5 if halves else v
    if cat:
        trees = lf.add_categorical_splits(trees, [1, 4], 40, seed=5, edge_frac=0.2, root_trees=3)
    if linear:
        trees = lf.add_linear_leaves(trees, F, seed=6)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.txt")
        lf.write_lightgbm_text(p, trees, F, "binary sigmoid:1" if K == 1 else "multiclass num_class:%d" % K,
                               num_class=K)
        return load_lightgbm_model(p)


def _xgb_082():
    trees, ti = xf.synthetic_complete_trees(ITER, 3, F, seed=77)
    return dataclasses.replace(xf.forest_from_raw_trees(trees, ti, F, 0, 0.3, "binary:logistic"), base_first=False)


FORESTS = {
    "lgb-k1": _lgb,
    "lgb-k3": lambda: _lgb(K=3),
    "lgb-cat": lambda: _lgb(cat=True),
    "lgb-deep": lambda: _lgb(leaves=127),        # deeper than 8
    "xgb-082": _xgb_082,                         # XGBoost rule, float32 sums, base added last
    "halves-k1": lambda: _lgb(halves=True),      # sums that meet a threshold exactly
    "halves-k3": lambda: _lgb(K=3, halves=True),
}


def reference(f, X, R, m):
    """([rows, K] margins, the test a row stopped at or -1, [rows, tests] the unstopped chain's statistics)."""
    lv = canon_eval.leaves(f, X)
    acc_t = np.float32 if f.accum_dtype == TI_F32 else np.float64
    rows, K = lv.shape[0], f.n_groups
    acc = np.zeros((rows, K), dtype=acc_t)
    free = np.zeros((rows, K), dtype=acc_t)     # the chain without stopping: the statistics
    if f.base_first:
        acc += f.base_margin.astype(acc_t)
        free += f.base_margin.astype(acc_t)
    live, stop_at, stats = np.ones(rows, dtype=bool), np.full(rows, -1), []

    def stat(a):
        top = np.sort(a.astype(np.float64), axis=1)
        return 2.0 * np.abs(top[:, 0]) if K == 1 else top[:, -1] - top[:, -2]
    for t in range(f.n_trees):
        v = f.leaf_value[f.tree_offset[t] + lv[:, t]].astype(acc_t)
        cols = slice(None) if f.leaf_width > 1 else slice(f.tree_group[t], f.tree_group[t] + 1)
        free[:, cols] = free[:, cols] + v
        acc[:, cols] = np.where(live[:, None], acc[:, cols] + v, acc[:, cols])
        if (t + 1) % R == 0:
            stats.append(stat(free))
            hit = live & (stat(acc) > m)
            stop_at[hit] = len(stats) - 1
            live &= ~hit
    out = acc if f.base_first else f.base_margin.astype(acc_t) + acc
    if f.average_divisor != 1.0:
        out = out / acc_t(f.average_divisor)
    return out, stop_at, np.stack(stats, axis=1)


@functools.lru_cache(maxsize=None)
def _case(name):
    f = FORESTS[name]()
    rng = np.random.default_rng(12)
    X = rng.standard_normal((ROWS, F))
    X[:, [1, 4]] = rng.integers(-2, 44, (ROWS, 2))     # categories, some outside every bitset
    X[rng.random(X.shape) < 0.05] = np.nan
    X[rng.random(X.shape) < 0.05] = 1e-36              # LightGBM reads these as 0
    X.setflags(write=False)
    return f, DeviceForest(f, [0]), X


@functools.lru_cache(maxsize=None)
def _want(name, xdt, R, m):
    f, _, X = _case(name)
    return reference(f, X.astype(xdt), R, m)


def _threshold(name, xdt, R):
    """From the reference's own statistics: three rows in ten never exceed it."""
    f, _, X = _case(name)
    return float(np.quantile(reference(f, X.astype(xdt), R, np.inf)[2].max(axis=1), 0.3))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("iters", [10, 1])
@pytest.mark.parametrize("name", ["lgb-k1", "lgb-k3", "lgb-cat", "lgb-deep", "xgb-082"])
def test_margins_match_the_rule(name, iters):
    f, dev, X = _case(name)
    R = iters * f.n_groups
    for xdt in [np.float32] + [np.float64] * (f.input_dtype != 0):   # prepare_input casts an XGBoost forest's rows
        m = _threshold(name, xdt, R)
        want, stop_at, _ = _want(name, xdt, R, m)
        # the reference alone: somebody stops at each of the two tests, or at 20 of the 25; somebody never
        assert (stop_at == -1).any()
        assert len(set(stop_at[stop_at >= 0])) >= (2 if iters == 10 else 20)
        dev.set_early_stop(R, m)
        for rows in (1, 63, 65, 257, ROWS):
            got = dev.predict(X[:rows].astype(xdt), OUT_EARLY_STOP).reshape(rows, -1)
            assert np.array_equal(_bits(got), _bits(want[:rows].astype(got.dtype))), (xdt, rows)
        assert np.array_equal(_bits(dev.predict(X.astype(xdt), OUT_EARLY_STOP).reshape(ROWS, -1)), _bits(got))
    assert dev.info()["early_stop_walk"] == 1


@pytest.mark.parametrize("name", ["halves-k1", "halves-k3"])
def test_a_sum_that_meets_the_threshold_goes_on(name):
    """m is a statistic rows have exactly at the first test (K = 3: 0, a tie): they must not stop there."""
    f, dev, X = _case(name)
    R = f.n_groups
    first = _want(name, np.float64, R, np.inf)[2][:, 0]
    m = 0.0 if f.n_groups > 1 else float(np.median(first))
    want, stop_at, stats = _want(name, np.float64, R, m)
    met = stats[:, 0] == m
    assert met.any() and (stop_at[met] != 0).all() and (stop_at == 0).any()
    dev.set_early_stop(R, m)
    got = dev.predict(X, OUT_EARLY_STOP).reshape(ROWS, -1)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", ["lgb-k3", "xgb-082"])
def test_limits_and_transformed(name):
    f, dev, X = _case(name)
    T, K = f.n_trees, f.n_groups
    plain = dev.predict(X, OUT_MARGIN)
    for R, m in ((K, np.inf), (T, 0.1), (T + 7, -1.0)):     # no test passes, or none is followed by a tree
        dev.set_early_stop(R, m)
        assert np.array_equal(_bits(dev.predict(X, OUT_EARLY_STOP)), _bits(plain)), (R, m)
    xdt = np.float32 if f.input_dtype == 0 else np.float64
    want, stop_at, _ = _want(name, xdt, 10 * K, -1.0)
    assert (stop_at == 0).all()                            # m = -1: every row stops at the first test
    dev.set_early_stop(10 * K, -1.0)
    got = dev.predict(X, OUT_EARLY_STOP).reshape(ROWS, -1)
    assert np.array_equal(_bits(got), _bits(want))
    m = _threshold(name, xdt, 10 * K)
    dev.set_early_stop(10 * K, m, transformed=True)
    assert dev.early_stop == (10 * K, m, True)
    got = dev.predict(X, OUT_EARLY_STOP).reshape(ROWS, -1)
    want_p = canon_eval.transform(f, _want(name, xdt, 10 * K, m)[0]).reshape(ROWS, -1)
    np.testing.assert_allclose(got, want_p, rtol=RTOL, atol=0)


@pytest.mark.parametrize("case", ["linear", "csr", "pre-steps"])
def test_refusals_leave_the_handle_serving(case):
    f = {"linear": lambda: _lgb(linear=True), "csr": _lgb,
         "pre-steps": lambda: sk_pipeline_cases.forest("imp-std-gb")}[case]()
    dev = DeviceForest(f, [0])
    X = np.random.default_rng(2).standard_normal((65, f.n_features))
    dev.set_early_stop(2, 0.5)
    for bad in ((0, 1.0), (3, float("nan"))):                 # TI_ERR_INVALID, the state kept
        with pytest.raises(TreeInferError):
            dev.set_early_stop(*bad)
    assert dev.early_stop == (2, 0.5, False)
    with pytest.raises(TreeInferError) as e:
        dev.predict(sp.csr_matrix(X) if case == "csr" else X, OUT_EARLY_STOP)
    assert e.value.code == UNSUPPORTED
    assert np.isfinite(dev.predict(X, OUT_MARGIN)).all()      # the handle serves on
    dev.close()
