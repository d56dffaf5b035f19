"""CSR rows on the device (ti_predict_csr, treeinfer_sparse.h): the sparse
answer is bit for bit DeviceForest.predict on the densified matrix, its leaf
ids are tests/canon_eval's scalar walk of the same dense rows and its margins
the oracle restatement the forest's family is held to in the dense tests."""
import functools
import os
import tempfile

import numpy as np
import pytest
import scipy.sparse as sp

from kfserving_amd.engine import DeviceForest
from kfserving_amd.forest import OUT_CONTRIB, OUT_LEAF, OUT_MARGIN, OUT_PREDICT, TI_F32, TI_F64
from kfserving_amd.formats import load_tree_arrays
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from oracle import lgb_ref, sk_ref, xgb_ref
from tests import canon_eval

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _xgb(n_trees, depth, F, seed, K=0, base=0.0, objective="binary:logistic", spread=0):
    trees, ti = xf.synthetic_complete_trees(n_trees, depth, F, seed=seed, num_class=K)
    if spread:   # the F split columns become F seeded columns of a matrix `spread` wide
        pool = np.sort(np.random.default_rng(seed).choice(spread, F, replace=False)).astype(np.uint32)
        for t in trees:
            s = t["sindex"][:(1 << depth) - 1]
            s[:] = pool[s & 0x7fffffff] | (s & 0x80000000)
        F = spread
    ref = xgb_ref.from_raw_trees(trees, ti, F, K, base, objective)
    return (xf.forest_from_raw_trees(trees, ti, F, K, base, objective),
            lambda D: xgb_ref.predict(ref, D.astype(np.float32), output_margin=True))


def _lgb(n_trees, leaves, F, seed, cat=()):
    trees = lf.synthetic_leafwise_trees(n_trees, leaves, F, seed=seed)
    if cat:
        lf.add_categorical_splits(trees, list(cat), n_categories=300, seed=seed + 1)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.txt")
        lf.write_lightgbm_text(p, trees, F, "binary sigmoid:1")
        f, m = lf.load_lightgbm_model(p), lgb_ref.read_lgb_text(p)
    return f, lambda D: lgb_ref.predict(m, D.astype(np.float64), raw_score=True)


def _sk_clf():
    from tests.test_oracle import _sk_trees
    path = os.path.join(GOLDEN, "sk_rf_clf_model.npz")
    trees, _ = _sk_trees(path)
    f = load_tree_arrays(path)
    return f, lambda D: sk_ref.predict_proba(trees, D.astype(np.float32), f.n_groups)


# kind -> (forest and oracle, absent, categorical columns)
KINDS = {
    "xgb": (lambda: _xgb(40, 8, 28, 1), "nan", ()),
    "xgb3": (lambda: _xgb(30, 6, 28, 2, 3, 0.5, "multi:softprob"), "nan", ()),
    "lgb_zero": (lambda: _lgb(20, 63, 28, 3), "zero", ()),
    "lgb_cat": (lambda: _lgb(24, 31, 12, 21, cat=(0, 3, 7)), "zero", (0, 3, 7)),
    "sk_clf": (_sk_clf, "zero", ()),
    "lgb_7trees": (lambda: _lgb(7, 7, 40, 9), "zero", ()),   # 7 is no multiple of kExpIlp
    # U against the LDS image at R = 64 of float32 values (256 columns): past it, just under it
    "wide_search": (lambda: _xgb(200, 3, 600, 5, spread=20000), "nan", ()),
    "wide_image": (lambda: _xgb(100, 3, 256, 6, spread=20000), "nan", ()),
}


@functools.lru_cache(maxsize=None)
def _kind(name):
    make, absent, cat = KINDS[name]
    f, oracle = make()
    return f, oracle, absent, cat, DeviceForest(f, [0])


def _csr(f, n, n_cols, density, seed, dtype, absent, cat=(), keep=None):
    """Seeded rows as (CSR, the dense matrix it stands for): N(0,1) float32
    values with stored 0.0, -0.0, NaN and the zero map's edges among them;
    `keep` masks what may be stored."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, n_cols)).astype(np.float32)
    specials = np.array([0.0, -0.0, np.nan, 1e-40, 1e-35, 2e-35], dtype=np.float32)
    pick = rng.random(X.shape) < 0.1
    X[pick] = specials[rng.integers(0, len(specials), int(pick.sum()))]
    for c in cat:
        X[:, c] = rng.integers(-5, 320, size=n) + rng.choice([0, 0.5], size=n)
    X = X.astype(dtype)
    stored = rng.random(X.shape) < density
    if keep is not None:
        stored &= keep
    r, c = np.nonzero(stored)
    D = np.full(X.shape, np.nan if absent == "nan" else 0.0, dtype=dtype)
    D[stored] = X[stored]
    return sp.csr_matrix((X[stored], (r, c)), shape=X.shape), D


def _check(dev, f, oracle, S, D, absent):
    """Both kinds of check for one batch, leaf ids and margins."""
    F = f.n_features
    full = np.full((D.shape[0], max(F, D.shape[1])), np.nan, dtype=D.dtype)   # a column >= n_cols is NaN
    full[:, :D.shape[1]] = D
    leaf = dev.predict(S, OUT_LEAF, absent=absent)
    margin = dev.predict(S, OUT_MARGIN, absent=absent)
    assert np.array_equal(leaf, dev.predict(D, OUT_LEAF))
    assert np.array_equal(margin, dev.predict(D, OUT_MARGIN), equal_nan=True)
    assert np.array_equal(dev.predict(S, OUT_PREDICT, absent=absent), dev.predict(D, OUT_PREDICT),
                          equal_nan=True)
    if D.shape[0]:
        assert np.array_equal(leaf, canon_eval.predict(f, full[:, :F], OUT_LEAF))
        assert np.array_equal(margin, np.asarray(oracle(full[:, :F])).reshape(margin.shape))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("search", [False, True])
@pytest.mark.parametrize("name", ["xgb", "xgb3", "lgb_zero", "lgb_cat", "sk_clf", "lgb_7trees"])
def test_csr_parity(name, search, dtype, monkeypatch):
    f, oracle, absent, cat, dev = _kind(name)
    if search:
        monkeypatch.setenv("TI_DEV_KNOBS", "1")
        monkeypatch.setenv("TI_SPARSE_SEARCH", "1")
    S, D = _csr(f, 300, f.n_features, 0.3, 11, dtype, absent, cat)
    _check(dev, f, oracle, S, D, absent)
    assert dev.info()["sparse_walk"] == ([2, 2] if search else [1, 1])


@pytest.mark.parametrize("name,walk,rows", [("wide_search", 2, 256), ("wide_image", 1, 64)])
def test_csr_regime_follows_the_used_columns(name, walk, rows):
    f, oracle, absent, _, dev = _kind(name)
    S, D = _csr(f, 130, f.n_features, 0.01, 12, np.float32, absent)
    _check(dev, f, oracle, S, D, absent)
    info = dev.info()
    U = len(set(f.feature[f.feature >= 0].tolist()))
    assert info["sparse_cols"] == U and (U > 256) == (walk == 2)
    assert (info["sparse_walk"][0], info["sparse_rows"][0]) == (walk, rows)


def _call(dev, indptr, indices, data, n_cols, absent, kind):
    """ti_predict_csr on raw arrays (what scipy would refuse or repair)."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int32)
    n = len(indptr) - 1
    out = np.empty(n * dev.forest.output_width(kind), dtype=dev.forest.output_dtype(kind))
    rc = dev._lib.ti_predict_csr(dev._handle, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data,
                                 TI_F32 if data.dtype == np.float32 else TI_F64, n, n_cols,
                                 {"zero": 0, "nan": 1}[absent], kind, out.ctypes.data, out.shape[0])
    return rc, out


EDGES = ["rows1", "rows63", "rows65", "rows257", "nnz0", "empty_between", "unread_columns",
         "columns_past_F", "fewer_columns", "indptr_base"]


@pytest.mark.parametrize("absent", ["zero", "nan"])
@pytest.mark.parametrize("search", [False, True])
@pytest.mark.parametrize("edge", EDGES)
def test_csr_edges(edge, search, absent, monkeypatch):
    f, oracle, _, _, dev = _kind("lgb_7trees")   # F = 40, R = 256, zero map, some columns unread
    F = f.n_features
    if search:
        monkeypatch.setenv("TI_DEV_KNOBS", "1")
        monkeypatch.setenv("TI_SPARSE_SEARCH", "1")
    n = int(edge[4:]) if edge.startswith("rows") else 9
    n_cols = F + 10 if edge == "columns_past_F" else F - 5 if edge == "fewer_columns" else F
    keep = np.ones((n, n_cols), dtype=bool)
    if edge == "empty_between":
        keep[1::2] = False                     # rows 1, 3, 5, 7 store nothing
    elif edge == "unread_columns":
        unread = sorted(set(range(F)) - set(f.feature.tolist()))
        assert unread
        keep[4] = False
        keep[4, unread] = True                 # row 4 stores unread columns alone
    S, D = _csr(f, n, n_cols, 0.0 if edge == "nnz0" else 0.4, 13, np.float32, absent, keep=keep)
    if edge != "indptr_base":
        return _check(dev, f, oracle, S, D, absent)
    pad = 5                                    # indptr starts at 5: arrays read from element 5 on
    rc, leaf = _call(dev, S.indptr.astype(np.int64) + pad, np.r_[[0] * pad, S.indices],
                     np.r_[[7.0] * pad, S.data].astype(np.float32), n_cols, absent, OUT_LEAF)
    assert rc == 0 and np.array_equal(leaf.reshape(n, -1), dev.predict(D, OUT_LEAF))
    assert np.array_equal(leaf.reshape(n, -1), canon_eval.predict(f, D, OUT_LEAF))


@pytest.mark.parametrize("case,code", [("unsorted", -1), ("index_range", -1), ("indptr_decreases", -1),
                                       ("contrib", -4), ("linear", -4)])
def test_csr_refusals_leave_the_handle_serving(case, code):
    if case == "linear":
        from tests.test_gpu_lgb_linear import _model
        f = _model(4, 2)[2]
        dev = DeviceForest(f, [0])
    else:
        f, dev = _kind("xgb")[0], _kind("xgb")[4]
    indptr, indices = [0, 2, 3], [1, 5, 2]
    if case == "unsorted":
        indices = [5, 5, 2]
    elif case == "index_range":
        indices = [1, f.n_features, 2]
    elif case == "indptr_decreases":
        indptr = [0, 3, 2]
    rc, _ = _call(dev, indptr, indices, np.ones(3, np.float32), f.n_features, "nan",
                  OUT_CONTRIB if case == "contrib" else OUT_MARGIN)
    assert rc == code and dev._lib.ti_last_error()
    X = np.zeros((3, f.n_features), np.float32)
    got = dev.predict(X, OUT_MARGIN)
    assert got.shape == (3,) and (case == "linear" or
                                  np.array_equal(got, canon_eval.predict(f, X, OUT_MARGIN)))


def test_absent_must_be_named():
    with pytest.raises(ValueError):
        _kind("xgb")[4].predict(sp.csr_matrix((2, 28), dtype=np.float32), OUT_MARGIN, absent="missing")
