"""The categorical records (layout 11) against oracle/lgb_ref (LightGBM) and
tests/canon_eval (XGBoost's rule, the fallbacks): leaf ids and margins bit for
bit, predictions at RTOL.  The generators split a categorical feature
numerically too, which layout 11 refuses: _unmix moves those splits one up."""
import dataclasses
import json

import numpy as np
import pytest

from kfserving_amd.forest import (NODE_CAT_XGB, NODE_CATEGORICAL, OUT_LEAF, OUT_MARGIN, OUT_PREDICT)
from kfserving_amd.formats import load_lightgbm_model
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from oracle import lgb_ref
from tests import canon_eval
from tests.test_gpu_xgb_categorical import _deep_trees, _dev

pytestmark = pytest.mark.gpu

RTOL = 1e-5
KINDS = (OUT_LEAF, OUT_MARGIN, OUT_PREDICT)
CATS = (0, 3, 7)
N_ROWS = 1537   # 256-row tiles: two of them without a NaN, and a last one of one row
LGB_MISSING = {"lgb": None, "lgb_zero": (lf.MISSING_ZERO,), "lgb_nan": (lf.MISSING_NONE, lf.MISSING_NAN)}


def _unmix(trees):
    for t in trees:
        f = np.asarray(t["split_feature"]).copy()
        num = (np.asarray(t["decision_type"]) & 1) == 0
        f[num & np.isin(f, CATS)] += 1
        t["split_feature"] = f
    return trees


def _lgb(tmp, name, trees, num_class=3):
    p = str(tmp / (name + ".txt"))
    lf.write_lightgbm_text(p, trees, 12, "multiclass num_class:%d" % num_class if num_class > 1
                           else "regression", num_class=num_class)
    return load_lightgbm_model(p), lgb_ref.read_lgb_text(p)


def _limits(forest):
    cat = (forest.feature >= 0) & ((forest.flags & NODE_CATEGORICAL) != 0)
    return {j: 32 * int(forest.cat_nwords[cat & (forest.feature == j)].max()) for j in CATS}


def _edges(forest, j):
    """Column j's last member, the codes around its limit L_f, the non-member values."""
    L = _limits(forest)[j]
    last = 0
    for g in np.nonzero((forest.feature == j) & ((forest.flags & NODE_CATEGORICAL) != 0))[0]:
        bits = forest.cat_bits[forest.cat_offset[g]:forest.cat_offset[g] + forest.cat_nwords[g]]
        w = int(np.nonzero(bits)[0][-1])
        last = max(last, 32 * w + int(bits[w]).bit_length() - 1)
    return [float(last), L - 1.0, float(L), L + 1.0, -0.0, -0.5, -1.0, 1e-36, 2.0 ** 24, 2.0 ** 31, 3e9,
            np.inf, -np.inf, np.nan, 5.999, last + 0.999]


def _rows(forest, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N_ROWS, 12))
    X[rng.random(X.shape) < 0.02] = np.nan
    for j in CATS:
        X[:, j] = rng.integers(-5, max(_limits(forest).values()) + 20, size=N_ROWS) + rng.choice([0, 0.5, 0.999], size=N_ROWS)
    X[512:1024] = np.nan_to_num(X[512:1024], nan=0.25)       # two tiles that take the fast step
    where = {}
    for j in CATS:
        for i, v in enumerate(_edges(forest, j)):
            r = np.concatenate([rng.choice(512, 4, replace=False), 512 + rng.choice(512, 4, replace=False)])
            r = r[:4] if np.isnan(v) else r   # NaN stays out of the two fast tiles
            X[r, j] = v
            where[j, i] = r
    X = X.astype(np.float32)
    assert not np.isnan(X[512:1024]).any() and np.isnan(X[:512]).any()
    return X, where


_MODELS = {}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """name -> (forest, X float32, want(X, kinds): the reference, rows of each edge)."""
    def get(name):
        if name in _MODELS:
            return _MODELS[name]
        if name == "xgb":
            trees = _deep_trees()
            for t in trees:
                s = t["sindex"]
                num = np.array([t["cleft"][n] >= 0 and n not in t["cats"] for n in range(len(s))])
                s[num & np.isin(s & 0x7FFFFFFF, CATS)] += 1
            doc = xf.json_model_doc(trees, np.zeros(12, dtype=np.int32), 12, 0, 0.5, "binary:logistic",
                                    version=(2, 0, 0))
            forest = xf.parse_xgboost_bytes(json.dumps(doc).encode())
            want = lambda X, kinds=KINDS: [canon_eval.predict(forest, X, k) for k in kinds]
        else:
            kw = {} if LGB_MISSING[name] is None else {"missing_types": LGB_MISSING[name]}
            trees = _unmix(lf.add_categorical_splits(lf.synthetic_leafwise_trees(60, 31, 12, seed=21, **kw),
                                                     list(CATS), n_categories=300, seed=22))
            forest, m = _lgb(tmp_path_factory.mktemp(name), name, trees)
            ref = {OUT_LEAF: lambda Xd: lgb_ref.leaf_index(m, Xd), OUT_PREDICT: lambda Xd: lgb_ref.predict(m, Xd),
                   OUT_MARGIN: lambda Xd: lgb_ref.predict(m, Xd, raw_score=True)}
            want = lambda X, kinds=KINDS: [ref[k](X.astype(np.float64)) for k in kinds]
        X, where = _rows(forest, seed=len(name))
        _MODELS[name] = (forest, X, want, where)
        return _MODELS[name]
    return get


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["lgb", "lgb_zero", "lgb_nan", "xgb"])
def test_parity_and_layout(model, name, dtype):
    """The default of the deep LightGBM forests, forced for XGBoost's rule."""
    forest, X, want, _ = model(name)
    dev = _dev(forest, "crecord" if name == "xgb" else "", dtype)
    info = dev.info()
    assert info["layout"] == 11, info
    assert name == "xgb" or info["n_stages"] >= 2, info
    leaf, margin, predict = want(X)
    X = X.astype(dtype)
    assert np.array_equal(dev.predict(X, OUT_LEAF), leaf)
    assert np.array_equal(dev.predict(X, OUT_MARGIN).reshape(margin.shape), margin)
    np.testing.assert_allclose(dev.predict(X, OUT_PREDICT).reshape(predict.shape), predict, rtol=RTOL, atol=0)
    dev.close()


@pytest.mark.parametrize("name", ["lgb", "xgb"])
def test_edge_values_are_decided(model, name):
    """The reference alone, no device code.  A proxy for "inverting the edge's
    decision changes a leaf": a node's decision cannot be inverted through the
    reference, so another value in the edge's place (one no bitset covers, or a
    low category) must change a leaf of a row that carries it."""
    forest, X, want, where = model(name)
    leaf = want(X, (OUT_LEAF,))[0]
    for (j, i), rows in where.items():
        changed = False
        for other in (float(_limits(forest)[j]), 1.0, 2.0, 6.0, 9.0, 12.0, 17.0):
            Y = X[rows].copy()
            Y[:, j] = other
            changed = changed or not np.array_equal(want(Y, (OUT_LEAF,))[0], leaf[rows])
        assert changed, (name, j, _edges(forest, j)[i])


@pytest.mark.parametrize("name", ["lgb", "xgb"])
def test_same_bits_as_the_explicit_kernel(model, name):
    forest, X, _, _ = model(name)
    a, b = _dev(forest, "crecord"), _dev(forest, "explicit")
    assert (a.info()["layout"], b.info()["layout"]) == (11, 1)
    for kind in (OUT_LEAF, OUT_MARGIN):
        assert np.array_equal(a.predict(X, kind), b.predict(X, kind))
    a.close(), b.close()


@pytest.mark.parametrize("why", ["category 65534", "mixed rules", "split both ways", "block over a stage"])
def test_fallbacks_to_the_explicit_kernel(model, tmp_path, why):
    """What layout 11 refuses stays on layout 1, forced or not, and right."""
    if why == "mixed rules":
        forest = model("xgb")[0]
        cat = np.nonzero((forest.flags & NODE_CATEGORICAL) != 0)[0]
        flags = forest.flags.copy()
        flags[cat[::2]] &= ~np.uint8(NODE_CAT_XGB)
        forest = dataclasses.replace(forest, flags=flags)
    else:
        n_cat, leaves = {"category 65534": (65535, 31), "split both ways": (300, 31),
                         "block over a stage": (2000, 255)}[why]
        trees = lf.synthetic_leafwise_trees(4, leaves, 12, seed=5)
        if why == "category 65534":   # one categorical root a tree, its set at the bitset's edges
            lf.add_categorical_splits(trees, list(CATS), n_cat, seed=6, frac=0.0, root_trees=4)
        else:
            lf.add_categorical_splits(trees, list(CATS), n_cat, seed=6)
        forest = _lgb(tmp_path, "fallback", trees if why == "split both ways" else _unmix(trees), 1)[0]
    rng = np.random.default_rng(9)
    X = rng.standard_normal((300, 12))
    for j in CATS:
        X[:, j] = rng.choice([3.0, 65534.0, 65535.5, 1999.0, -0.5, np.nan, 40.999], size=300)
    for layout in ("", "crecord"):
        dev = _dev(forest, layout)
        assert dev.info()["layout"] == 1, (why, layout)
        for kind in (OUT_LEAF, OUT_MARGIN):
            assert np.array_equal(dev.predict(X, kind), canon_eval.predict(forest, X, kind)), (why, layout)
        dev.close()
