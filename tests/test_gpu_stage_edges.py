"""The edges of the staged walks, deterministically: every kernel that copies
tree stages into LDS -- layouts 7, 8 and 9 on the record bottom, layout 9 on
the u8 bottom and on the u16 bottom one and two lanes a row, the binned heap's
indexed walk, the float heap and the categorical heap -- at the tree counts
where its stage pipeline and its group of trees a lane change shape:

* 1 tree; ``tree_ilp - 1`` and ``tree_ilp + 1`` for every tree_ilp the walks
  take (4, 7, 8, 16: the counts 3 .. 9, 15 and 17 hold them all, and the test
  asserts that info()["tree_ilp"] is one of those);
* for the walks whose stages are runs of whole trees (stage_start), the
  smallest count of 1, 2, 4, 8 ... at which info()["n_stages"] reaches 2, and
  that count plus one;
* for the walks whose stages are S records, S - 1, S and S + 1: layout 8 takes
  S from TI_HX_STAGE (5, with 4 trees a lane: counts 4, 5, 6; and its default
  8: counts 7, 8, 9).  The heaps read TI_BHEAP_STAGE / TI_HEAP_LDS_KB once a
  process, so here they keep the host's rule for forests this small -- S is
  the largest multiple of the trees a lane walks (4 binned, 8 float) within
  the forest, and the forest itself below that -- which puts S - 1, S, S + 1
  at 3, 4, 5 and 7, 8, 9.  info() reports a stage count for the categorical
  heap only (it is asserted, and the float heap sizes its stages by the same
  host function); for layouts 0 and 3 it reports none, so a change of the
  host's rule for them would not show here.

With K = 3 a LightGBM forest holds K trees an iteration, so its counts are 3,
6, 9 and 15: tree_ilp - 1 for 4, 7 and 16 and tree_ilp + 1 for 8; the other
edges (5, 8, 17) are reached at K = 1 only.

Rows: 1, 257 and 513 (a 256- or 512-row tile plus one row).  One batch holds
NaN, +-0 and values inside LightGBM's 1e-35 zero map, one holds none, so both
the slow and the fast step of every walk run.  K = 1 and K = 3.  Margins are
bit for bit those of the C restatement of LightGBM's loop (oracle.port) or of
XGBoost's (oracle.xgb_ref); leaf ids are the canonical evaluator's
(tests/canon_eval.py).  Forests are small: 31 leaves or depth 5, 12 features."""
import os
import tempfile

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest
from kfserving_amd.forest import OUT_LEAF, OUT_MARGIN
from kfserving_amd.formats import load_lightgbm_model
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from oracle import port, xgb_ref
from tests import canon_eval

pytestmark = pytest.mark.gpu

F = 12
ROWS = (1, 257, 513)
COUNTS = (1, 3, 4, 5, 6, 7, 8, 9, 15, 17)
ILPS = {4, 7, 8, 16}
CAT_FEATURES = (0, 3, 7)
SPECIALS = np.array([np.nan, 0.0, -0.0, 1e-36, -1e-40])

# name -> (model family, developer knobs, (layout, bottom) the forest must land on);
# TI_RX_B8=0 keeps u16 bins for forests whose few thresholds would fit u8, and
# layout 9 is named so that a forest of depth <= 8 does not take a heap layout
L9 = {"TI_FORCE_LAYOUT": "texplicit"}
LGB_WALKS = {
    "staged-records": ("leafwise", {"TI_FORCE_LAYOUT": "lexplicit"}, (7, 0)),
    "heap-top-records": ("leafwise", {"TI_FORCE_LAYOUT": "hexplicit"}, (8, 0)),
    "heap-top-records-s5": ("leafwise", {"TI_FORCE_LAYOUT": "hexplicit", "TI_HX_ILP": "4",
                                         "TI_HX_STAGE": "5"}, (8, 0)),
    "top-staged-records-u16": ("leafwise", {**L9, "TI_RX_B8": "0", "TI_TX16": "0"}, (9, 0)),
    "top-staged-records-u8": ("maxbin", {**L9, "TI_TX8": "0"}, (9, 0)),
    "bottom-u8": ("maxbin", L9, (9, 1)),
    "bottom-u16": ("leafwise", {**L9, "TI_RX_B8": "0", "TI_TX16_SPLIT": "0"}, (9, 2)),
    "bottom-u16-two-lanes": ("leafwise", {**L9, "TI_RX_B8": "0"}, (9, 3)),
}
XGB_WALKS = {
    "binned-heap": ("complete", {"TI_BHEAP_FIX": "0"}, (3, 0)),
    "float-heap": ("complete", {"TI_FORCE_LAYOUT": "heap"}, (0, 0)),
    "categorical-heap": ("categorical", {}, (10, 0)),
}

_BATCHES = {}
_MODELS = {}


def _batch(special, n):
    """The first n rows of one fixed batch with specials and one without; the
    categorical columns hold category codes in both."""
    if special not in _BATCHES:
        rng = np.random.default_rng([71, int(special)])
        X = rng.standard_normal((max(ROWS), F))
        for j in CAT_FEATURES:
            X[:, j] = rng.integers(0, 80, size=X.shape[0])
        if special:
            m = rng.random(X.shape) < 0.1
            X[m] = SPECIALS[rng.integers(0, len(SPECIALS), m.sum())]
        _BATCHES[special] = X
    return _BATCHES[special][:n]


def _model(family, count, K):
    """(forest, reference margins and leaves per (special, n, dtype)) of the
    family's model of `count` trees; built and walked by the oracle once."""
    key = (family, count, K)
    if key in _MODELS:
        return _MODELS[key]
    if family in ("leafwise", "maxbin"):
        mts = (lf.MISSING_NONE, lf.MISSING_ZERO, lf.MISSING_NAN)
        if family == "leafwise":   # i.i.d. thresholds: u16 bins
            trees = lf.synthetic_leafwise_trees(count, 31, F, seed=1000 + count, missing_types=mts)
        else:                      # bin-bound thresholds: u8 bins (125 with the zero rule)
            trees = lf.synthetic_maxbin_trees(count, 31, F, seed=1000 + count, max_bin=125,
                                              missing_types=mts)
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "model.txt")
            lf.write_lightgbm_text(p, trees, F, "binary sigmoid:1" if K == 1 else
                                   f"multiclass num_class:{K}", num_class=K)
            forest = load_lightgbm_model(p)
        dtypes = (np.float64, np.float32)

        def margin(X):
            return port.lgb_predict_raw(trees, K, F, X.astype(np.float64))
    else:
        trees, ti = xf.synthetic_complete_trees(count, 5, F, seed=2000 + count,
                                                num_class=0 if K == 1 else K)
        if family == "categorical":
            xf.add_categorical_splits(trees, list(CAT_FEATURES), 70, seed=3000 + count, root_trees=2)
        objective = "binary:logistic" if K == 1 else "multi:softprob"
        forest = xf.forest_from_raw_trees(trees, ti, F, 0 if K == 1 else K, 0.5, objective)
        ref = xgb_ref.from_raw_trees(trees, ti, F, 0 if K == 1 else K, 0.5, objective)
        dtypes = (np.float32,)

        def margin(X):
            return xgb_ref.predict(ref, X, output_margin=True)
    want = {}
    for special in (True, False):
        for n in ROWS:
            for dt in dtypes:
                X = _batch(special, n).astype(dt)
                want[special, n, dt] = (X, np.asarray(margin(X)).reshape(n, -1),
                                        canon_eval.predict(forest, X, OUT_LEAF))
    _MODELS[key] = (forest, want)
    return _MODELS[key]


def _check(name, family, env, where, count, K, monkeypatch):
    """The walk's forest of `count` trees on the device: where it landed, and
    its margins and leaf ids on every batch.  Returns its info()."""
    forest, want = _model(family, count, K)
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        dev = DeviceForest(forest, [0])
        try:
            info = dev.info()
            if count >= 2 or where[0] not in (7, 9):   # (stage_start's planners leave a single tree to layout 6)
                assert (info["layout"], info["bottom"]) == where, (name, count, K, info)
            for (special, n, dt), (X, margin, leaf) in want.items():
                got = dev.predict(X, OUT_MARGIN).reshape(n, -1)
                assert np.array_equal(got, margin), (name, count, K, special, n, dt, info)
                assert np.array_equal(dev.predict(X, OUT_LEAF), leaf), (name, count, K, special, n, dt, info)
        finally:
            dev.close()
    return info


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", sorted(LGB_WALKS))
def test_record_walks_at_stage_and_group_edges(name, K, monkeypatch):
    family, env, where = LGB_WALKS[name]
    counts = [c for c in COUNTS if c % K == 0]   # LightGBM: K trees an iteration
    for count in counts:
        info = _check(name, family, env, where, count, K, monkeypatch)
        if count >= 2:
            assert info["tree_ilp"] in ILPS, info
    if where[0] == 8:
        return   # stages of S tops: the counts above straddle S (TI_HX_STAGE, or 8)
    count = K
    while _check(name, family, env, where, count, K, monkeypatch)["n_stages"] < 2:
        count *= 2
        assert count <= 1024 * K, "no forest of this family takes two stages"
    info = _check(name, family, env, where, count + K, K, monkeypatch)
    assert info["n_stages"] >= 2, info


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("name", sorted(XGB_WALKS))
def test_heap_walks_at_stage_edges(name, K, monkeypatch):
    family, env, where = XGB_WALKS[name]
    for count in COUNTS:
        info = _check(name, family, env, where, count, K, monkeypatch)
        if where[0] == 10 and count in (7, 8, 9):   # the float heap's rule: S = 8 here
            assert info["n_stages"] == (2 if count == 9 else 1), info
