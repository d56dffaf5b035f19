"""Randomised parity of the categorical kernels: the LDS-staged categorical
heap (layout 10) and the float explicit kernel (layout 1) on the seeded
forests of tests/cat_fuzz_cases.py -- depth 1 to 8, 1 to 123 trees, 1 to 17
groups, 1 to 200 features (both sides of the widest LDS feature image),
bitsets of 1 to 282 words, category sets at the bitset edges, categorical
roots, rows that carry the edge values (the last member, the first value past
the words, -0.0, denormals, +-inf, 2^24, 2^31, 2^32, NaN) with NaN-free and
NaN-holding tiles side by side, row counts around every tile height.

XGBoost forests against the vectorised oracle/xgb_ref.py (which
tests/test_cat_oracle.py pins to the scalar ``walk_doc`` and the hand-computed
answers): leaves equal, margins bit for bit (float32 sums in tree order),
transformed outputs at RTOL.  LightGBM forests against oracle/lgb_ref.py.
"""
import dataclasses

import numpy as np
import pytest

from kfserving_amd.forest import (NODE_CAT_XGB, NODE_CATEGORICAL, NODE_ZERO_FLIP, OUT_LEAF,
                                  OUT_MARGIN, OUT_PREDICT)
from tests import canon_eval
from tests import cat_fuzz_cases as cases
from tests.test_gpu_xgb_categorical import RTOL, _dev

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
SUBSET_SEED, SUBSET_CUT = 4, 13          # 72 trees in several stages, cut inside a lane's eight
MIXED_SEED = 6


def _check(dev, want, dtype, ctx):
    for X, leaf, margin, pred, _ in want:
        Xd = X.astype(dtype)
        at = ctx + (X.shape[0],)
        assert np.array_equal(dev.predict(Xd, OUT_LEAF), leaf), at
        got = dev.predict(Xd, OUT_MARGIN)
        assert np.array_equal(got.reshape(margin.shape), margin), at
        np.testing.assert_allclose(dev.predict(Xd, OUT_PREDICT).reshape(pred.shape), pred,
                                   rtol=RTOL, atol=0, err_msg=str(at))


def _layout(forest, layout=""):
    dev = _dev(forest, layout)
    info = dev.info()
    dev.close()
    return info


@pytest.mark.parametrize("seed", cases.XGB_SEEDS)
def test_fuzz_xgboost_categorical(seed):
    """The default layout, the explicit kernel, and the categorical heap
    forced where the default refused the forest; float32 and float64 rows;
    leaves, margins and predictions."""
    c = cases.xgb_case(seed)
    want = c.want()
    layouts = ["", "explicit"]
    if _layout(c.forest)["layout"] != 10:
        layouts.append("cheap")
    for layout in layouts:
        for dtype in DTYPES:
            dev = _dev(c.forest, layout, dtype)
            try:
                info = dev.info()
                assert layout != "explicit" or info["layout"] == 1
                _check(dev, want, dtype, (c.desc, layout, dtype.__name__, info["layout"]))
            finally:
                dev.close()


@pytest.mark.parametrize("seed", cases.LGB_SEEDS)
def test_fuzz_lightgbm_categorical(seed):
    """LightGBM's rule on its default layout (1) and on the forced
    categorical heap, float64 and float32 rows, against oracle/lgb_ref."""
    c = cases.lgb_case(seed)
    want = c.want()
    for layout in ("", "cheap"):
        for dtype in (np.float64, np.float32):
            dev = _dev(c.forest, layout)
            try:
                info = dev.info()
                assert layout != "" or info["layout"] == 1
                for X, leaf, raw, pred, _ in want:
                    Xd = X.astype(dtype)
                    at = (c.desc, layout, dtype.__name__, info["layout"], X.shape[0])
                    assert np.array_equal(dev.predict(Xd, OUT_LEAF), leaf), at
                    assert np.array_equal(dev.predict(Xd, OUT_MARGIN), raw), at
                    np.testing.assert_allclose(dev.predict(Xd, OUT_PREDICT), pred, rtol=RTOL,
                                               err_msg=str(at))
            finally:
                dev.close()


def test_mixed_rules_stay_on_the_explicit_layout():
    """A forest whose categorical nodes use both rules is served by layout 1,
    forced or not, as the canonical evaluator walks it."""
    c = cases.xgb_case(MIXED_SEED)
    assert _layout(c.forest)["layout"] == 10          # all XGBoost's rule: the heap takes it
    flags = c.forest.flags.copy()
    cat = np.nonzero((c.forest.feature >= 0) & ((flags & NODE_CATEGORICAL) != 0))[0]
    flags[cat[::2]] &= np.uint8(~NODE_CAT_XGB & 0xFF)  # every other one: LightGBM's rule
    mixed = dataclasses.replace(c.forest, flags=flags)
    assert np.any(flags[cat] & NODE_CAT_XGB) and not np.all(flags[cat] & NODE_CAT_XGB)
    for layout in ("", "cheap"):
        for dtype in DTYPES:
            dev = _dev(mixed, layout, dtype)
            try:
                assert dev.info()["layout"] == 1
                for X in (c.rows[9], c.rows[-1]):
                    Xd = X.astype(dtype)
                    assert np.array_equal(dev.predict(Xd, OUT_LEAF),
                                          canon_eval.predict(mixed, Xd, OUT_LEAF)), (layout, dtype)
            finally:
                dev.close()


@pytest.mark.parametrize("layout", ["", "explicit"])
def test_tree_subsets_on_the_device(layout):
    """Tree-sharded mode: the leaves of trees [0, m) and [m, T) served as
    forests of their own (cat_offset cut, cat_bits whole) are the columns of
    the whole forest's, and the oracle's."""
    c = cases.xgb_case(SUBSET_SEED)
    X, leaf, _, _, _ = c.want()[-1]
    m = SUBSET_CUT
    assert m % 8 and 0 < m < c.T
    got = []
    for f in (c.forest, c.forest.tree_subset(0, m), c.forest.tree_subset(m, c.T)):
        dev = _dev(f, layout)
        try:
            if layout == "" and f is c.forest:
                info = dev.info()
                assert info["layout"] == 10 and info["n_stages"] >= 2, info
            got.append(dev.predict(X, OUT_LEAF))
        finally:
            dev.close()
    assert np.array_equal(got[0], leaf)
    assert np.array_equal(np.concatenate(got[1:], axis=1), got[0])


K_CLASS = {1: "K = 1", 3: "K in 3, 4", 4: "K in 3, 4", 5: "K in 5..16", 16: "K in 5..16",
           17: "K = 17"}
REACH = {"heap, one stage", "heap, several stages", "heap, T < 8", "explicit: forest too wide",
         "explicit: bitsets too large", "explicit: tile too low for eight trees",
         "heap forced after the default refused",
         "heap, K = 1", "heap, K in 3, 4", "heap, K in 5..16", "heap, K = 17",
         "heap, LightGBM zero rule"}


def test_fuzz_cases_reach_every_path():
    """The seeds land on the paths they are meant to cover: the categorical
    heap with one and with several stages, with fewer trees than a lane walks,
    with every accumulator width; the hand-over to layout 1 past the widest
    feature image and past the prefetch budget; the forced heap on what the
    default refused; LightGBM's zero rule on the heap."""
    seen = set()
    for seed in cases.XGB_SEEDS:
        c = cases.xgb_case(seed)
        info = _layout(c.forest)
        if info["layout"] == 10:
            seen.add("heap, one stage" if info["n_stages"] == 1 else "heap, several stages")
            if c.T < 8:
                seen.add("heap, T < 8")
            seen.add("heap, " + K_CLASS[c.K])
        else:
            assert info["layout"] == 1, (c.desc, info)
            # eight float32 blocks must fit the prefetch registers, 128 bytes a row
            # of the tile (256 rows up to 64 features, 128 up to 128): without its
            # bitsets a block is 8-byte nodes and 4-byte leaves
            plain = 8 * ((1 << c.depth) - 1) + 4 * (1 << c.depth)
            seen.add("explicit: forest too wide" if c.F > 128 else
                     "explicit: bitsets too large" if 8 * plain <= 128 * (256 if c.F <= 64 else 128)
                     else "explicit: tile too low for eight trees")
            if _layout(c.forest, "cheap")["layout"] == 10:
                seen.add("heap forced after the default refused")
    for seed in cases.LGB_SEEDS:
        c = cases.lgb_case(seed)
        f = c.forest
        numeric = (f.feature >= 0) & ((f.flags & NODE_CATEGORICAL) == 0)
        if np.any(f.flags[numeric] & NODE_ZERO_FLIP) and _layout(f, "cheap")["layout"] == 10:
            seen.add("heap, LightGBM zero rule")
    assert seen == REACH, sorted(REACH - seen)
