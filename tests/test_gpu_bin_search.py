"""The binned kernels' pre-walk phase: bucket-first rank search and the X
prefetch of stage_bins (treeinfer_kernels.h rank_search / stage_bins, host
tables treeinfer_pack.h bucket_tables).

A rank is an integer, b(x) = 1 + #{u < x}, so the new search must give the
very same bins as the 5-ary one for every input.  Each forest is built twice
in one process, with the developer knobs off (TI_BIN_BUCKETS=0, TI_BIN_XPF=0:
the old search and the old staging) and on, and the outputs are compared bit
for bit with each other and with the oracle's C port.  Inputs sit where a
bucket search can go wrong: every threshold and one ulp either side, every
bucket edge lo + k / scale and one ulp either side, +-0, +-inf, NaN,
denormals, +-FLT_MAX.  Whether a forest took the bucket tables shows in its
device_bytes (the two table forms differ in size; a forest that falls back
holds the same bytes either way); _bucket_plan restates the pack-time choice.
"""
import os
import tempfile

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest
from kfserving_amd.forest import OUT_MARGIN, OUT_PREDICT
from kfserving_amd.formats import load_lightgbm_model
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from oracle import port

pytestmark = pytest.mark.gpu

BHEAP = 3
F = 28
ROWS = 1025   # two full 512-row tiles plus one row
OLD = {"TI_BIN_BUCKETS": "0", "TI_BIN_XPF": "0"}
f32 = np.float32
FLT_MAX = np.finfo(f32).max
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, -1.4e-45,
                     FLT_MAX, -FLT_MAX], dtype=f32)


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(autouse=True)
def _knobs_default(monkeypatch):
    monkeypatch.setenv("TI_DEV_KNOBS", "1")
    for k in list(OLD) + ["TI_KARY", "TI_BHEAP_NG", "TI_BHEAP_FIX", "TI_FORCE_LAYOUT", "TI_FIX_PERM",
                          "TI_FIX_SPREAD"]:
        monkeypatch.delenv(k, raising=False)


def _view_thresholds(forest):
    """Per feature the sorted distinct thresholds of the float32 view: the
    largest float32 <= the canonical (left iff x <= t) threshold."""
    t = np.asarray(forest.threshold, dtype=np.float64)
    with np.errstate(over="ignore"):
        v = t.astype(f32)
    v = np.where(v.astype(np.float64) > t, np.nextafter(v, f32(-np.inf)), v).astype(f32)
    feat = np.asarray(forest.feature)
    out = []
    for f in range(forest.n_features):
        d = v[feat == f]
        out.append(np.unique(d[~np.isnan(d)]))
    return out


def _first_nb(thr):
    nb = 2
    while nb < 4096 and nb < max(len(d) for d in thr):
        nb *= 2
    return nb


def _fullest_bucket(thr, nb):
    """The largest number of thresholds in one of nb buckets, or None when a
    feature's span or scale is not a positive finite float32."""
    occ = 0
    for d in thr:
        if len(d) == 0:
            continue
        b = np.zeros(len(d), dtype=np.int64)
        if len(d) > 1:
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                span = f32(d[-1] - d[0])
                scale = f32(nb) / span
                if not (np.isfinite(span) and np.isfinite(scale) and scale > 0):
                    return None
                t = ((d - d[0]).astype(f32) * scale).astype(f32)   # two roundings
            b = np.clip(t, 0, nb - 1).astype(np.int64)
        occ = max(occ, int(np.bincount(b).max()))
    return occ


def _bucket_plan(thr):
    """The pack-time choice restated: NB of the bucket tables -- the first
    power of two from the largest threshold count up to 4,096 at which no
    bucket holds more than 4 thresholds -- or None when the forest keeps the
    5-ary tables (no such NB, at most 24 thresholds a feature so that the 5-ary
    tree has two levels, or a feature's span is unusable)."""
    if max(len(d) for d in thr) <= 24:
        return None
    nb = _first_nb(thr)
    while True:
        occ = _fullest_bucket(thr, nb)
        if occ is None:
            return None
        if occ <= 4:
            return nb
        if nb >= 4096:
            return None
        nb *= 2


def _around(v):
    v = np.asarray(v, dtype=f32)
    return np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))])


def _probe_rows(thr, seed):
    """[rows, len(thr)] float32: column f holds, at seeded rows, feature f's
    thresholds, the bucket edges lo + k / scale computed in float32, one ulp
    either side of each, and the specials; N(0,1) elsewhere.  The rows are
    whole 512-row tiles plus one row, two tiles at least, as many as give
    every probe a row.  Rows 512 .. 1023 (the second tile) hold no NaN, so both
    the NaN step and the fast step of the walk run."""
    plan = _bucket_plan(thr)
    nb = plan or _first_nb(thr)
    cols = []
    for d in thr:
        probes = [SPECIALS]
        if len(d):
            probes.append(_around(d))
        if len(d) > 1:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                scale = f32(nb) / f32(d[-1] - d[0])
                edges = (d[0] + np.arange(nb + 1, dtype=f32) / scale).astype(f32)
            probes.append(_around(edges[np.isfinite(edges)]))
        cols.append(np.concatenate(probes).astype(f32))
    rows = max(ROWS, 512 * -(-max(len(p) for p in cols) // 512) + 1)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, len(thr))).astype(f32)
    for f, p in enumerate(cols):
        X[rng.permutation(rows)[:len(p)], f] = p
    tile1 = X[512:1024]
    tile1[np.isnan(tile1)] = 0.25
    return X


def _set_feature_thresholds(trees, f, fn, seed):
    """Redraw the thresholds of every node that tests feature f with fn(rng, n)."""
    rng = np.random.default_rng(seed)
    for t in trees:
        n_int = int((t["cleft"] >= 0).sum())
        at = np.nonzero((t["sindex"][:n_int] & 0x7FFFFFFF) == f)[0]
        t["value"][at] = fn(rng, len(at)).astype(f32)


def _base(n_trees=8, seed=71, **kw):
    return xf.synthetic_complete_trees(n_trees, 8, F, seed=seed, **kw)


def _case_u16():
    # > 253 distinct thresholds a feature: u16 bins
    return _base(n_trees=40, seed=72)


def _case_crowded():
    # ~1,400 thresholds a feature: the fullest of 4,096 buckets holds more
    # than 4 (as in the 500-tree headline forest), which keeps the 5-ary search
    return _base(n_trees=150, seed=78)


def _case_one_threshold():
    trees, ti = _base(seed=73)
    _set_feature_thresholds(trees, 3, lambda rng, n: np.full(n, 0.125), 1)
    return trees, ti


def _case_unused_feature():
    trees, ti = _base(seed=74)
    for t in trees:
        n_int = int((t["cleft"] >= 0).sum())
        s = t["sindex"][:n_int]
        s[(s & 0x7FFFFFFF) == 5] += 1   # feature 5 -> 6, the default-left bit kept
    return trees, ti


def _case_outlier():
    # one feature's thresholds in one bucket but for an outlier at 1e30: the
    # fullest bucket needs as many steps as the 5-ary search, which stays
    trees, ti = _base(seed=75)

    def draw(rng, n):
        v = rng.uniform(1.0, 2.0, n)
        v[:1] = 1e30
        return v
    _set_feature_thresholds(trees, 0, draw, 2)
    return trees, ti


def _case_overflow():
    # hi - lo overflows float32
    trees, ti = _base(seed=76)

    def draw(rng, n):
        v = rng.standard_normal(n)
        k = min(n, 2)
        v[:k] = [-3e38, 3e38][:k]
        return v
    _set_feature_thresholds(trees, 1, draw, 3)
    return trees, ti


def _case_hist():
    # thresholds on 253 histogram bin bounds: u8 bins, one search step
    return _base(n_trees=40, seed=77, max_bin=254)


CASES = {
    # name: (builder, takes the bucket tables (False: the 5-ary fallback), bin bits)
    "base": (_base, True, 8),
    "u16": (_case_u16, True, 16),
    "u16_crowded_fallback": (_case_crowded, False, 16),
    "one_threshold": (_case_one_threshold, True, 8),
    "unused_feature": (_case_unused_feature, True, 8),
    "outlier_fallback": (_case_outlier, False, 8),
    "overflow_fallback": (_case_overflow, False, 8),
    "hist_u8": (_case_hist, True, 8),
}


def _pair(forest):
    """(old, new): the forest with the knobs off and with the defaults."""
    old = _with_env(OLD, lambda: DeviceForest(forest, [0]))
    return old, DeviceForest(forest, [0])


@pytest.mark.parametrize("name", list(CASES))
def test_bucket_search_matches_old_search_and_oracle(name):
    build, buckets, bits = CASES[name]
    trees, ti = build()
    forest = xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    thr = _view_thresholds(forest)
    assert (_bucket_plan(thr) is not None) == buckets   # the case is what its name says
    X = _probe_rows(thr, seed=5)
    want = port.xgb_predict(trees, ti, 1, 0.0, F, X)[:, 0]
    old, new = _pair(forest)
    try:
        got_old = _with_env(OLD, lambda: old.predict(X, OUT_MARGIN))
        got_new = new.predict(X, OUT_MARGIN)
        # each half of the change on its own: old search with the register
        # staging, new search with the staging through LDS
        got_old_xpf = old.predict(X, OUT_MARGIN)
        got_new_lds = _with_env({"TI_BIN_XPF": "0"}, lambda: new.predict(X, OUT_MARGIN))
        # the indexed walk (the leaf ids' kernel) bins through the LDS staging too
        got_new_idx = _with_env({"TI_BHEAP_FIX": "0"}, lambda: new.predict(X, OUT_MARGIN))
        io, inw = old.info(), new.info()
        assert inw["layout"] == BHEAP and inw["walk"] == 2 and inw["bin_bits"] == bits, inw
        if buckets:
            assert inw["device_bytes"] != io["device_bytes"]
        else:
            assert inw["device_bytes"] == io["device_bytes"]
        assert np.array_equal(got_old, want)
        for got in (got_new, got_old_xpf, got_new_lds, got_new_idx):
            assert np.array_equal(got, got_old)
    finally:
        old.close()
        new.close()


@pytest.mark.parametrize("stride", [29, 32], ids=["unaligned_rows", "aligned_padded_rows"])
def test_row_strides_take_the_scalar_and_the_vector_staging(stride):
    """A row stride of 29 floats is not 16-byte aligned (the scalar X path
    through LDS); 32 floats is, with rows wider than the features (the
    register path, one 16-byte load per lane and chunk)."""
    import torch
    trees, ti = _base()
    forest = xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    X = _probe_rows(_view_thresholds(forest) + [np.zeros(0, f32)] * (stride - F), seed=6)
    rows = X.shape[0]
    want = port.xgb_predict(trees, ti, 1, 0.0, F, np.ascontiguousarray(X[:, :F]))[:, 0]
    Xt = torch.from_numpy(X).cuda()
    old, new = _pair(forest)
    try:
        outs = []
        for dev, env in ((old, OLD), (new, {})):
            out = torch.empty(rows, dtype=torch.float32, device="cuda")
            _with_env(env, lambda: dev.predict_device(Xt.data_ptr(), 0, rows, stride, stride, OUT_MARGIN,
                                                      out.data_ptr(), out.numel()))
            torch.cuda.synchronize()
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], want)
        assert np.array_equal(outs[1], outs[0])
    finally:
        old.close()
        new.close()


def test_all_nan_tile_and_ragged_last_tile():
    trees, ti = _base()
    forest = xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    X = _probe_rows(_view_thresholds(forest), seed=7)
    X[:512] = np.nan          # a tile of nothing but NaN
    want = port.xgb_predict(trees, ti, 1, 0.0, F, X)[:, 0]
    old, new = _pair(forest)
    try:
        for rows in (X.shape[0], 700, 1):
            got_old = _with_env(OLD, lambda: old.predict(X[:rows], OUT_MARGIN))
            assert np.array_equal(got_old, want[:rows]), rows
            assert np.array_equal(new.predict(X[:rows], OUT_MARGIN), got_old), rows
    finally:
        old.close()
        new.close()


def test_lightgbm_leafwise_float32_and_float64_views():
    """Shallow leaf-wise LightGBM trees on the binned heap's indexed walk:
    float32 input searches the bucket tables, float64 input keeps its own
    Eytzinger tables."""
    nf = 20
    trees = lf.synthetic_leafwise_trees(50, 12, nf, seed=8,
                                        missing_types=(lf.MISSING_NONE, lf.MISSING_NAN))
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.txt")
        lf.write_lightgbm_text(p, trees, nf, "binary sigmoid:1")
        forest = load_lightgbm_model(p)
    assert forest.depths().max() <= 8
    thr = _view_thresholds(forest)
    assert _bucket_plan(thr) is not None
    X = _probe_rows(thr, seed=9)
    want = port.lgb_predict_raw(trees, 1, nf, X.astype(np.float64))[:, 0]
    old, new = _pair(forest)
    try:
        for Xv in (X, X.astype(np.float64)):
            got_old = _with_env(OLD, lambda: old.predict(Xv, OUT_MARGIN))
            assert np.array_equal(got_old, want)
            assert np.array_equal(new.predict(Xv, OUT_MARGIN), got_old)
        assert new.info()["layout"] == BHEAP
        assert new.info()["device_bytes"] != old.info()["device_bytes"]
    finally:
        old.close()
        new.close()


def test_sklearn_forest():
    from sklearn.ensemble import RandomForestRegressor
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn, tree_arrays_from_sklearn
    nf = 12
    rng = np.random.default_rng(1)
    Xtr = rng.standard_normal((400, nf)).astype(f32)
    y = Xtr[:, 0] * Xtr[:, 1] + np.sin(Xtr[:, 2]) + 0.1 * rng.standard_normal(400)
    est = RandomForestRegressor(n_estimators=8, max_depth=7, random_state=0).fit(Xtr, y)
    forest = forest_from_sklearn(est)
    arrays = [tree_arrays_from_sklearn(e.tree_) for e in est.estimators_]
    X = _probe_rows(_view_thresholds(forest), seed=10)
    want = port.sk_predict(arrays, 1, nf, X)[:, 0]
    old, new = _pair(forest)
    try:
        got_old = _with_env(OLD, lambda: old.predict(X, OUT_PREDICT))
        assert np.array_equal(got_old, want)
        assert np.array_equal(new.predict(X, OUT_PREDICT), got_old)
    finally:
        old.close()
        new.close()


def test_knobs_need_the_dev_gate(monkeypatch):
    trees, ti = _base()
    forest = xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    X = np.zeros((1, F), dtype=f32)

    def info():
        d = DeviceForest(forest, [0])
        try:
            d.predict(X, OUT_MARGIN)   # the replica is resident
            return d.info()
        finally:
            d.close()

    monkeypatch.delenv("TI_DEV_KNOBS", raising=False)
    default = info()
    for k, v in OLD.items():
        monkeypatch.setenv(k, v)
    assert info() == default                  # no gate: the same tables
    monkeypatch.setenv("TI_DEV_KNOBS", "0")
    assert info() == default
    monkeypatch.setenv("TI_DEV_KNOBS", "1")
    assert info()["device_bytes"] != default["device_bytes"]   # the 5-ary tables are back
