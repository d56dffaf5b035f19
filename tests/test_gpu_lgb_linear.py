"""LightGBM linear-tree models on the device: the forest's own walk for the
leaf ids, then linear_leaf_kernel (treeinfer_linear.h) on the raw features.

Raw scores are compared bit for bit with tests/linear_eval.py (the same IEEE
operations in the same order; NaN scores compare as NaN, whose sign and
payload differ between x86 and the GPU); transformed scores within the
project's 1e-5 relative error.
"""
import functools
import os
import tempfile
import threading

import numpy as np
import pytest
import torch

from kfserving_amd.engine import (OPT_HOST_REGISTER, OPT_LINEAR_SCRATCH_MB, DeviceForest,
                                  TreeInferError)
from kfserving_amd.forest import (MISSING_NONE, OUT_CONTRIB, OUT_LEAF, OUT_MARGIN, OUT_PREDICT,
                                  TI_F64)
from kfserving_amd.formats import lightgbm_format as lf
from oracle import lgb_ref, port
from tests import linear_eval
from tests.test_lgb_linear_format import SIX_FELL, SIX_ROWS, SIX_ROWS_TEXT, SIX_WANT

pytestmark = pytest.mark.gpu

RTOL = 1e-5
F = 40
LEAVES = 63
N_STAT = 2055     # rows the fallback / NaN-score shares are taken over
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-36, 1e-35, 2e-35, np.inf, -np.inf])


def _text_of(trees, n_features, objective, num_class=1, names=None):
    fd, path = tempfile.mkstemp(suffix=".txt")
    os.close(fd)
    try:
        lf.write_lightgbm_text(path, trees, n_features, objective, num_class=num_class,
                               feature_names=names)
        with open(path) as fh:
            return fh.read()
    finally:
        os.remove(path)


@functools.lru_cache(maxsize=None)
def _model(T, max_terms, K=1, leaves=LEAVES, seed=0, missing=None, n_feat=F):
    """(trees, text, forest) of a seeded linear model; every 4th tree is
    constant (a one-tree model is all linear)."""
    kw = {} if missing is None else {"missing_types": missing}
    trees = lf.synthetic_leafwise_trees(T, leaves, n_feat, seed=100 + seed + T, **kw)
    lf.add_linear_leaves(trees, n_feat, seed=200 + seed + T, max_terms=max_terms,
                         const_tree_every=4 if T > 1 else 0)
    objective = "binary sigmoid:1" if K == 1 else f"multiclass num_class:{K}"
    text = _text_of(trees, n_feat, objective, num_class=K)
    return trees, text, lf.parse_lightgbm_text(text)


def _rows(n, seed, n_cols=F):
    """N(0,1) with 5 % NaN and 5 % of the values at which the zero map, the
    NaN fallback and inf propagation change the answer."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, n_cols))
    u = rng.random(X.shape)
    X[u < 0.05] = np.nan
    sp = (u >= 0.05) & (u < 0.10)
    X[sp] = SPECIALS[rng.integers(0, len(SPECIALS), int(sp.sum()))]
    return X


def _dev(forest, layout=None):
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


def _squeeze(score, K):
    return score[:, 0] if K == 1 else score


# ----------------------------------------------------------- the six rows
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_six_hand_computed_rows(dtype):
    f = lf.parse_lightgbm_text(SIX_ROWS_TEXT)
    dev = DeviceForest(f, [0])
    assert dev.info()["linear"] == 1
    X = SIX_ROWS.astype(dtype)          # every value is float32-representable
    got = dev.predict(X, OUT_MARGIN)
    print("six rows", dtype.__name__, got.tolist())
    assert linear_eval.same_bits(got, SIX_WANT)
    assert np.isnan(got[5])
    score, fell = linear_eval.raw_scores(SIX_ROWS_TEXT, X)
    assert fell[:, 0].tolist() == SIX_FELL and linear_eval.same_bits(got, score[:, 0])
    dev.close()


# ------------------------------------------- trees x rows x terms x groups
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("max_terms", [0, 1, F])
@pytest.mark.parametrize("T", [1, 31, 33, 65, 130])
def test_margins_bit_exact(T, max_terms, K):
    """Trees on either side of the kernel's 32-tree leaf-id chunk, row counts
    around the wave and the tile, leaves without terms, with one, with up to
    every feature.

    The shares of the two branches, over N_STAT rows.  A term reads a NaN with
    probability 0.05, so a leaf of m terms falls back with 1 - 0.95^m:
      max_terms = 0: no leaf has a term, nothing falls back (asserted: none);
      max_terms = 1: half the leaves have one, 2.5 % (x 3/4 linear trees)
                     -- under the 5 % floor, asserted only as "some";
      max_terms = F: m uniform on 0..40, mean 57 %, x 3/4 linear trees = 43 %:
                     asserted inside [5 %, 60 %] for T >= 31 (one tree of 63
                     leaves is too few leaves for a share to be stable).
    NaN scores (0.0 * inf, or +inf and -inf meeting in one sum) need a handful
    of trees to be certain over N_STAT rows: asserted for T >= 31."""
    _, text, forest = _model(T, max_terms, K)
    dev = DeviceForest(forest, [0])
    assert dev.info()["linear"] == 1
    for dtype in (np.float64, np.float32):
        X = _rows(N_STAT, seed=7 * T + max_terms + K).astype(dtype)
        want, fell = linear_eval.raw_scores(text, X)
        share = fell.mean()
        n_nan = int(np.isnan(want).any(axis=1).sum())
        print(f"T={T} max_terms={max_terms} K={K} {dtype.__name__}: fallback share "
              f"{share:.4f}, rows with a NaN score {n_nan}")
        if max_terms == 0:
            assert not fell.any()
        else:
            assert fell.any() and not fell.all()
            if T >= 31:
                assert n_nan > 0
                if max_terms == F:
                    assert 0.05 <= share <= 0.60
        R = dev.linear_tile_rows(dtype)
        for rows in (1, 63, 65, R - 1, R + 1, 2 * R + 7, N_STAT):
            got = dev.predict(X[:rows], OUT_MARGIN)
            assert linear_eval.same_bits(got, _squeeze(want[:rows], K)), (dtype, rows)
        got = dev.predict(X[:2 * R + 7], OUT_PREDICT)
        ref = _squeeze(linear_eval.predict(text, X[:2 * R + 7]), K)
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0, equal_nan=True)
    dev.close()


# ------------------------------------------------------ narrow and wide X
def test_missing_and_extra_columns():
    _, text, forest = _model(33, 4)
    dev = DeviceForest(forest, [0])
    for dtype in (np.float64, np.float32):
        R = dev.linear_tile_rows(dtype)
        base = _rows(R + 9, seed=3).astype(dtype)
        narrow = np.ascontiguousarray(base[:, :F - 7])              # columns 33..39 read NaN
        want, fell = linear_eval.raw_scores(text, narrow)
        full = np.concatenate([narrow, np.full((R + 9, 7), np.nan, dtype)], axis=1)
        want_full, fell_full = linear_eval.raw_scores(text, full)
        assert linear_eval.same_bits(want, want_full) and np.array_equal(fell, fell_full)
        # every reached leaf with a term on a missing column fell back
        leaves = linear_eval.tree_outputs(text, narrow)[2]
        reads_missing = np.zeros_like(fell)
        for t, tr in enumerate(linear_eval.read_linear_blocks(text)):
            if tr.is_linear:
                hit = np.array([bool((f >= F - 7).any()) for f in tr.leaf_features])
                reads_missing[:, t] = hit[leaves[:, t]]
        assert reads_missing.any() and fell[reads_missing].all()
        assert (fell & ~reads_missing).any()       # and NaNs inside the columns still do
        assert linear_eval.same_bits(dev.predict(narrow, OUT_MARGIN), want[:, 0])
        wide = np.concatenate([_rows(R + 9, seed=4).astype(dtype),
                               np.full((R + 9, 5), 1e30, dtype)], axis=1)  # extra columns ignored
        want_w, _ = linear_eval.raw_scores(text, wide[:, :F])
        assert linear_eval.same_bits(dev.predict(wide, OUT_MARGIN), want_w[:, 0])
    dev.close()


def test_wide_forest_reads_features_from_hbm():
    """130 float64 columns do not fit the 64 KiB LDS image even at 64 rows a
    tile: the kernel reads the row in HBM (tiles of 256 rows), with the
    explicit kernel's n_cols rule; float32 X of the same forest still fits."""
    W = 130
    _, text, forest = _model(33, 6, n_feat=W)
    dev = DeviceForest(forest, [0])
    assert W * 64 * 8 > 64 * 1024 and dev.linear_tile_rows(np.float64) == 256
    assert dev.linear_tile_rows(np.float32) == 64
    X = _rows(2 * 256 + 7, seed=21, n_cols=W)
    want, fell = linear_eval.raw_scores(text, X)
    assert fell.any() and np.isnan(want).any()
    assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
    X32 = X.astype(np.float32)
    assert linear_eval.same_bits(dev.predict(X32, OUT_MARGIN),
                                 linear_eval.raw_scores(text, X32)[0][:, 0])
    narrow = np.ascontiguousarray(X[:, :W - 30])
    assert linear_eval.same_bits(dev.predict(narrow, OUT_MARGIN),
                                 linear_eval.raw_scores(text, narrow)[0][:, 0])
    dev.set_option(OPT_LINEAR_SCRATCH_MB, 0)           # three row blocks
    assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
    dev.close()


# ------------------------------------------------- every walk for pass 1
def test_every_layout_same_margins():
    _, text, forest = _model(65, 4)
    X = _rows(777, seed=5)
    want, _ = linear_eval.raw_scores(text, X)
    X32 = X.astype(np.float32)
    want32, _ = linear_eval.raw_scores(text, X32)
    seen = {}
    for layout in (None, "explicit", "rexplicit", "lexplicit", "texplicit"):
        dev = _dev(forest, layout)
        info = dev.info()
        assert info["linear"] == 1
        seen[layout] = info["layout"]
        assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0]), layout
        assert linear_eval.same_bits(dev.predict(X32, OUT_MARGIN), want32[:, 0]), layout
        dev.close()
    print("layouts", seen)
    os.environ["TI_LINEAR_FEAT_LDS"] = "0"      # features from HBM where the image would fit
    try:
        dev = DeviceForest(forest, [0])
        assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
        assert linear_eval.same_bits(dev.predict(X32, OUT_MARGIN), want32[:, 0])
        dev.close()
    finally:
        del os.environ["TI_LINEAR_FEAT_LDS"]
    assert seen["explicit"] == 1 and seen["rexplicit"] == 6
    assert seen[None] != 1       # a linear forest keeps its fast walk


def test_shallow_forest_on_a_heap_layout():
    """Trees of 8 leaves without zero-missing nodes fit the heap layouts, whose
    padded leaves report the library leaf id too."""
    _, text, forest = _model(33, 3, leaves=8, missing=(MISSING_NONE,))
    dev = DeviceForest(forest, [0])
    info = dev.info()
    print("shallow layout", info["layout"], "depth", info["depth"])
    assert info["linear"] == 1
    X = _rows(700, seed=6)
    want, fell = linear_eval.raw_scores(text, X)
    assert fell.any()
    assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
    dev.close()


# ------------------------------------------------------------ row blocks
def test_scratch_cap_splits_row_blocks():
    _, text, forest = _model(130, 4)
    dev = DeviceForest(forest, [0])
    R = dev.linear_tile_rows(np.float64)
    X = _rows(2 * R + 7, seed=8)
    want, _ = linear_eval.raw_scores(text, X)
    whole = dev.predict(X, OUT_MARGIN)
    dev.set_option(OPT_LINEAR_SCRATCH_MB, 0)       # one tile a block: three blocks
    split = dev.predict(X, OUT_MARGIN)
    assert linear_eval.same_bits(whole, want[:, 0]) and linear_eval.same_bits(split, want[:, 0])
    np.testing.assert_allclose(dev.predict(X, OUT_PREDICT),
                               linear_eval.predict(text, X)[:, 0], rtol=RTOL, equal_nan=True)
    dev.set_option(OPT_LINEAR_SCRATCH_MB, 1024)
    with pytest.raises(TreeInferError):
        dev.set_option(OPT_LINEAR_SCRATCH_MB, -1)
    dev.close()


@pytest.fixture
def small_chunks():
    old = os.environ.get("TI_CHUNK_MB")
    os.environ["TI_CHUNK_MB"] = "1"
    yield
    if old is None:
        del os.environ["TI_CHUNK_MB"]
    else:
        os.environ["TI_CHUNK_MB"] = old


def test_host_pipeline_chunks(small_chunks):
    """8,000 float64 rows of 40 columns are 2.4 MiB: three 1 MiB chunks on the
    pipelined path, staged and with the caller's buffers registered."""
    _, text, forest = _model(33, 4)
    X = _rows(8000, seed=9)
    want, _ = linear_eval.raw_scores(text, X)
    dev = DeviceForest(forest, [0])
    assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
    dev.set_option(OPT_HOST_REGISTER, 1)
    assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
    dev.close()


def test_two_slots_shard_rows():
    _, text, forest = _model(33, 4)
    X = _rows(1001, seed=10)
    want, _ = linear_eval.raw_scores(text, X)
    dev = DeviceForest(forest, [0, 0])
    assert linear_eval.same_bits(dev.predict(X, OUT_MARGIN), want[:, 0])
    dev.close()


def test_concurrent_predicts_on_one_handle():
    _, text, forest = _model(65, 4, K=3)
    dev = DeviceForest(forest, [0])
    Xs = [_rows(1500, seed=11), _rows(1300, seed=12)]
    serial = [dev.predict(x, OUT_MARGIN) for x in Xs]
    for x, s in zip(Xs, serial):
        assert linear_eval.same_bits(s, linear_eval.raw_scores(text, x)[0])
    got = [None, None]

    def run(i):
        for _ in range(4):
            got[i] = dev.predict(Xs[i], OUT_MARGIN)

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for g, s in zip(got, serial):
        assert linear_eval.same_bits(g, s)
    dev.close()


def test_predict_device_on_a_side_stream():
    _, text, forest = _model(65, 4, K=3)
    dev = DeviceForest(forest, [0])
    X = _rows(900, seed=13)
    for kind in (OUT_MARGIN, OUT_PREDICT):
        host = dev.predict(X, kind)
        Xd = torch.from_numpy(X).cuda()
        out = torch.empty((900, 3), dtype=torch.float64, device="cuda")
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            dev.predict_device(Xd.data_ptr(), TI_F64, 900, F, F, kind, out.data_ptr(),
                               out.numel(), stream=st.cuda_stream)
        st.synchronize()
        assert linear_eval.same_bits(out.cpu().numpy(), host)
    dev.close()


def test_transform_device_of_linear_margins():
    _, text, forest = _model(33, 4, K=3)
    dev = DeviceForest(forest, [0])
    X = _rows(500, seed=14)
    margin = torch.from_numpy(dev.predict(X, OUT_MARGIN)).cuda()
    out = torch.empty_like(margin)
    dev.transform_device(margin.data_ptr(), 500, out.data_ptr(), out.numel(),
                         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert linear_eval.same_bits(out.cpu().numpy(), dev.predict(X, OUT_PREDICT))
    dev.close()


# ------------------------------------------------ leaf ids, contributions
def test_leaf_ids_equal_the_constant_forest():
    trees, text, forest = _model(65, 4)
    const = lf.parse_lightgbm_text(_text_of(lf.strip_linear_leaves(trees), F, "binary sigmoid:1"))
    assert not const.has_linear
    X = _rows(600, seed=15)
    a, b = DeviceForest(forest, [0]), DeviceForest(const, [0])
    assert b.info()["linear"] == 0
    leaves = a.predict(X, OUT_LEAF)
    assert np.array_equal(leaves, b.predict(X, OUT_LEAF))
    assert np.array_equal(leaves, linear_eval.tree_outputs(text, X)[2])
    a.close()
    b.close()


def test_contributions_are_refused():
    _, _, forest = _model(31, 4)
    dev = DeviceForest(forest, [0])
    with pytest.raises(TreeInferError) as e:
        dev.predict(_rows(10, seed=16), OUT_CONTRIB)
    assert e.value.code == -4 and "linear" in str(e.value)
    dev.close()


def test_more_than_16_groups_refused_at_create():
    _, _, forest = _model(34, 2, K=17)
    with pytest.raises(TreeInferError) as e:
        DeviceForest(forest, [0])
    assert e.value.code == -4 and "linear" in str(e.value)


# ----------------------------------------------------------------- serving
def test_lgbserver_loads_a_linear_model(tmp_path):
    from kfserving_amd.lgbserver import LightGBMModel
    names = ["a", "b", "c", "d"]
    trees = lf.synthetic_leafwise_trees(10, 15, 4, seed=41)
    lf.add_linear_leaves(trees, 4, seed=42, max_terms=3, const_tree_every=5)
    path = str(tmp_path / "model.bst")
    lf.write_lightgbm_text(path, trees, 4, "binary sigmoid:1", feature_names=names)
    model = LightGBMModel("m", str(tmp_path), nthread=1)
    assert model.load()
    req = {"a": {0: 0.3, 1: -1.0, 2: float("nan")}, "b": {0: 7.0, 1: 1e-36, 2: 0.5},
           "c": {0: 0.0, 1: 2.0, 2: -0.25}, "d": {0: 1.0, 1: 0.5, 2: 3.0}}
    got = np.asarray(model.predict({"inputs": [req]})["predictions"])
    m = lgb_ref.read_lgb_text(path)
    X = lgb_ref.rows_from_inputs(m, [req])
    text = open(path).read()
    assert linear_eval.raw_scores(text, X)[1].any()       # the NaN row falls back somewhere
    np.testing.assert_allclose(got, linear_eval.predict(text, X)[:, 0], rtol=RTOL)


# ------------------------------------------------ the old path, undisturbed
def test_constant_forest_still_matches_the_port():
    trees = lf.synthetic_leafwise_trees(65, LEAVES, F, seed=51)
    forest = lf.parse_lightgbm_text(_text_of(trees, F, "binary sigmoid:1"))
    assert not forest.has_linear
    dev = DeviceForest(forest, [0])
    assert dev.info()["linear"] == 0
    X = _rows(1500, seed=17)
    want = port.lgb_predict_raw(trees, 1, F, X)[:, 0]
    got = dev.predict(X, OUT_MARGIN)
    assert linear_eval.same_bits(got, want)
    X32 = X.astype(np.float32)
    assert linear_eval.same_bits(dev.predict(X32, OUT_MARGIN),
                                 port.lgb_predict_raw(trees, 1, F, X32.astype(np.float64))[:, 0])
    dev.close()
