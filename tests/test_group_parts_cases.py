"""The conditions under which tests/test_gpu_group_parts.py cannot pass by
accident, asserted from the references of tests/group_parts_cases.py alone (no
GPU).

Every forest is in group parts, split as its case states, and each part's
contributions row lies on the side of kShapLdsW (128 columns) that sends it to
the kernel the case is named for.

A misplaced row or column block cannot hide in a generated case: in every
batch of 64 rows or more and for every kind, the rows of the reference are
pairwise distinct within the column block of each part of at least 4 groups,
no two parts' blocks are equal, and two successive batches of a call sequence
differ in every row.  A tail part of fewer than 4 groups cannot meet the first
condition (one group of 2 trees takes a handful of values), which is why
k20-sliced has a 4-group tail; for the one-group tails of k17-design and
k33-generic and the two-group tail of lgb-k18-f64 only this is asserted: the
tail's block takes at least 2 distinct values over the batch.

The references agree among themselves: contributions plus bias sum to the
margins at 1e-9 in float64, and tests/canon_eval.py gives the leaf ids,
margins and predictions of the library restatements."""
import numpy as np
import pytest

from kfserving_amd.forest import (NODE_NAN_LEFT, NODE_ZERO_FLIP, OUT_CONTRIB, OUT_CONTRIB_APPROX,
                                  OUT_LEAF, OUT_MARGIN, OUT_PREDICT, TI_F32, TI_F64)
from tests import canon_eval
from tests import group_parts_cases as gp
from tests import shap_cat_eval as sc

KINDS = [OUT_MARGIN, OUT_PREDICT, OUT_LEAF, OUT_CONTRIB, OUT_CONTRIB_APPROX]
KIND_IDS = ["margin", "predict", "leaf", "contrib", "approx"]


@pytest.mark.parametrize("name", gp.CASES + ["k20-softmax"])
def test_forest_is_in_parts_as_stated(name):
    c = gp.case(name)
    f = c.forest
    assert f.n_groups > gp.MAX_GROUPS
    split = tuple(kc for _, kc in gp.parts(f))
    assert split == c.split and sum(split) == f.n_groups
    assert all(kc <= gp.MAX_GROUPS for kc in split)
    if f.leaf_width == 1:                     # every part has trees (create_chunked refuses otherwise)
        for k0, kc in gp.parts(f):
            assert len(gp.part_columns(f, OUT_LEAF, k0, kc)) > 0
    else:
        assert f.leaf_width == f.n_groups


def _paths(f, k0, kc):
    """Root-to-leaf paths of the trees a part holds."""
    trees = range(f.n_trees) if f.leaf_width != 1 else gp.part_columns(f, OUT_LEAF, k0, kc)
    n = 0
    for t in trees:
        b, e = int(f.tree_offset[t]), int(f.tree_offset[t + 1])
        n += int(np.count_nonzero(f.feature[b:e] < 0))
    return n


def test_each_part_reaches_the_kernel_it_is_meant_to():
    width = {n: [kc * (gp.case(n).forest.n_features + 1) for kc in gp.case(n).split] for n in gp.CASES}
    assert width["k17-design"] == [96, 6]
    assert width["k20-sliced"] == [112, 28]
    assert width["k33-generic"] == [144, 144, 9]
    assert width["lgb-k18-f64"] == [112, 14]
    assert width["sk-k20-vector"] == [112, 28]
    for n in ("k17-design", "k20-sliced", "lgb-k18-f64", "sk-k20-vector"):
        assert all(w <= gp.LDS_W for w in width[n]), n            # contrib_reg_kernel
        assert sc.path_element_kinds(gp.case(n).forest)["max_unique"] <= 32
    assert width["k33-generic"][0] > gp.LDS_W and width["k33-generic"][1] > gp.LDS_W   # contrib_kernel
    # path slices need kShapMinPathsPerSlice = 256 paths a slice
    assert _paths(gp.case("k17-design").forest, 0, 16) == 64      # never sliced
    assert _paths(gp.case("k20-sliced").forest, 0, 16) == 768     # TI_SHAP_SLICES=2 holds
    assert gp.case("k20-sliced").forest.accum_dtype == TI_F32
    assert gp.case("k33-generic").forest.accum_dtype == TI_F32    # the float64 accumulator scratch
    lgb = gp.case("lgb-k18-f64").forest
    assert lgb.accum_dtype == TI_F64 and lgb.n_trees == 36
    internal = lgb.feature >= 0
    assert lgb.lgb_zero_map or np.any(lgb.flags[internal] & NODE_ZERO_FLIP)
    assert np.any(lgb.flags[internal] & NODE_NAN_LEFT) and not np.all(lgb.flags[internal] & NODE_NAN_LEFT)
    sk = gp.case("sk-k20-vector").forest
    assert sk.leaf_width == 20 and sk.accum_dtype == TI_F64
    assert gp.part_columns(sk, OUT_LEAF, 0, 16) is None           # launch_chunked's early return


def test_call_sequences():
    assert gp.SIZES == (70, 6, 70, 1, 257, 8, 64, 65) and max(gp.SIZES) <= 257
    for name in gp.CASES:
        seq = gp.sequence(name)
        assert [n for n, _ in seq] == list(gp.SIZES)
        assert len({s for _, s in seq}) == len(seq)
        X = gp.batch(name, 70, seq[0][1])
        assert np.array_equal(X, X.astype(np.float32).astype(np.float64), equal_nan=True)
        assert np.isnan(X).any() == (gp.case(name).lib != "sk")


def _distinct_rows(block):
    return len(np.unique(np.ascontiguousarray(block), axis=0))


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("name", gp.GENERATED)
def test_a_misplaced_block_cannot_hide(name, kind):
    f = gp.case(name).forest
    seq = gp.sequence(name)
    for i, (n, seed) in enumerate(seq):
        if n < 64:
            continue
        w = gp.want(name, kind, n, seed).reshape(n, -1)
        blocks = []
        for k0, kc in gp.parts(f):
            cols = gp.part_columns(f, kind, k0, kc)
            if cols is None:
                continue
            blocks.append(w[:, cols])
            if kc >= 4:
                assert _distinct_rows(w[:, cols]) == n, (name, kind, i, k0)
            else:
                assert len(np.unique(w[:, cols])) >= 2, (name, kind, i, k0)
        for a in range(len(blocks)):
            for b in range(a + 1, len(blocks)):
                assert blocks[a].shape != blocks[b].shape or not np.array_equal(blocks[a], blocks[b])
        # against the batch the call before it left in the buffers: no row the same
        pn, pseed = seq[i - 1]
        if i and blocks:
            prev = gp.want(name, kind, pn, pseed).reshape(pn, -1)
            m = min(n, pn)
            assert np.all(np.any(prev[:m] != w[:m], axis=1)), (name, kind, i)


@pytest.mark.parametrize("kind", [OUT_MARGIN, OUT_CONTRIB, OUT_CONTRIB_APPROX],
                         ids=["margin", "contrib", "approx"])
def test_k17_tail_and_batches_differ(kind):
    """k17-design is kept as DESIGN.md has it: its 16-group part's rows are
    pairwise distinct at 70 rows too, and its one-group tail takes at least 2
    values."""
    f = gp.case("k17-design").forest
    for n, seed in gp.K17_70:
        w = gp.want("k17-design", kind, n, seed)
        (k0, kc), (t0, tc) = gp.parts(f)
        assert _distinct_rows(w[:, gp.part_columns(f, kind, k0, kc)]) == n
        assert len(np.unique(w[:, gp.part_columns(f, kind, t0, tc)])) >= 2


@pytest.mark.parametrize("kind", [OUT_MARGIN, OUT_CONTRIB], ids=["margin", "contrib"])
def test_k17_two_slot_batches(kind):
    """The 257-row batches of the two-slot test: the rows are cut 129 + 128, so
    a shard that lands in the other's place, or a batch left from the call
    before, must differ from the right answer in every row it covers.  (16
    depth-2 trees cannot make 257 rows pairwise distinct; what two slots can
    get wrong is a shard, not a row.)"""
    f = gp.case("k17-design").forest
    cols = gp.part_columns(f, kind, 0, 16)
    prev = None
    for n, seed in gp.K17_257:
        w = gp.want("k17-design", kind, n, seed)[:, cols]
        per = (n + 1) // 2
        assert np.all(np.any(w[:n - per] != w[per:], axis=1)), seed
        assert prev is None or np.all(np.any(prev != w, axis=1)), seed
        prev = w


def test_one_part_case():
    """k16-one-part: 16 groups, so no group part; its contributions take
    contrib_reg_kernel (112 columns) and can take path slices (768 paths)."""
    c = gp.case("k16-one-part")
    f = c.forest
    assert f.n_groups == gp.MAX_GROUPS and gp.parts(f) == [(0, 16)] and c.split == (16,)
    assert f.n_groups * (f.n_features + 1) == 112 <= gp.LDS_W and _paths(f, 0, 16) == 768
    n, seed = gp.sequence("k16-one-part")[4]
    assert n == 257
    assert np.array_equal(canon_eval.predict(f, gp.batch("k16-one-part", n, seed), OUT_MARGIN),
                          gp.want("k16-one-part", OUT_MARGIN, n, seed))


def _margin64(f, lv):
    """[rows, K] float64 margins from the leaves each row reaches."""
    m = np.zeros((lv.shape[0], f.n_groups))
    for t in range(f.n_trees):
        v = np.asarray(f.leaf_value, dtype=np.float64)[f.tree_offset[t] + lv[:, t]]
        if f.leaf_width == 1:
            m[:, f.tree_group[t]] += v.reshape(len(v), -1)[:, 0]
        else:
            m += v
    if f.average_divisor != 1.0:              # averaged forests (sklearn) carry no base
        assert not np.any(f.base_margin)
    return (m + np.asarray(f.base_margin, dtype=np.float64)) / f.average_divisor


@pytest.mark.parametrize("name", gp.CASES)
def test_references_agree(name):
    c = gp.case(name)
    f = c.forest
    F, K = f.n_features, f.n_groups
    for n, seed in gp.sequence(name)[:2] + gp.sequence(name)[6:]:
        X = gp.batch(name, n, seed)
        margin = gp.want(name, OUT_MARGIN, n, seed)
        for xt in (np.float32, np.float64):
            Xc = X.astype(xt)
            assert np.array_equal(canon_eval.predict(f, Xc, OUT_LEAF), gp.want(name, OUT_LEAF, n, seed))
            assert np.array_equal(canon_eval.predict(f, Xc, OUT_MARGIN), margin)
        pred = gp.want(name, OUT_PREDICT, n, seed)
        canon = canon_eval.predict(f, X.astype(np.float32 if f.accum_dtype == TI_F32 else np.float64),
                                   OUT_PREDICT)
        if pred.ndim == 1:
            assert np.array_equal(canon, pred)
        else:
            np.testing.assert_allclose(canon, pred, rtol=1e-5)
        # efficiency: the contributions and the bias column sum to the margin,
        # in float64 (the reference leaves' values summed in float64); a
        # float32 forest's own margin is that sum within its float32 rounding
        m64 = _margin64(f, canon_eval.leaves(f, X))
        assert np.abs(m64 - margin).max() <= (1e-9 if f.accum_dtype == TI_F64 else 1e-6)
        for kind in (OUT_CONTRIB, OUT_CONTRIB_APPROX):
            phi = gp.want(name, kind, n, seed).reshape(n, K, F + 1)
            assert np.abs(phi.sum(axis=2) - m64).max() <= 1e-9, (name, kind)


def test_k20_softmax_labels():
    """The argmax twin of k20-sliced: the same margins, labels from them."""
    n, seed = gp.sequence("k20-softmax")[0]
    assert np.array_equal(gp.batch("k20-softmax", n, seed), gp.batch("k20-sliced", n, seed),
                          equal_nan=True)
    m = gp.want("k20-sliced", OUT_MARGIN, n, seed)
    assert np.array_equal(gp.want("k20-softmax", OUT_MARGIN, n, seed), m)
    lab = gp.want("k20-softmax", OUT_PREDICT, n, seed)
    assert lab.shape == (n,) and np.array_equal(lab, np.argmax(m, axis=1))
    assert len(np.unique(lab)) >= 8
