"""The fixed walk's trimmed stage loop (treeinfer_kernels.h bheap_fix_kernel:
the unguarded full stages and the guarded last ones, the forest read through
a buffer resource, level 0 as an arithmetic select on rank - bin), bit for
bit against the oracle's C port (oracle.port.xgb_predict, margins).

What can go wrong sits at the forest's end and at level 0, so the forests
are small: 1 .. 9 depth-8 trees of 28 features (4 trees a stage: no full
stage, one, two, and each with a short one behind it), with one output group
(the peeled loop) and with three (the multiclass kernels, which keep the one
guarded loop), on u16 and on u8 bins.  Rows: every threshold of the forest --
the roots' among them, which level 0 compares, and the first-level keys of
each feature's 5-ary search table -- with one ulp either side, +-0, +-inf,
NaN, denormals and +-FLT_MAX.  The first 512-row tile holds no NaN and the
second does, so one launch runs both instantiations of the stage.
"""
import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest
from kfserving_amd.forest import OUT_MARGIN
from kfserving_amd.formats import xgboost_format as xf
from oracle import port

pytestmark = pytest.mark.gpu

BHEAP = 3
F = 28
f32 = np.float32
FLT_MAX = np.finfo(f32).max
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, -1.4e-45,
                     FLT_MAX, -FLT_MAX], dtype=f32)
COUNTS = [1, 2, 3, 4, 5, 7, 8, 9]


def _around(v):
    v = np.asarray(v, dtype=f32)
    return np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))])


def _thresholds(trees):
    """Per feature the sorted distinct float32 thresholds of the trees."""
    feat, val = [], []
    for t in trees:
        n_int = int((t["cleft"] >= 0).sum())
        feat.append(t["sindex"][:n_int] & 0x7FFFFFFF)
        val.append(t["value"][:n_int])
    feat, val = np.concatenate(feat), np.concatenate(val)
    return [np.unique(val[feat == f]) for f in range(F)]


def _first_level_keys(thr):
    """The 4 keys of node 0 of each feature's 5-ary table: a complete 5-ary
    tree of the smallest height H with 5^H - 1 >= the largest threshold count,
    filled in order, so key c of the top node is the sorted threshold at
    (c + 1) 5^(H-1) - 1 (+inf past the end: no probe)."""
    m = max(len(d) for d in thr)
    p = 5
    while p - 1 < m:
        p *= 5
    return [d[[i for i in ((c + 1) * (p // 5) - 1 for c in range(4)) if i < len(d)]] for d in thr]


def _probe_rows(trees, seed, every=1, tail=0):
    """[rows, F] float32.  Column f holds, at seeded rows, the specials and,
    each with one ulp either side: the thresholds of the roots that test f,
    the first-level keys of f's 5-ary table, every `every`-th of f's sorted
    thresholds and its last `tail` ones; N(0,1) elsewhere.  Whole 512-row
    tiles plus one row, two tiles at least.  Tile 0 holds no NaN; tile 1 does."""
    thr = _thresholds(trees)
    keys = _first_level_keys(thr)
    cols = []
    for f in range(F):
        roots = [t["value"][0] for t in trees if (t["sindex"][0] & 0x7FFFFFFF) == f]
        d = thr[f]
        pick = np.concatenate([d[::every], d[len(d) - min(tail, len(d)):], keys[f],
                               np.asarray(roots, dtype=f32)])
        cols.append(np.concatenate([SPECIALS, _around(np.unique(pick))]).astype(f32))
    rows = max(1025, 512 * -(-max(len(p) for p in cols) // 512) + 1)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, F)).astype(f32)
    for f, p in enumerate(cols):
        X[rng.permutation(rows)[:len(p)], f] = p
    tile0 = X[:512]
    tile0[np.isnan(tile0)] = 0.25
    X[600, 3] = np.nan
    return X


def _pool(max_bin):
    """9 depth-8 trees.  u16 bins: every node of tree 0 tests feature 0, so any
    prefix of the pool has 255 thresholds (> 253) on it.  u8 bins: thresholds
    on the 253 bounds of max_bin = 254."""
    trees, _ = xf.synthetic_complete_trees(9, 8, F, seed=91, max_bin=max_bin)
    if not max_bin:
        s = trees[0]["sindex"]
        n_int = int((trees[0]["cleft"] >= 0).sum())
        s[:n_int] &= np.uint32(0x80000000)   # feature 0, the default-left bit kept
    return trees


_cache = {}


def _pool_and_rows(bits):
    if bits not in _cache:
        trees = _pool(0 if bits == 16 else 254)
        _cache[bits] = (trees, _probe_rows(trees, seed=bits))
    return _cache[bits]


def _forest(trees, groups):
    ti = (np.arange(len(trees)) % groups).astype(np.int32)
    if groups == 1:
        return ti, xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    return ti, xf.forest_from_raw_trees(trees, ti, F, groups, 0.0, "multi:softprob")


def _check(trees, groups, X, bits, row_counts=None):
    ti, forest = _forest(trees, groups)
    want = port.xgb_predict(trees, ti, groups, 0.0, F, X)
    dev = DeviceForest(forest, [0])
    try:
        inf = dev.info()
        assert inf["layout"] == BHEAP and inf["walk"] == 2 and inf["bin_bits"] == bits, inf
        for rows in row_counts or [X.shape[0]]:
            got = np.asarray(dev.predict(X[:rows], OUT_MARGIN)).reshape(rows, groups)
            assert np.array_equal(got, want[:rows]), (len(trees), groups, rows)
    finally:
        dev.close()


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", COUNTS)
def test_tree_counts(n_trees, bits, groups):
    """The forest's end: no full stage, the last full stage with a clamped
    prefetch, a short stage behind it; both tiles of the mix in one launch."""
    trees, X = _pool_and_rows(bits)
    _check(trees[:n_trees], groups, X, bits)


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
def test_row_counts(bits, groups):
    """A partial tile and the lane clamp: 1, 511, 512, 513 and 1025 rows."""
    trees, X = _pool_and_rows(bits)
    _check(trees, groups, X, bits, row_counts=[1, 511, 512, 513, 1025])


def test_ranks_in_the_top_half_of_16_bits():
    """132 depth-8 trees that split on feature 0 alone: more than 32,768
    distinct thresholds on it, so ranks and bins reach the top half of the
    16-bit range (the sign of rank - bin must still be rank < bin).  The
    packer keeps the binned heap and u16 bins for it (checked in _check on
    the host's own report)."""
    trees, _ = xf.synthetic_complete_trees(132, 8, F, seed=92)
    for t in trees:
        n_int = int((t["cleft"] >= 0).sum())
        t["sindex"][:n_int] &= np.uint32(0x80000000)
    thr = _thresholds(trees)
    assert len(thr[0]) > 32768 and all(len(d) == 0 for d in thr[1:])
    X = _probe_rows(trees, seed=3, every=16, tail=300)
    _check(trees, 1, X, 16)
