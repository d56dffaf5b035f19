"""Forests, probe rows and the one check of the fixed walk's GPU tests
(tests/test_gpu_fix_floor.py, test_gpu_fix_rotate.py, test_gpu_fix_dma.py):
depth-8 trees of 28 features whose rows sit on every threshold, compared bit
for bit with the oracle's C port (oracle.port.xgb_predict, margins)."""
import numpy as np

from kfserving_amd.engine import TI_F64, DeviceForest, _check, _ptr
from kfserving_amd.forest import OUT_MARGIN
from kfserving_amd.formats import xgboost_format as xf
from oracle import port

BHEAP = 3
F = 28
ROWS = 1025
f32 = np.float32
FLT_MAX = np.finfo(f32).max
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.4e-45, -1.4e-45,
                     FLT_MAX, -FLT_MAX], dtype=f32)

_cache = {}


def _around(v):
    v = np.asarray(v, dtype=f32)
    return np.concatenate([v, np.nextafter(v, f32(np.inf)), np.nextafter(v, f32(-np.inf))])


def thresholds(trees):
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


def probe_rows(trees, seed, every=1, tail=0):
    """[rows, F] float32.  Column f holds, at seeded rows, the specials and,
    each with one ulp either side: the thresholds of the roots that test f,
    the first-level keys of f's 5-ary table, every `every`-th of f's sorted
    thresholds and its last `tail` ones; N(0,1) elsewhere.  Whole 512-row
    tiles plus one row, two tiles at least.  Tile 0 holds no NaN; tile 1 does."""
    thr = thresholds(trees)
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


def _trees(bits, n, seed):
    """n depth-8 trees.  u16 bins: every node of tree 0 tests feature 0, so any
    prefix of the pool has 255 thresholds (> 253) on it.  u8 bins: thresholds
    on the 253 bounds of max_bin = 254."""
    trees, _ = xf.synthetic_complete_trees(n, 8, F, seed=seed, max_bin=0 if bits == 16 else 254)
    if bits == 16:
        n_int = int((trees[0]["cleft"] >= 0).sum())
        trees[0]["sindex"][:n_int] &= np.uint32(0x80000000)   # feature 0, default-left kept
    return trees


def floor_pool(bits):
    """9 trees and probe rows on every one of their thresholds."""
    key = ("floor", bits)
    if key not in _cache:
        trees = _trees(bits, 9, 91)
        _cache[key] = (trees, probe_rows(trees, seed=bits))
    return _cache[key]


def pool(bits, n=17, seed=191):
    """n trees and 1,025 probe rows: tile 0 holds no NaN, tile 1 does, tile 2
    is one row."""
    key = (bits, n, seed)
    if key not in _cache:
        trees = _trees(bits, n, seed)
        # (every 2nd threshold and more of a u16 pool, so the probes fit 1,025 rows)
        X = probe_rows(trees, seed=seed + bits, every=1 if bits == 8 else max(2, n // 8))
        assert X.shape[0] == ROWS and not np.isnan(X[:512]).any() and np.isnan(X[512:1024]).any()
        _cache[key] = (trees, X)
    return _cache[key]


def forest(trees, groups):
    ti = (np.arange(len(trees)) % groups).astype(np.int32)
    if groups == 1:
        return ti, xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    return ti, xf.forest_from_raw_trees(trees, ti, F, groups, 0.0, "multi:softprob")


def _predict_f64(dev, X, groups):
    """Margins of float64 rows handed to the library as float64."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    rows, cols = X.shape
    out = np.empty(rows * groups, dtype=dev.forest.output_dtype(OUT_MARGIN))
    _check(dev._lib, dev._lib.ti_predict(dev._handle, _ptr(X), TI_F64, rows, cols, cols, OUT_MARGIN,
                                         _ptr(out), out.shape[0]))
    return out


def check(trees, groups, X, bits, row_counts=None, f64=False):
    """The forest takes the fixed walk at `bits`-wide bins, and its margins of
    the first `rows` rows of X (all of X by default) are the oracle's bits;
    with f64 also when the rows go to the library as float64."""
    ti, fo = forest(trees, groups)
    want = port.xgb_predict(trees, ti, groups, 0.0, F, X)
    dev = DeviceForest(fo, [0])
    try:
        inf = dev.info()
        assert inf["layout"] == BHEAP and inf["walk"] == 2 and inf["bin_bits"] == bits, inf
        for rows in row_counts or [X.shape[0]]:
            got = np.asarray(dev.predict(X[:rows], OUT_MARGIN)).reshape(rows, groups)
            assert np.array_equal(got, want[:rows]), (len(trees), groups, rows)
            if f64:
                got = _predict_f64(dev, X[:rows], groups).reshape(rows, groups)
                assert np.array_equal(got, want[:rows]), (len(trees), groups, rows, "f64")
    finally:
        dev.close()
