"""The one-group fixed walk's trimmed binning search (treeinfer_kernels.h,
rank_search_kary_regs on stage_bins' register path: the 5-ary search's first
level from scalar loads, the other levels' gathers through a buffer resource
with 32-bit offsets, the count of keys below x as a carry chain), bit for bit
against the oracle's C port (oracle.port.xgb_predict, margins), as
tests/test_gpu_fix_dma.py does.

Shapes: depth-8 forests of 8, 12 and 13 trees (one peeled stage from each
buffer, then the guarded loop with a full and a 1-tree last stage); 513 and
1,025 rows (a full tile plus a one-row tile, and two plus one); a row stride of
28 floats (stage_bins' register path, the trimmed search) and of 29 (its
scalar path, the search as it was); a NaN-free batch and the same batch with
one NaN (a NaN compares false against every key, in both forms of the count);
u16 bins and u8 bins (255 and at most 253 thresholds on the fullest feature:
whichever tables the packer builds for each; bucket tables keep the search
they had).  The rows sit at, and one ulp either side of, each feature's
smallest and largest threshold and the first-level keys of its 5-ary table,
plus +-inf (the scalar first level's edges).  One forest puts more than 32,768
thresholds on a feature, so ranks reach the top half of 16 bits and the search
is 7 levels deep.
"""
import numpy as np
import pytest

from kfserving_amd.engine import TI_F32, DeviceForest, _check, _ptr
from kfserving_amd.forest import OUT_MARGIN
from kfserving_amd.formats import xgboost_format as xf
from oracle import port
from tests import fix_walk_cases as cases
from tests.fix_walk_cases import BHEAP, ROWS, F

pytestmark = pytest.mark.gpu

N_POOL = 13
_cache = {}


def batches(bits):
    """(trees, NaN-free rows, the same rows with one NaN in tile 1): the pool's
    probe rows, with every feature's smallest and largest threshold, one ulp
    either side of each, and +-inf written into tile 0 and tile 1."""
    if bits not in _cache:
        trees, X = cases.pool(bits, n=N_POOL)
        X = X.copy()
        X[np.isnan(X)] = 0.25
        thr = cases.thresholds(trees)
        for f, d in enumerate(thr):
            if len(d) == 0:
                continue
            edge = np.concatenate([cases._around([d[0], d[-1]]), [np.inf, -np.inf]]).astype(np.float32)
            for base in (0, 512):   # rows 8 f .. 8 f + 7 of both tiles
                X[base + 8 * f:base + 8 * f + len(edge), f] = edge
        Xn = X.copy()
        Xn[600, 3] = np.nan
        assert not np.isnan(X).any() and np.isnan(Xn).sum() == 1
        _cache[bits] = (trees, X, Xn)
    return _cache[bits]


def margins(dev, X, ld):
    """Margins of X handed over with a row stride of `ld` floats."""
    rows = X.shape[0]
    if ld > F:
        X = np.concatenate([X, np.full((rows, ld - F), 7.0, np.float32)], axis=1)
    X = np.ascontiguousarray(X, dtype=np.float32)
    out = np.empty(rows, dtype=dev.forest.output_dtype(OUT_MARGIN))
    _check(dev._lib, dev._lib.ti_predict(dev._handle, _ptr(X), TI_F32, rows, ld, ld, OUT_MARGIN,
                                         _ptr(out), out.shape[0]))
    return out.reshape(rows, 1)


def wanted(bits, n_trees):
    """The oracle's margins of both batches, once a forest."""
    key = ("want", bits, n_trees)
    if key not in _cache:
        trees, X, Xn = batches(bits)
        ti, _ = cases.forest(trees[:n_trees], 1)
        _cache[key] = [port.xgb_predict(trees[:n_trees], ti, 1, 0.0, F, b) for b in (X, Xn)]
    return _cache[key]


@pytest.mark.parametrize("tables", ["packer's choice", "5-ary"])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", [8, 12, 13])
def test_forms(n_trees, bits, tables, monkeypatch):
    """Every combination of row count, row stride and NaN content on one
    forest, with the tables the packer chooses and with the 5-ary tables
    forced (the packer's developer knob), so the trimmed search runs whatever
    the bucket rule makes of these thresholds."""
    for k in ("TI_KARY", "TI_BIN_XPF", "TI_BIN_BUCKETS", "TI_DEV_KNOBS"):
        monkeypatch.delenv(k, raising=False)
    if tables == "5-ary":
        monkeypatch.setenv("TI_DEV_KNOBS", "1")
        monkeypatch.setenv("TI_BIN_BUCKETS", "0")
    trees, X, Xn = batches(bits)
    trees = trees[:n_trees]
    _, forest = cases.forest(trees, 1)
    dev = DeviceForest(forest, [0])
    try:
        inf = dev.info()
        assert inf["layout"] == BHEAP and inf["walk"] == 2 and inf["bin_bits"] == bits, inf
        for name, batch, want in zip(("no NaN", "one NaN"), (X, Xn), wanted(bits, n_trees)):
            for rows in (513, ROWS):
                for ld in (F, F + 1):
                    got = margins(dev, batch[:rows], ld)
                    assert np.array_equal(got, want[:rows]), (n_trees, bits, tables, name, rows, ld)
    finally:
        dev.close()


def test_ranks_in_the_top_half_of_16_bits():
    """132 trees that split on feature 0 alone, more than 32,768 thresholds on
    it: the arithmetic level 0 (the sign of rank - bin) with its VGPR masks, on
    rows at the thresholds' ends and every 64th between."""
    trees, _ = xf.synthetic_complete_trees(132, 8, F, seed=93)
    for t in trees:
        n_int = int((t["cleft"] >= 0).sum())
        t["sindex"][:n_int] &= np.uint32(0x80000000)
    thr = cases.thresholds(trees)
    assert len(thr[0]) > 32768 and all(len(d) == 0 for d in thr[1:])
    X = cases.probe_rows(trees, seed=4, every=64, tail=100)
    cases.check(trees, 1, X, 16)
