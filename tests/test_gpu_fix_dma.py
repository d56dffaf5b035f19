"""The fixed walk's two-buffer stage (treeinfer_kernels.h bheap_fix_kernel:
the peeled stages of the one-group kernels alternate between two
LDS buffers that each wave fills by LDS-DMA, one barrier a stage), bit for bit
against the oracle's C port (oracle.port.xgb_predict, margins).

What can go wrong is an order, not an arithmetic: a stage read before its fill
has landed, a buffer refilled while a slower wave still walks it, the
hand-over to the guarded loop's register stage out of either buffer.  So the
forests sit at the loop's edges: depth 8, 28 features, of 7 trees (no
two-buffer loop: 38,912 B of LDS), then 8, 9, 12, 13, 16, 17, 20, 21, 24 and 25
(one to five peeled stages, so the hand-over happens out of the second buffer
and out of the first; from 16 trees on a buffer is refilled; a full and a
1-tree last stage behind each).  Rows are tests/fix_walk_cases.py's
(1,025: tile 0 holds no NaN, tile 1 does, tile 2 is one row).  A row stride of
29 floats sends the binning through the first buffer while stage 0's fill into
the second is in flight.  Three output groups keep the register stage and must
give the bits they gave.
"""
import numpy as np
import pytest

from kfserving_amd.engine import TI_F32, DeviceForest, _check, _ptr
from kfserving_amd.forest import OUT_MARGIN
from oracle import port
from tests import fix_walk_cases as cases
from tests.fix_walk_cases import BHEAP, ROWS, F

pytestmark = pytest.mark.gpu

COUNTS = [7, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25]
N_POOL = 25


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", COUNTS)
def test_tree_counts(n_trees, bits):
    """No two-buffer loop (7), one to five peeled stages, a full and a 1-tree
    last stage; NaN-free and NaN tiles and a one-row tile in one launch."""
    trees, X = cases.pool(bits, n=N_POOL)
    cases.check(trees[:n_trees], 1, X[:ROWS], bits, [ROWS])


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", [17, 21])
def test_unaligned_rows(n_trees, bits):
    """n_cols = row_stride = 29: rows are not 16-byte aligned, so stage_bins
    copies through its temp (the first buffer) while stage 0's fill into the
    second is in flight."""
    trees, X = cases.pool(bits, n=N_POOL)
    trees = trees[:n_trees]
    ti, forest = cases.forest(trees, 1)
    want = port.xgb_predict(trees, ti, 1, 0.0, F, X)
    X29 = np.ascontiguousarray(np.concatenate([X, np.full((ROWS, 1), 7.0, np.float32)], axis=1))
    dev = DeviceForest(forest, [0])
    try:
        inf = dev.info()
        assert inf["layout"] == BHEAP and inf["walk"] == 2 and inf["bin_bits"] == bits, inf
        out = np.empty(ROWS, dtype=dev.forest.output_dtype(OUT_MARGIN))
        _check(dev._lib, dev._lib.ti_predict(dev._handle, _ptr(X29), TI_F32, ROWS, F + 1, F + 1, OUT_MARGIN,
                                             _ptr(out), out.shape[0]))
        assert np.array_equal(out.reshape(ROWS, 1), want), n_trees
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [16, 8])
def test_partial_tiles(bits):
    """1, 63 and 65 rows on 21 trees: the clamped lanes still fill and walk
    (the last two with the NaN of row 600 at their row 40)."""
    trees, X = cases.pool(bits, n=N_POOL)
    cases.check(trees[:21], 1, X[560:], bits, [1, 63, 65])


def test_several_workgroups_on_a_cu():
    """40 trees x 3,000 rows: six workgroups, ten stages through each one's two
    buffers; predicted twice, both outputs compared."""
    trees, X = cases.pool(16, n=40, seed=192)
    rng = np.random.default_rng(5)
    X = np.concatenate([X[:ROWS], rng.standard_normal((3000 - ROWS, F)).astype(np.float32)])
    X[2900, 7] = np.nan
    cases.check(trees, 1, X, 16, [3000, 3000])


def test_two_streams():
    """24 trees, two 1,025-row batches on two streams, both launched before
    either is synchronised (how the headline runs)."""
    import torch
    trees, X = cases.pool(16, n=N_POOL)
    trees = trees[:24]
    ti, forest = cases.forest(trees, 1)
    Xb = [X, np.ascontiguousarray(X[::-1])]
    want = [port.xgb_predict(trees, ti, 1, 0.0, F, x) for x in Xb]
    dev = DeviceForest(forest, [0])
    try:
        inf = dev.info()
        assert inf["layout"] == BHEAP and inf["walk"] == 2, inf
        Xd = [torch.from_numpy(x).cuda() for x in Xb]
        outs = [torch.zeros(ROWS, dtype=torch.float32, device="cuda") for _ in Xb]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for x, o, s in zip(Xd, outs, streams):
            dev.predict_device(x.data_ptr(), TI_F32, ROWS, F, F, OUT_MARGIN, o.data_ptr(), ROWS,
                               slot=0, stream=s.cuda_stream)
        for s in streams:
            s.synchronize()
        for o, w in zip(outs, want):
            assert np.array_equal(o.cpu().numpy().reshape(ROWS, 1), w)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", [8, 17])
def test_three_output_groups(n_trees, bits):
    """The multiclass kernels keep the register stage (38,912 B)."""
    trees, X = cases.pool(bits, n=N_POOL)
    cases.check(trees[:n_trees], 3, X[:ROWS], bits, [ROWS])
