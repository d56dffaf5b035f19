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

from kfserving_amd.formats import xgboost_format as xf
from tests import fix_walk_cases as cases

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 4, 5, 7, 8, 9]


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", COUNTS)
def test_tree_counts(n_trees, bits, groups):
    """The forest's end: no full stage, the last full stage with a clamped
    prefetch, a short stage behind it; both tiles of the mix in one launch."""
    trees, X = cases.floor_pool(bits)
    cases.check(trees[:n_trees], groups, X, bits)


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
def test_row_counts(bits, groups):
    """A partial tile and the lane clamp: 1, 511, 512, 513 and 1025 rows."""
    trees, X = cases.floor_pool(bits)
    cases.check(trees, groups, X, bits, row_counts=[1, 511, 512, 513, 1025])


def test_ranks_in_the_top_half_of_16_bits():
    """132 depth-8 trees that split on feature 0 alone: more than 32,768
    distinct thresholds on it, so ranks and bins reach the top half of the
    16-bit range (the sign of rank - bin must still be rank < bin).  The
    packer keeps the binned heap and u16 bins for it (checked in cases.check
    on the host's own report)."""
    trees, _ = xf.synthetic_complete_trees(132, 8, cases.F, seed=92)
    for t in trees:
        n_int = int((t["cleft"] >= 0).sum())
        t["sindex"][:n_int] &= np.uint32(0x80000000)
    thr = cases.thresholds(trees)
    assert len(thr[0]) > 32768 and all(len(d) == 0 for d in thr[1:])
    X = cases.probe_rows(trees, seed=3, every=16, tail=300)
    cases.check(trees, 1, X, 16)
