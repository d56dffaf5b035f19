"""The fixed walk's rotated 4-tree group (treeinfer_kernels.h bheap_fix_stage:
a tree's step is followed by its own next level's reads, the four trees of a
group one step apart), bit for bit against the oracle's C port
(oracle.port.xgb_predict, margins).

The rotation changes the order of a group's instructions in every stage form
-- the unguarded full stages and the guarded last ones, with and without the
NaN check -- so the forests sit at the stage edges: depth 8, 28 features, of
1, 3, 4, 5, 8, 9, 12, 13, 16 and 17 trees (4 trees a stage: no full stage;
one, two and three peeled stages; and a short last stage of 1 tree behind
each, whose clamped trees walk but must not be added).  One output group (the
peeled loop) and three (the multiclass kernels), u16 and u8 bins, the stage of
8 trees (TI_BHEAP_NG=2) for two of the forests.  Rows are
tests/fix_walk_cases.py's: every threshold with one ulp either side and the
specials; 1,025 of them, so tile 0 holds no NaN, tile 1 does and tile 2 is one
row; and 1, 63 and 65 rows (less than a wave, a wave and a lane).  float64 X
goes to the library as it is (it takes the indexed walk) and must give the
same bits.  One case of 40 trees x 3,000 rows puts several workgroups on a
compute unit, each reusing its stage area across ten stages.
"""
import numpy as np
import pytest

from tests import fix_walk_cases as cases
from tests.fix_walk_cases import ROWS, F

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 4, 5, 8, 9, 12, 13, 16, 17]


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", COUNTS)
def test_tree_counts(n_trees, bits, groups):
    """Every stage count and both forms of the last stage, NaN-free and NaN
    tiles in one launch; float64 X beside float32 at the two ends."""
    trees, X = cases.pool(bits)
    cases.check(trees[:n_trees], groups, X[:ROWS], bits, [ROWS], f64=n_trees in (1, 17))


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
def test_row_counts(bits, groups):
    """Partial tiles: 1, 63 and 65 rows (the clamped lanes walk too), the
    last two with the NaN of row 600 at their row 40."""
    trees, X = cases.pool(bits)
    cases.check(trees, groups, X[560:], bits, [1, 63, 65], f64=True)


@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("n_trees", [9, 17])
def test_stage_of_eight_trees(n_trees, bits, groups, monkeypatch):
    """TI_BHEAP_NG=2: two rotated groups a stage (the guarded loop alone for 9
    trees, one peeled stage and two guarded ones for 17)."""
    monkeypatch.setenv("TI_DEV_KNOBS", "1")
    monkeypatch.setenv("TI_BHEAP_NG", "2")
    trees, X = cases.pool(bits)
    cases.check(trees[:n_trees], groups, X[:ROWS], bits, [ROWS])


def test_across_tiles():
    """40 trees x 3,000 rows: six workgroups, several on one compute unit, ten
    stages through each one's stage area."""
    trees, X = cases.pool(16, n=40, seed=192)
    rng = np.random.default_rng(5)
    X = np.concatenate([X[:ROWS], rng.standard_normal((3000 - ROWS, F)).astype(np.float32)])
    X[2900, 7] = np.nan
    cases.check(trees, 1, X, 16, [3000])
