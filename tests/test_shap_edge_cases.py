"""The edge cases of tests/shap_edge_cases.py cannot hide a defect -- shown on
the CPU, from the references alone:

  * every split threshold of every case is met by a row and by the next value
    above it, in both row types, also at nodes whose feature an ancestor split
    on, after a left and after a right turn (the value is then a `hi` and a
    `lo` of a merged path element);
  * each of five wrong split rules (shap_edge_cases.decisions(mutant=)) moves
    at least 4 rows of every case it applies to by more than 100 x the bound
    the GPU is held to on that case, so a kernel with that defect fails
    tests/test_gpu_shap_edges.py;
  * the references agree with each other on these rows (oracle/shap_ref, the
    recursion of tests/shap_cat_eval, brute-force Shapley values; interaction
    rows sum to contributions);
  * the float32 restatement's own error, which sets the float32 bounds, is the
    one written beside the cases.
"""
import numpy as np
import pytest

from kfserving_amd.forest import NODE_ZERO_FLIP, TI_F32
from oracle import shap_ref
from tests import saabas_eval as sa
from tests import shap_cat_eval as sc
from tests import shap_edge_cases as ec
from tests import shap_interact_eval as si

F32_CASES = [n for n in ec.CASES if n.startswith("xgb-")]
REPEATING = ["lgb-mixed-f32thr", "lgb-f64thr", "xgb-d8"]     # a feature comes back on a path


def test_cases_are_what_they_claim():
    for name in ec.CASES:
        f = ec.forest(name)
        assert not f.has_categorical and f.leaf_width == 1
        assert (f.accum_dtype == TI_F32) == (name in F32_CASES)
    for name in REPEATING:
        assert ec.feature_repeats(name), name
    mixed, plain = ec.forest("lgb-mixed-f32thr"), ec.forest("lgb-f64thr")
    assert ec.f32_can_meet(mixed) and not ec.f32_exact_thresholds(plain).any()
    assert np.array_equal(mixed.feature, plain.feature) and np.array_equal(mixed.flags, plain.flags)
    assert np.any(mixed.flags & NODE_ZERO_FLIP) and mixed.lgb_zero_map
    d8 = ec.forest("xgb-d8")
    k = ec.kinds("xgb-d8")
    assert k["max_unique"] == 8
    assert k["paths"] >= 512 and k["paths"] % 2 and k["paths"] % 3, k
    split = d8.feature >= 0
    assert np.isnan(d8.threshold[split]).sum() == 1                 # the -inf split value
    assert (d8.threshold[split] == ec.FLT_MAX).sum() == 1           # the +inf one
    for n in ec.CHAINS_XGB:
        assert ec.max_unique(f"xgb-chain-{n}") == n == ec.forest(f"xgb-chain-{n}").n_features
        assert ec.forest(f"xgb-chain-{n}").n_trees == 3
    for n in ec.CHAINS_LGB:
        assert ec.max_unique(f"lgb-chain-{n}") == n == ec.forest(f"lgb-chain-{n}").n_features
    assert [ec.maxn(f"lgb-chain-{n}") for n in ec.CHAINS_LGB] == [8, 16, 16, 32, 32, 0]
    assert [ec.maxn(f"xgb-chain-{n}") for n in ec.CHAINS_XGB] == [16, 16, 32, 32, 0]
    assert ec.maxn("xgb-d8") == 8
    assert (ec.width("w128"), ec.width("w129")) == (128, 129)
    assert ec.takes_register_kernel("w128") and not ec.takes_register_kernel("w129")
    sk = ec.forest("sk-rf")
    assert sk.average_divisor == 4.0 and not ec.f32_can_meet(sk)


def test_rows_are_what_they_claim():
    for name in ("lgb-mixed-f32thr", "xgb-chain-17", "w129"):
        f = ec.forest(name)
        for variant, dtype in (("x32", np.float32), ("x64", np.float64)):
            X = ec.rows(name, variant)
            assert X.shape == (ec.ROWS, f.n_features) and X.dtype == dtype
            assert np.all(np.isneginf(X[0])) and np.all(np.isposinf(X[1])) and np.all(np.isnan(X[2]))
            assert not X[3].any() and np.all(np.signbit(X[3]))
            body = X[4:].astype(np.float64)
            for v in ec.specials(dtype):
                v = float(dtype(v))
                hit = np.isnan(body) if np.isnan(v) else (body == v) & (np.signbit(body) == np.signbit(v))
                assert hit.any(), (name, variant, v)
            special = ec.specials(dtype).astype(dtype).astype(np.float64)
            share = np.isin(body, special).mean() + np.isnan(body).mean()
            assert 0.2 <= share <= 0.3, share
        assert ec.rows(name, "x64-short").shape == (ec.ROWS, f.n_features - 2)
    assert ec.rows("xgb-d8", "x32-stride") is ec.rows("xgb-d8", "x32")


def _met(name, variant):
    """Per numerical node: rows whose value on the node's feature is the
    node's on-threshold value, and rows on the next value above."""
    f = ec.forest(name)
    X = ec.rows(name, variant).astype(np.float64)
    nodes = ec.numerical_nodes(f)
    on, above = ec.on_threshold_values(f.threshold[nodes], np.float64 if variant == "x64" else np.float32)
    x = X[:, f.feature[nodes]]
    return f, nodes, x == on[None, :], x == above[None, :]


@pytest.mark.parametrize("variant", ec.XDTYPES)
@pytest.mark.parametrize("name", ec.CASES)
def test_every_threshold_is_met(name, variant):
    """Every numerical node with a finite threshold has a row on the largest
    value of the row type that turns left and one on the next value, which
    turns right.  For float64 rows, and for float32 rows of forests whose
    thresholds float32 holds, the first is the threshold itself."""
    f, nodes, on, above = _met(name, variant)
    assert nodes.size
    assert on.any(axis=0).all(), f"{(~on.any(axis=0)).sum()} of {nodes.size} thresholds not met"
    assert above.any(axis=0).all(), f"{(~above.any(axis=0)).sum()} of {nodes.size} not met from above"
    left = ec.decisions(f, ec.rows(name, variant))
    assert left[:, nodes][on].all() and not left[:, nodes][above].any()
    if variant == "x32" and name == "lgb-f64thr":
        assert not ec.f32_exact_thresholds(f).any()      # no float32 equals a threshold


def _ancestor_turns(f):
    """node -> set of turns (True: left) taken at ancestors of the same feature."""
    turns = {}
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        stack = [(0, ())]
        while stack:
            v, path = stack.pop()
            g = b + v
            if f.feature[g] < 0:
                continue
            fe = int(f.feature[g])
            turns[g] = {turn for a, turn in path if a == fe}
            stack.append((int(f.left[g]), path + ((fe, True),)))
            stack.append((int(f.right[g]), path + ((fe, False),)))
    return turns


def _reached(f, left):
    """[rows, N] bool: the nodes each row's own walk visits."""
    out = np.zeros(left.shape, dtype=bool)
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        node = np.zeros(left.shape[0], dtype=np.int64)
        live = np.ones(left.shape[0], dtype=bool)
        while live.any():
            g = b + node
            out[live, g[live]] = True
            live = live & (f.feature[g] >= 0)
            node = np.where(live, np.where(left[np.arange(len(g)), g], f.left[g], f.right[g]), node)
    return out


@pytest.mark.parametrize("name,variant", [(n, v) for n in REPEATING for v in ec.XDTYPES
                                          if not (n == "lgb-f64thr" and v == "x32")])
def test_thresholds_are_met_under_an_ancestor_of_the_same_feature(name, variant):
    """Some rows sit on the threshold of a node they themselves reach after a
    left turn, and some after a right turn, on the node's own feature: the
    value is then the `hi` of an element that has a `lo`, and the `lo` of one
    that has a `hi`."""
    f, nodes, on, _ = _met(name, variant)
    turns = _ancestor_turns(f)
    reached = _reached(f, ec.decisions(f, ec.rows(name, variant)))[:, nodes]
    after_left = np.array([True in turns[g] for g in nodes])
    after_right = np.array([False in turns[g] for g in nodes])
    n_left = int((on & reached)[:, after_left].sum())
    n_right = int((on & reached)[:, after_right].sum())
    print(f"{name} {variant}: on-threshold (row, node) pairs reached after a left turn {n_left}, "
          f"after a right turn {n_right}")
    assert n_left >= 1 and n_right >= 1


def _moved(name, variant, mutant):
    """(rows whose decisions the mutant changes, of which the number that
    move by more than 100 x the case's device bound; counting stops at 8)."""
    f = ec.forest(name)
    X = ec.rows(name, variant)
    base = ec.decisions(f, X)
    wrong = ec.decisions(f, X, mutant=mutant)
    differ = np.nonzero((base != wrong).any(axis=1))[0]
    want = ec.want_contrib(name, variant)
    need = 100 * ec.bound(name)
    moved = 0
    for r in differ:
        got = ec.contributions_from(f, wrong[r:r + 1], 1)
        if sa.scaled_error(got, want[r:r + 1]) > need:
            moved += 1
            if moved == 8:
                break
    return differ.size, moved


_APPLIES = [(n, v, m) for n in ec.CASES for v in ec.XDTYPES for m in ec.MUTANTS
            if ec.mutant_applies(n, v, m)]


@pytest.mark.parametrize("name,variant,mutant", _APPLIES)
def test_every_mutant_shows(name, variant, mutant):
    differ, moved = _moved(name, variant, mutant)
    print(f"{name} {variant} {mutant}: {differ} rows decide differently, {moved}{'+' if moved == 8 else ''} "
          f"move by more than {100 * ec.bound(name):g}")
    assert moved >= 4


def test_mutants_apply_wherever_they_can_change_a_decision():
    """A mutant is left out of a case only where it changes no decision: the
    zero mutants in forests without a zero flag, `strict` on float32 rows of
    forests none of whose thresholds float32 holds."""
    left_out = [(n, v, m) for n in ec.CASES for v in ec.XDTYPES for m in ec.MUTANTS
                if (n, v, m) not in _APPLIES]
    assert left_out and {m for _, _, m in left_out} == {"strict", "no_zero_flip", "no_zero_map"}
    for name, variant, mutant in left_out:
        f = ec.forest(name)
        if mutant == "strict" and ec.f32_exact_thresholds(f).any():
            assert name == "sk-rf"          # a few of its midpoints are float32 values
            continue
        X = ec.rows(name, variant)
        assert np.array_equal(ec.decisions(f, X, mutant=mutant), ec.decisions(f, X)), (name, variant, mutant)
    for name in ec.CASES:
        for variant in ec.XDTYPES:
            assert ec.mutant_applies(name, variant, "drop_neg_inf")
            assert ec.mutant_applies(name, variant, "nan_inverted")


@pytest.mark.parametrize("name", ec.CASES)
def test_decisions_restate_the_canonical_rule(name):
    f = ec.forest(name)
    for variant in ("x32", "x64", "x64-short"):
        X = ec.rows(name, variant)
        assert np.array_equal(ec.decisions(f, X), sc.decisions(f, X))


RESTATED_ROWS = 24      # rows 0..3 are the all-special ones; the rest hold every kind of value


@pytest.mark.parametrize("name", ec.CASES)
def test_the_two_restatements_agree(name):
    f = ec.forest(name)
    for variant in ec.XDTYPES:
        X = ec.rows(name, variant)[:RESTATED_ROWS]
        got = shap_ref.contributions(f, X.astype(np.float64))
        assert np.abs(got - ec.want_contrib(name, variant)[:RESTATED_ROWS]).max() <= 1e-12


@pytest.mark.parametrize("variant", ["x32", "x64", "x64-short"])
def test_brute_force_pins_both_on_edge_rows(variant):
    name = "lgb-mixed-f32thr"
    f = ec.forest(name)
    assert f.n_features <= 5
    X = ec.rows(name, variant)
    want = ec.want_contrib(name, variant)
    for r in range(RESTATED_ROWS):
        x = np.full(f.n_features, np.nan)
        x[:X.shape[1]] = X[r]
        bf = sc.brute_force(f, x)
        assert np.abs(bf - want[r]).max() <= 1e-12, r
        assert np.abs(bf - shap_ref.brute_force(f, x)).max() <= 1e-12, r


@pytest.mark.parametrize("name", [n for n in ec.CASES if ec.takes_interactions(n)])
def test_interactions_are_consistent_with_contributions(name):
    f = ec.forest(name)
    F, K = f.n_features, f.n_groups
    m = ec.want_interact(name, "x64")
    c = ec.want_contrib(name, "x64")[:ec.INTERACT_ROWS].reshape(-1, K, F + 1)
    assert si.scaled_error(m.sum(axis=3), c) <= 1e-12
    # the reference's own asymmetry: rounding on paths of up to 20 elements, and
    # 5e-12 on the 32-element chains, whose unwound sums cancel even in float64
    asym = si.scaled_error(m, np.swapaxes(m, 2, 3))
    print(f"{name}: asymmetry of the float64 reference {asym:.3g}")
    assert asym <= (1e-12 if ec.max_unique(name) <= 20 else 1e-10)


def test_approximate_contributions_sum_to_the_exact_ones():
    """Saabas values and TreeSHAP values split the same margin."""
    for name in ("lgb-mixed-f32thr", "xgb-d8", "lgb-chain-17"):
        f = ec.forest(name)
        a = ec.want_approx(name, "x64").reshape(ec.ROWS, f.n_groups, -1).sum(axis=2)
        c = ec.want_contrib(name, "x64").reshape(ec.ROWS, f.n_groups, -1).sum(axis=2)
        assert np.abs(a - c).max() <= 1e-12 * max(1.0, np.abs(c).max())


@pytest.mark.parametrize("name", F32_CASES)
def test_float32_restatement_error_is_the_recorded_one(name):
    err = ec.f32_cpu_error(name)
    rec = ec.F32_CPU_ERROR[name]
    print(f"{name}: float32 restatement vs float64, max scaled error {err:.3g} (recorded {rec:.3g}); "
          f"device bound {ec.bound(name):g}")
    assert rec / 2 <= err <= rec * 2
    assert ec.bound(name) <= 1e-5


def test_between_rows_lie_between_two_float32():
    f = ec.forest("xgb-d8")
    X = ec.between_rows()
    assert X.dtype == np.float64
    inexact = X.astype(np.float32).astype(np.float64) != X
    assert inexact[4:].mean() > 0.3
    # the float64 rule sends them right where the float32 below them turns left
    with np.errstate(over="ignore"):
        below = np.nextafter(X.astype(np.float32), np.float32(-np.inf)).astype(np.float64)
    down = ec.decisions(f, below)
    assert (ec.decisions(f, X) != down).any(axis=1).sum() >= ec.ROWS // 2
