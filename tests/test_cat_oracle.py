"""The references of the categorical rule against each other (CPU only), and
what the fuzz cases of tests/cat_fuzz_cases.py cover.

Three statements of XGBoost's rule exist: the hand-computed answers of the
``KA`` fixture, ``walk_doc`` (a scalar walk over the JSON document) and the
vectorised oracle/xgb_ref.py (integer sets from the writers' raw trees).  They
share no code and must agree bit for bit; tests/canon_eval.py, the evaluator
of the ABI's canonical forest, must give the same leaves on what the loader
made of the document -- whole, and cut by ``Forest.tree_subset``.
"""
import json
import os

import numpy as np
import pytest

from kfserving_amd.forest import NODE_CATEGORICAL, OUT_LEAF
from kfserving_amd.formats import load_xgboost_model
from kfserving_amd.formats import xgboost_format as xf
from oracle import xgb_ref
from tests import canon_eval
from tests import cat_fuzz_cases as cases
from tests.test_xgb_categorical_format import KA_FILE, KA_LEAF, KA_MARGIN, KA_X, walk_doc

WALK_SEEDS = list(range(0, 32, 3))      # eleven forests for the scalar walk
WALK_BLOCK = 9                          # their 257-row block: every edge value, in seconds


def raw_trees_of_doc(doc):
    """The writers' raw trees (RegTree arrays and ``cats``) of a JSON model
    document, for xgb_ref.from_raw_trees."""
    model = doc["learner"]["gradient_booster"]["model"]
    trees = []
    for jt in model["trees"]:
        dl = np.array(jt["default_left"], dtype=np.uint32)
        cats = {}
        for i, node in enumerate(jt.get("categories_nodes", [])):
            b = jt["categories_segments"][i]
            cats[int(node)] = jt["categories"][b:b + jt["categories_sizes"][i]]
        trees.append({"cleft": np.array(jt["left_children"]), "cright": np.array(jt["right_children"]),
                      "sindex": np.array(jt["split_indices"], dtype=np.uint32) | (dl << 31),
                      "value": np.array(jt["split_conditions"], dtype=np.float32), "cats": cats})
    return trees, model["tree_info"]


def _margins(ref, X, K):
    return np.asarray(xgb_ref.predict(ref, X, output_margin=True)).reshape(X.shape[0], K)


def test_xgb_ref_on_the_known_answers(golden):
    with open(os.path.join(golden, KA_FILE)) as fh:
        doc = json.load(fh)
    trees, ti = raw_trees_of_doc(doc)
    ref = xgb_ref.from_raw_trees(trees, ti, 1, 0, 0.5, "reg:squarederror", major_version=2)
    leaf, margin = walk_doc(doc, KA_X)
    assert np.array_equal(xgb_ref.leaf_index(ref, KA_X), KA_LEAF)
    assert np.array_equal(xgb_ref.leaf_index(ref, KA_X), leaf)
    assert np.array_equal(_margins(ref, KA_X, 1)[:, 0], KA_MARGIN)
    assert np.array_equal(_margins(ref, KA_X, 1), margin)
    f = load_xgboost_model(os.path.join(golden, KA_FILE))
    assert np.array_equal(canon_eval.predict(f, KA_X, OUT_LEAF), KA_LEAF)


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_xgb_ref_equals_walk_doc(seed):
    c = cases.xgb_case(seed)
    X, want_leaf, want_margin, _, _ = c.want()[WALK_BLOCK]
    assert X.shape[0] <= 300
    leaf, margin = walk_doc(c.doc, X)
    assert np.array_equal(want_leaf, leaf), c.desc
    assert want_margin.dtype == np.float32 and np.array_equal(want_margin, margin), c.desc
    # the document's own trees give the same reference as the writers' input
    trees, ti = raw_trees_of_doc(c.doc)
    again = xgb_ref.from_raw_trees(trees, ti, c.F, 0 if c.K == 1 else c.K, 0.5, c.objective,
                                   major_version=2)
    assert np.array_equal(xgb_ref.leaf_index(again, X), leaf), c.desc
    assert np.array_equal(canon_eval.predict(c.forest, X, OUT_LEAF), leaf), c.desc


@pytest.mark.parametrize("seed", cases.XGB_SEEDS)
def test_canon_eval_equals_xgb_ref(seed):
    c = cases.xgb_case(seed)
    X, leaf, _, _, _ = c.want()[-1]         # the largest block
    assert np.array_equal(canon_eval.predict(c.forest, X, OUT_LEAF), leaf), (c.desc, X.shape)


def _subset_ranges(T):
    if T <= 9:
        return [(a, b) for a in range(T) for b in range(a + 1, T + 1)]
    cuts = sorted({1, 7, 8, 9, 13, T // 2, T - 1})
    return ([(t, t + 1) for t in range(T)] + [(0, m) for m in cuts] + [(m, T) for m in cuts] +
            [(3, 13), (8, 16), (5, T - 2)])


def _subset_forests(golden):
    yield "ka", load_xgboost_model(os.path.join(golden, KA_FILE)), KA_X
    for seed in WALK_SEEDS:
        c = cases.xgb_case(seed)
        yield c.desc, c.forest, c.rows[WALK_BLOCK]
    for seed in cases.LGB_SEEDS:
        c = cases.lgb_case(seed)
        yield c.desc, c.forest, c.rows[WALK_BLOCK].astype(np.float64)


def test_tree_subsets_keep_their_bitsets(golden):
    """tree_subset cuts cat_offset / cat_nwords and keeps cat_bits whole: the
    leaves of trees [t0, t1) alone are columns [t0:t1] of the whole forest's."""
    for desc, f, X in _subset_forests(golden):
        assert f.has_categorical
        whole = canon_eval.predict(f, X, OUT_LEAF)
        for t0, t1 in _subset_ranges(f.n_trees):
            sub = f.tree_subset(t0, t1)
            sub.validate()
            assert sub.cat_bits is f.cat_bits
            assert np.array_equal(canon_eval.predict(sub, X, OUT_LEAF), whole[:, t0:t1]), \
                (desc, t0, t1)


# ------------------------------------------------------------- what they cover
def _coverage(c, extra=(), zero_fill=False):
    """``zero_fill``: LightGBM's predictor reads |x| <= 1e-35 as +0.0 before
    any node sees it, so that is the value its reference reports."""
    values, left = [], []
    for _, _, _, _, trace in c.want():
        v, g = cases.decided(trace)
        values.append(v)
        left.append(g)
    values, left = np.concatenate(values), np.concatenate(left)
    want = cases.edge_values(c.nw) + list(extra)
    if zero_fill:
        want = [0.0 if abs(v) <= 1e-35 else v for v in want]
    missing = [v for v in want if not cases.holds(values, v)]
    assert not missing, (c.desc, missing)
    assert left.any() and not left.all(), c.desc


@pytest.mark.parametrize("seed", cases.XGB_SEEDS)
def test_xgb_cases_decide_every_edge_value_at_a_categorical_node(seed):
    """From the reference alone: every edge value reaches a categorical node
    in every case, and categorical nodes send rows both ways."""
    c = cases.xgb_case(seed)
    assert 0 in c.trees[0]["cats"]
    assert int(c.trees[0]["sindex"][0]) & 0x7FFFFFFF in c.cat_features
    assert int(np.max(c.trees[0]["cats"][0])) == 32 * c.nw - 1     # bit 31 of the last word
    _coverage(c)
    # the value one past the longest bitset and its last member meet a node of
    # that many words, and go opposite ways there
    X, _, _, _, trace = c.want()[-1]
    nodes_nw = {(t, int(n)): int(np.max(s)) // 32 + 1
                for t, tr in enumerate(c.trees) for n, s in tr.get("cats", {}).items()}
    seen = {}
    for t, _, nodes, vals, went_left in trace:
        for n, v, g in zip(nodes, vals, went_left):
            if nodes_nw[t, int(n)] == c.nw and v in (32.0 * c.nw - 1, 32.0 * c.nw):
                seen.setdefault(float(v), set()).add(bool(g))
    assert seen.get(32.0 * c.nw) == {True}, (c.desc, seen)         # not a member: left
    assert False in seen.get(32.0 * c.nw - 1, ()), (c.desc, seen)  # a member somewhere: right


@pytest.mark.parametrize("seed", cases.LGB_SEEDS)
def test_lgb_cases_decide_every_edge_value_at_a_categorical_node(seed):
    c = cases.lgb_case(seed)
    assert int(c.trees[0]["decision_type"][0]) & 1
    _coverage(c, cases.LGB_EXTRA, zero_fill=True)


def test_cases_take_every_shape():
    """Each value of the issue's ranges occurs, and so does each edge set."""
    xs = [cases.xgb_case(s) for s in cases.XGB_SEEDS]
    assert {c.depth for c in xs} == set(cases.DEPTHS)
    assert {c.K for c in xs} == set(cases.GROUPS)
    assert {c.F for c in xs} == set(cases.FEATURES)
    assert {c.ncat for c in xs} == set(cases.CATEGORIES)
    assert {c.T // c.K for c in xs} == set(cases.TREES)
    assert all(c.T <= cases.MAX_TREES and c.rows[-1].shape[0] <= 2100 for c in xs)
    assert max(c.nw for c in xs) >= 256          # nwords past 8 bits
    for c in xs:
        # the roots of the first five trees hold the five edge sets, in order
        for i, want in enumerate(xf.edge_category_sets(c.ncat)[:c.T]):
            assert np.array_equal(c.trees[i]["cats"][0], want), (c.desc, i)
        ncat = int(np.count_nonzero((c.forest.flags & NODE_CATEGORICAL) != 0))
        assert ncat == len(c.sets)
        # tiles of 64, 128 and 256 rows without NaN beside tiles with NaN
        big = np.isnan(c.rows[-1]).any(axis=1)
        assert big[:64].any() and big[:256].any() and big[512:576].any()
        assert not big[64:128].any() and not big[256:512].any() and not big[576:640].any()
    ls = [cases.lgb_case(s) for s in cases.LGB_SEEDS]
    assert {c.mts for c in ls} == set(cases.LGB_MISSING)
    assert {c.K for c in ls} == set(cases.LGB_GROUPS)
    assert {c.ncat for c in ls} == set(cases.LGB_CATEGORIES)
    assert all(int(c.forest.depths().max()) <= 8 for c in ls)
