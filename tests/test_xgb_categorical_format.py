"""XGBoost categorical splits: the loader, the writers and the split rule.

No xgboost is importable where these tests run, so the rule (xgboost >= 1.7
``common::Decision`` / ``GetNextNode``) is pinned by hand-computed answers on
a hand-written fixture and by ``walk_doc`` below: a per-row, per-node scalar
walk over the JSON document itself.  ``walk_doc`` reads none of the loader's
arrays, so the loader and the restatement cannot share a mistake.
"""
import json
import math
import os

import numpy as np
import pytest

from kfserving_amd.forest import (NODE_CAT_XGB, NODE_CATEGORICAL, NODE_NAN_LEFT, OUT_LEAF, Forest,
                                  TI_F32)
from kfserving_amd.formats import load_xgboost_model
from kfserving_amd.formats import ubjson
from kfserving_amd.formats import xgboost_format as xf
from kfserving_amd.formats.xgboost_format import XGBoostFormatError, parse_xgboost_bytes
from tests import canon_eval

KA_FILE = "xgb_categorical_ka.json"
INF, NAN = float("inf"), float("nan")
# the fixture: tree 0 = {node 0: C = {1, 3}, default right; leaves 1 (10.0) / 2 (20.0)};
# tree 1 = {node 0: C = {33}, default left; left leaf 1 (1.0); right node 2: x < 33.5 ?
# leaf 3 (2.0) : leaf 4 (4.0)}.  In the set -> right; invalid (x < 0, x >= 2^24) -> left.
# (value, leaf of tree 0, leaf of tree 1), computed by hand:
KA = [
    (0.0, 1, 1), (1.0, 2, 1), (1.9, 2, 1), (2.0, 1, 1), (3.0, 2, 1), (4.0, 1, 1),
    (31.0, 1, 1), (32.0, 1, 1), (33.0, 1, 3), (33.7, 1, 4), (64.0, 1, 1), (1000.0, 1, 1),
    (-0.0, 1, 1), (-0.5, 1, 1), (-1.0, 1, 1),
    (16777215.0, 1, 1), (16777216.0, 1, 1), (3e9, 1, 1), (INF, 1, 1), (-INF, 1, 1),
    (NAN, 2, 1),
]
KA_X = np.array([[v] for v, _, _ in KA], dtype=np.float32)
KA_LEAF = np.array([[a, b] for _, a, b in KA], dtype=np.int32)
_LEAF0 = {1: 10.0, 2: 20.0}
_LEAF1 = {1: 1.0, 3: 2.0, 4: 4.0}
# base_score 0.5 (reg:squarederror: the margin itself) + the two leaves, exact in float32
KA_MARGIN = np.array([0.5 + _LEAF0[a] + _LEAF1[b] for _, a, b in KA], dtype=np.float32)


# ------------------------------------------------------------ the restatement
def _f32(v) -> float:
    return float(np.float32(v))


def walk_doc(doc: dict, X) -> tuple:
    """(leaf node ids [rows, T] int32, margins [rows, K] float32) of the JSON
    model document ``doc`` for rows X, walked one row and one node at a time.

    Numerical node: missing -> default child, else left iff x < condition in
    float32.  Categorical node (split_type 1): missing -> default child; x < 0
    or x >= 2^24 -> left; else right iff trunc(x) is in the node's slice of
    ``categories``.  Margins: float32 sums in tree order per output group,
    started at the base margin (the documents here have version >= 1.4).
    """
    learner = doc["learner"]
    gb = learner["gradient_booster"]
    model = gb["model"] if gb["name"] == "gbtree" else gb["gbtree"]["model"]
    weights = gb.get("weight_drop")
    lmp = learner["learner_model_param"]
    K = max(1, int(lmp["num_class"]))
    objective = learner["objective"]["name"]
    base = float(str(lmp["base_score"]).strip("[]"))
    if objective in ("binary:logistic", "reg:logistic", "binary:logitraw"):
        base = -math.log(1.0 / base - 1.0)
    trees = []
    for jt in model["trees"]:
        sets = {}
        for i, node in enumerate(jt.get("categories_nodes", [])):
            b = jt["categories_segments"][i]
            sets[int(node)] = set(int(c) for c in jt["categories"][b:b + jt["categories_sizes"][i]])
        trees.append((
            [int(v) for v in jt["left_children"]], [int(v) for v in jt["right_children"]],
            [int(v) for v in jt["split_indices"]], [_f32(v) for v in jt["split_conditions"]],
            [int(v) for v in jt["default_left"]],
            [int(v) for v in jt.get("split_type", [0] * len(jt["left_children"]))], sets))
    info = [int(v) for v in model["tree_info"]]
    rows = [[_f32(v) for v in r] for r in np.asarray(X)]
    leaf = np.zeros((len(rows), len(trees)), dtype=np.int32)
    margin = np.zeros((len(rows), K), dtype=np.float32)
    for r, row in enumerate(rows):
        acc = [np.float32(base)] * K
        for t, (lc, rc, feat, cond, dl, st, sets) in enumerate(trees):
            n = 0
            while lc[n] != -1:
                x = row[feat[n]] if feat[n] < len(row) else NAN
                if x != x:
                    go_left = dl[n] != 0
                elif st[n] == 1:
                    if x < 0.0 or x >= 16777216.0:
                        go_left = True
                    else:
                        go_left = int(x) not in sets[n]
                else:
                    go_left = x < cond[n]
                n = lc[n] if go_left else rc[n]
            leaf[r, t] = n
            v = np.float32(cond[n])
            if weights is not None:
                v = v * np.float32(weights[t])
            acc[info[t]] = np.float32(acc[info[t]] + v)
        margin[r] = acc
    return leaf, margin


def forest_walk(f: Forest, X) -> np.ndarray:
    """Leaf ids of the canonical forest (the loader's arrays) on the host: the
    rule as include/treeinfer.h states it (tests/canon_eval.py), for checking
    the loader's output.  Every categorical node must carry XGBoost's rule."""
    cat = (f.feature >= 0) & ((f.flags & NODE_CATEGORICAL) != 0)
    assert np.all((f.flags[cat] & NODE_CAT_XGB) != 0)
    return canon_eval.predict(f, np.asarray(X, dtype=np.float32), OUT_LEAF)


def synthetic_cat_model(n_trees=12, depth=4, n_features=6, seed=3, num_class=0,
                        cat_features=(0, 3), n_categories=70):
    trees, ti = xf.synthetic_complete_trees(n_trees, depth, n_features, seed, num_class=num_class)
    xf.add_categorical_splits(trees, list(cat_features), n_categories, seed + 1)
    return trees, ti


def cat_rows(n, n_features, cat_features, seed, hi=80):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, n_features))
    for j in cat_features:
        X[:, j] = rng.integers(-5, hi, size=n) + rng.choice([0, 0.5, 0.999], size=n)
        X[rng.random(n) < 0.05, j] = np.nan
        X[rng.random(n) < 0.01, j] = 3e9
        X[rng.random(n) < 0.01, j] = 16777216.0
        X[rng.random(n) < 0.01, j] = -0.5
    return X.astype(np.float32)


# ------------------------------------------------------------------- fixture
def test_known_answers_restatement(golden):
    with open(os.path.join(golden, KA_FILE)) as fh:
        doc = json.load(fh)
    leaf, margin = walk_doc(doc, KA_X)
    assert np.array_equal(leaf, KA_LEAF)
    assert np.array_equal(margin[:, 0], KA_MARGIN)


def test_known_answers_loader(golden):
    f = load_xgboost_model(os.path.join(golden, KA_FILE))
    f.validate()
    assert f.has_categorical and f.n_trees == 2 and f.n_features == 1
    assert f.meta["version"] == (2, 0, 0) and f.meta["format"] == "json"
    # {1, 3} -> one word 0b1010; {33} -> two words, bit 1 of the second
    assert f.cat_bits.tolist() == [0b1010, 0, 0b10]
    assert f.cat_offset.tolist() == [0, -1, -1, 1, -1, -1, -1, -1]
    assert f.cat_nwords.tolist() == [1, 0, 0, 2, 0, 0, 0, 0]
    cat = NODE_CATEGORICAL | NODE_CAT_XGB
    assert f.flags.tolist() == [cat, 0, 0, cat | NODE_NAN_LEFT, 0, 0, 0, 0]
    assert f.threshold[0] == 0.0 and f.threshold[3] == 0.0
    assert f.base_margin.tolist() == [0.5] and f.accum_dtype == TI_F32
    assert np.array_equal(forest_walk(f, KA_X), KA_LEAF)


# --------------------------------------------------------- writers and loader
def test_json_and_ubjson_load_the_same_forest(tmp_path):
    trees, ti = synthetic_cat_model(num_class=3)
    assert sum(len(t.get("cats", {})) for t in trees) > 10
    pj, pu = str(tmp_path / "m.json"), str(tmp_path / "m.ubj")
    xf.write_json_model(pj, trees, ti, 6, 3, 0.5, "multi:softprob", version=(2, 0, 0))
    xf.write_ubj_model(pu, trees, ti, 6, 3, 0.5, "multi:softprob", version=(2, 0, 0))
    fj, fu = load_xgboost_model(pj), load_xgboost_model(pu)
    raw = xf.forest_from_raw_trees(trees, ti, 6, 3, 0.5, "multi:softprob", legacy=False)
    assert fu.meta["format"] == "ubj"
    for name in ("tree_offset", "tree_group", "feature", "threshold", "flags", "left", "right",
                 "leaf_id", "leaf_value", "base_margin", "cat_bits", "cat_offset", "cat_nwords",
                 "cover"):
        assert np.array_equal(getattr(fj, name), getattr(fu, name), equal_nan=True), name
        assert np.array_equal(getattr(fj, name), getattr(raw, name), equal_nan=True), name
    fj.validate()
    ncat = int(np.count_nonzero(fj.flags & NODE_CATEGORICAL))
    assert ncat == sum(len(t["cats"]) for t in trees if "cats" in t)
    assert np.all((fj.flags & NODE_CAT_XGB != 0) == (fj.flags & NODE_CATEGORICAL != 0))
    # each bitset just long enough for its highest category
    for t, tr in enumerate(trees):
        for node, codes in tr.get("cats", {}).items():
            g = int(fj.tree_offset[t]) + node
            assert fj.cat_nwords[g] == int(np.max(codes)) // 32 + 1
    # the loader's forest walks as the document does
    with open(pj) as fh:
        doc = json.load(fh)
    X = cat_rows(200, 6, (0, 3), seed=9)
    assert np.array_equal(forest_walk(fj, X), walk_doc(doc, X)[0])


def test_trees_without_cats_write_the_same_bytes(tmp_path):
    trees, ti = xf.synthetic_complete_trees(3, 3, 5, seed=4)
    doc = xf.json_model_doc(trees, ti, 5, 0, 0.5, "binary:logistic")
    for jt in doc["learner"]["gradient_booster"]["model"]["trees"]:
        assert sorted(jt) == ["default_left", "id", "left_children", "right_children",
                              "split_conditions", "split_indices", "sum_hessian", "tree_param"]
    with_cats = [dict(t) for t in trees]
    with_cats[1]["cats"] = {0: [2, 5]}
    d2 = xf.json_model_doc(with_cats, ti, 5, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    t0, t1 = d2["learner"]["gradient_booster"]["model"]["trees"][:2]
    assert "split_type" not in t0
    assert t1["split_type"] == [1] + [0] * 14 and t1["categories"] == [2, 5]
    assert t1["categories_nodes"] == [0] and t1["categories_segments"] == [0]
    assert t1["categories_sizes"] == [2]


def test_dart_scales_categorical_leaves():
    trees, ti = synthetic_cat_model(n_trees=4, depth=3)
    doc = xf.json_model_doc(trees, ti, 6, 0, 0.5, "binary:logistic", version=(2, 0, 0))
    plain = parse_xgboost_bytes(json.dumps(doc).encode())
    gb = doc["learner"]["gradient_booster"]
    w = [0.5, 1.0, 0.25, 2.0]
    doc["learner"]["gradient_booster"] = {"name": "dart", "gbtree": gb, "weight_drop": w}
    dart = parse_xgboost_bytes(json.dumps(doc).encode())
    assert np.array_equal(dart.flags, plain.flags) and np.array_equal(dart.cat_bits, plain.cat_bits)
    for t in range(4):
        s = plain.tree_slice(t)
        want = (plain.leaf_value[s, 0].astype(np.float32) * np.float32(w[t])).astype(np.float64)
        assert np.array_equal(dart.leaf_value[s, 0], want)
    X = cat_rows(50, 6, (0, 3), seed=2)
    leaf, margin = walk_doc(doc, X)
    assert np.array_equal(forest_walk(dart, X), leaf)


def test_add_categorical_splits_is_seeded_and_keeps_other_nodes():
    a, _ = synthetic_cat_model(seed=5)
    b, _ = synthetic_cat_model(seed=5)
    plain, _ = xf.synthetic_complete_trees(12, 4, 6, 5)
    some = 0
    for ta, tb, tp in zip(a, b, plain):
        assert sorted(ta.get("cats", {})) == sorted(tb.get("cats", {}))
        for k in ("cleft", "cright", "sindex", "value"):
            assert np.array_equal(ta[k], tp[k])
        for node, codes in ta.get("cats", {}).items():
            assert np.array_equal(codes, tb["cats"][node]) and len(codes) > 0
            assert ta["cleft"][node] != -1 and (int(ta["sindex"][node]) & 0x7FFFFFFF) in (0, 3)
            assert 0 <= min(codes) and max(codes) < 70
            some += 1
    assert some > 0


# ------------------------------------------------------------------ malformed
def _ka_doc(golden):
    with open(os.path.join(golden, KA_FILE)) as fh:
        return json.load(fh)


def _tree(doc, i):
    return doc["learner"]["gradient_booster"]["model"]["trees"][i]


def _set(key, value, tree=0):
    def change(doc):
        _tree(doc, tree)[key] = value
    return change


def _version(v):
    def change(doc):
        doc["version"] = v
    return change


MALFORMED = {
    "segment past the end": _set("categories_segments", [1]),
    "negative segment": _set("categories_segments", [-1]),
    "size past the end": _set("categories_sizes", [3]),
    "categories_nodes names a numeric node": _set("categories_nodes", [1]),
    "categorical node not named": _set("split_type", [1, 0, 1, 0, 0], tree=1),
    "categories_nodes not increasing": _set("categories_nodes", [0, 0]),
    "node id out of range": _set("categories_nodes", [7]),
    "category >= 2^24": _set("categories", [1, 16777216]),
    "negative category": _set("categories", [-1, 3]),
    "split_type length": _set("split_type", [1, 0]),
    "version 1.6.0": _version([1, 6, 0]),
    "version 1.5.2": _version([1, 5, 2]),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_categorical_models_raise_format_error(golden, case):
    doc = _ka_doc(golden)
    MALFORMED[case](doc)
    with pytest.raises(XGBoostFormatError):
        parse_xgboost_bytes(json.dumps(doc).encode())
    with pytest.raises(XGBoostFormatError):      # the same document as UBJSON
        parse_xgboost_bytes(ubjson.dumps(doc))


def test_old_version_error_names_the_version(golden):
    doc = _ka_doc(golden)
    doc["version"] = [1, 6, 0]
    with pytest.raises(XGBoostFormatError, match=r"1\.6\.0"):
        parse_xgboost_bytes(json.dumps(doc).encode())
    doc["version"] = [1, 7, 0]
    assert parse_xgboost_bytes(json.dumps(doc).encode()).has_categorical


# ----------------------------------------------------------------- base_score
def test_base_score_bracketed():
    trees, ti = xf.synthetic_complete_trees(3, 2, 4, seed=1, num_class=3)
    doc = xf.json_model_doc(trees, ti, 4, 3, 0.5, "multi:softprob", version=(2, 1, 0))
    lmp = doc["learner"]["learner_model_param"]
    plain = parse_xgboost_bytes(json.dumps(doc).encode())
    lmp["base_score"] = "[5E-1]"
    one = parse_xgboost_bytes(json.dumps(doc).encode())
    assert np.array_equal(one.base_margin, plain.base_margin) and one.meta["base_score"] == 0.5
    lmp["base_score"] = "[1E-1,2.5E-1,7E-1]"
    vec = parse_xgboost_bytes(json.dumps(doc).encode())
    assert vec.base_margin.tolist() == [float(np.float32(v)) for v in (0.1, 0.25, 0.7)]
    for bad in ("[1E-1,2E-1]", "[]", "[a]", "[5E-1"):
        lmp["base_score"] = bad
        with pytest.raises(XGBoostFormatError):
            parse_xgboost_bytes(json.dumps(doc).encode())
    # per element through ProbToMargin
    docb = xf.json_model_doc(trees[:1], [0], 4, 0, 0.5, "binary:logistic", version=(2, 1, 0))
    docb["learner"]["learner_model_param"]["base_score"] = "[2.5E-1]"
    fb = parse_xgboost_bytes(json.dumps(docb).encode())
    assert fb.base_margin.tolist() == [float(np.float32(xf.prob_to_margin("binary:logistic", 0.25)))]


# ------------------------------------------------------------------- validate
def test_validate_rejects_cat_xgb_without_categorical(golden):
    f = load_xgboost_model(os.path.join(golden, KA_FILE))
    f.validate()
    f.flags[3] = NODE_CAT_XGB | NODE_NAN_LEFT
    with pytest.raises(ValueError, match="NODE_CAT_XGB"):
        f.validate()
