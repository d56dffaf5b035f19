"""The CatBoost JSON loader: a hand-written model with the raw values worked
out by hand, the refusals, and the expansion's leaf ids."""
import copy
import json

import numpy as np
import pytest

from kfserving_amd.forest import OUT_LEAF, OUT_MARGIN
from kfserving_amd.formats import catboost_format as cf
from tests import canon_eval, catboost_cases

INF, NAN = np.inf, np.nan
F01 = float(np.float32(0.1))   # 0.1 is no float32: the border the model uses is this value


def _doc():
    feat = lambda i, nan: {"flat_feature_index": i, "borders": [0.0], "nan_value_treatment": nan}
    split = lambda f, b: {"float_feature_index": f, "border": b, "split_type": "FloatFeature"}
    return {
        "features_info": {"float_features": [feat(0, "AsIs"), feat(1, "AsFalse"), feat(2, "AsTrue")]},
        "model_info": {"params": {"loss_function": {"type": "RMSE"}}},
        "oblivious_trees": [
            {"splits": [split(0, 0.5), split(2, -1.0)], "leaf_values": [1.0, 2.0, 4.0, 8.0]},
            {"splits": [split(1, 0.1)], "leaf_values": [10.0, 20.0]},
        ],
        "scale_and_bias": [1.0, [100.0]],
    }


#        x0    x1    x2      leaves   raw = 100 + tree 0 + tree 1
HAND = [
    ([0.5, F01, -1.0], [0, 0], 111.0),    # every value on its border: not greater
    ([NAN, NAN, NAN], [2, 0], 114.0),     # AsIs 0, AsFalse 0, AsTrue 1 (bit 1 of tree 0)
    ([INF, INF, INF], [3, 1], 128.0),
    ([-INF, -INF, -INF], [0, 0], 111.0),
    ([0.75, 0.3, -2.0], [1, 1], 122.0),
    ([0.25, 0.1, -0.5], [2, 0], 114.0),   # the double 0.1 is cast onto the border's float32
]


def test_hand_model():
    doc = _doc()
    X = np.array([r[0] for r in HAND], dtype=np.float64)
    leaves = np.array([r[1] for r in HAND])
    raw = np.array([r[2] for r in HAND])
    assert np.array_equal(catboost_cases.leaf_index(doc, X), leaves)
    assert np.array_equal(catboost_cases.raw(doc, X)[:, 0], raw)
    forest = cf.forest_from_catboost_doc(doc)
    assert (forest.n_features, forest.n_trees, forest.leaf_width) == (3, 2, 1)
    X32 = X.astype(np.float32)
    assert np.array_equal(canon_eval.predict(forest, X32, OUT_MARGIN), raw)
    assert np.array_equal(canon_eval.predict(forest, X32, OUT_LEAF), leaves)


@pytest.mark.parametrize("dim,loss", [(1, "Logloss"), (3, "MultiClass")])
def test_expansion_matches_restatement(dim, loss):
    doc = cf.json_model_doc(9, [0, 3, 7, 1, 5, 2, 4, 6, 3], 5, dim=dim, loss=loss, seed=3,
                            leaf_weights=True)
    forest = cf.forest_from_catboost_doc(json.loads(json.dumps(doc)))
    rng = np.random.default_rng(1)
    X = rng.standard_normal((300, 5)).astype(np.float32)
    X[rng.random(X.shape) < 0.1] = np.nan
    X[:5, 0] = doc["features_info"]["float_features"][0]["borders"][:5]
    assert np.array_equal(canon_eval.predict(forest, X, OUT_LEAF), catboost_cases.leaf_index(doc, X))
    want = catboost_cases.raw(doc, X)
    assert np.array_equal(canon_eval.predict(forest, X, OUT_MARGIN), want if dim > 1 else want[:, 0])
    # a node's cover is the sum of the leaf weights below it
    for t, tree in enumerate(doc["oblivious_trees"]):
        assert forest.cover[forest.tree_offset[t]] == sum(tree["leaf_weights"])


def _with(path, value):
    doc = _doc()
    at = doc
    for k in path[:-1]:
        at = at[k]
    at[path[-1]] = value
    return doc


REFUSED = {
    "ctr split": (_with(["oblivious_trees", 0, "splits", 0, "split_type"], "OnlineCtr"), "OnlineCtr"),
    "categorical": (_with(["features_info", "categorical_features"], [{"flat_feature_index": 3}]),
                    "categorical"),
    "ctrs": (_with(["ctrs"], {"x": 1}), "CTR"),
    "scale": (_with(["scale_and_bias"], [2.0, [0.0]]), "scale"),
    "loss": (_with(["model_info", "params", "loss_function", "type"], "YetiRank"), "YetiRank"),
    "node cap": (_with(["oblivious_trees", 0, "splits"],
                       [copy.deepcopy(_doc()["oblivious_trees"][0]["splits"][0])] * 26), "depth 26"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refusals(case):
    doc, word = REFUSED[case]
    with pytest.raises(cf.CatBoostFormatError, match=word):
        cf.forest_from_catboost_doc(doc)


def test_cbm_is_refused(tmp_path):
    p = tmp_path / "model.json"
    p.write_bytes(b"CBM1" + bytes(64))
    with pytest.raises(cf.CatBoostFormatError, match='format="json"'):
        cf.load_catboost_model(str(p))
