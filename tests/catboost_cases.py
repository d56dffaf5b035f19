"""CatBoost's prediction rule restated in numpy float64, from the JSON document
itself (not from the Forest): the reference of tests/test_catboost_format.py
and tests/test_gpu_catboost.py."""
import numpy as np


def leaf_index(doc, X):
    """[rows, trees] CatBoost leaf indices: bit d = float32(x) > float32(border),
    a NaN's bit 1 only under AsTrue, splits[0] the least significant bit."""
    X = np.asarray(X).astype(np.float32)
    floats = doc["features_info"]["float_features"]
    out = np.zeros((X.shape[0], len(doc["oblivious_trees"])), dtype=np.int32)
    for t, tree in enumerate(doc["oblivious_trees"]):
        for d, s in enumerate(tree["splits"]):
            ff = floats[s["float_feature_index"]]
            x = X[:, ff["flat_feature_index"]]
            bit = x > np.float32(s["border"])
            bit = np.where(np.isnan(x), ff.get("nan_value_treatment", "AsIs") == "AsTrue", bit)
            out[:, t] |= bit.astype(np.int32) << d
    return out


def raw(doc, X):
    """[rows, dim] float64: the trees' leaves summed in tree order, then the bias."""
    leaves = leaf_index(doc, X)
    bias = np.atleast_1d(np.asarray(doc["scale_and_bias"][1], dtype=np.float64))
    dim = len(doc["oblivious_trees"][0]["leaf_values"]) >> len(doc["oblivious_trees"][0]["splits"])
    acc = np.zeros((leaves.shape[0], dim), dtype=np.float64)
    for t, tree in enumerate(doc["oblivious_trees"]):
        acc += np.asarray(tree["leaf_values"], dtype=np.float64).reshape(-1, dim)[leaves[:, t]]
    return acc + bias


def answer(doc, X):
    """The library's probability or value."""
    m = raw(doc, X)
    loss = doc["model_info"]["params"]["loss_function"]["type"]
    if loss in ("Logloss", "CrossEntropy", "MultiClassOneVsAll"):
        return 1.0 / (1.0 + np.exp(-m))
    if loss == "MultiClass":
        e = np.exp(m - m.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return m
