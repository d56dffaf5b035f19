"""CatBoost's JSON export (``model.save_model(path, format="json")``) as a Forest.

No catboost package is needed, so what follows is the specification this
loader implements; a document outside it raises :class:`CatBoostFormatError`.

Features.  ``features_info.float_features[i]`` carries ``flat_feature_index``
(the input column), ``borders`` and ``nan_value_treatment`` (``AsIs``,
``AsFalse`` or ``AsTrue``).  A non-empty ``features_info.categorical_features``,
any ``ctrs`` and any split whose ``split_type`` is not ``FloatFeature`` are
refused: CTR and one-hot splits need CatBoost's string hashing.

Trees.  ``oblivious_trees[t].splits[d]`` carries ``float_feature_index`` and
``border``; every node of level d tests that one split.  ``leaf_values`` holds
``2^D * dim`` values leaf-major (``leaf_values[leaf * dim + k]``); a tree may
have no split at all.

Rule.  Inputs are float32, as CatBoost's pool stores them:
``bit_d = float32(x) > float32(border)``; for a NaN the bit is 1 under
``AsTrue`` and 0 under ``AsFalse`` / ``AsIs``; ``leaf = sum(bit_d << d)``,
``splits[0]`` the least significant bit.

Accumulation.  ``raw[k] = scale * (sum over trees, in tree order, float64) +
bias[k]`` from ``scale_and_bias = [scale, [bias...]]``; ``scale != 1`` is
refused (folding it into the leaves would change the rounding).

Answer, from ``model_info.params.loss_function.type``: ``Logloss`` /
``CrossEntropy`` sigmoid, ``MultiClass`` softmax, ``MultiClassOneVsAll`` sigmoid
per class, ``RMSE`` / ``MAE`` / ``Quantile`` / ``MAPE`` / ``Huber`` /
``LogCosh`` identity; any other loss is refused by name.

Canonical encoding.  ``left iff x <= threshold`` with ``threshold =
float32(border)`` is the rule above, NAN_LEFT set unless the treatment is
``AsTrue``.  Each tree is expanded to a complete tree of explicit nodes in
heap order whose root tests the *last* split, so the leaves left to right are
``leaf_values`` in order and ``leaf_id`` is CatBoost's own leaf index;
``leaf_width = dim``, float64 sums, the bias added after the sum.  The library
recognises the expansion as oblivious when it packs it (layout 12).  A model
whose expansion exceeds 2^26 nodes is refused.  ``leaf_weights``, when the
document has them, become the node covers TreeSHAP needs.
"""
from __future__ import annotations

import json
from typing import Dict, Sequence, Union

import numpy as np

from ..forest import (NODE_NAN_LEFT, T_IDENTITY, T_SIGMOID, T_SOFTMAX, TI_F32, TI_F64, Forest)

MAX_NODES = 1 << 26
NAN_TREATMENTS = ("AsIs", "AsFalse", "AsTrue")
LOSS_TRANSFORM = {
    "Logloss": T_SIGMOID, "CrossEntropy": T_SIGMOID, "MultiClass": T_SOFTMAX,
    "MultiClassOneVsAll": T_SIGMOID, "RMSE": T_IDENTITY, "MAE": T_IDENTITY,
    "Quantile": T_IDENTITY, "MAPE": T_IDENTITY, "Huber": T_IDENTITY, "LogCosh": T_IDENTITY,
}


class CatBoostFormatError(ValueError):
    pass


def _loss_name(doc: dict) -> str:
    try:
        loss = doc["model_info"]["params"]["loss_function"]
    except (KeyError, TypeError):
        raise CatBoostFormatError("model_info.params.loss_function is missing")
    name = loss.get("type") if isinstance(loss, dict) else loss
    if not isinstance(name, str):
        raise CatBoostFormatError("model_info.params.loss_function has no type")
    return name.split(":")[0]


def forest_from_catboost_doc(doc: dict) -> Forest:
    if not isinstance(doc, dict) or "oblivious_trees" not in doc:
        raise CatBoostFormatError("not a CatBoost JSON model: no oblivious_trees")
    info = doc.get("features_info") or {}
    if info.get("categorical_features"):
        raise CatBoostFormatError("categorical features are not served (their splits need "
                                  "CatBoost's string hashing)")
    if doc.get("ctrs") or doc.get("ctr_data"):
        raise CatBoostFormatError("CTR features are not served (they need CatBoost's string hashing)")
    floats = info.get("float_features") or []
    column, nan_left = [], []
    for ff in floats:
        treatment = ff.get("nan_value_treatment", "AsIs")
        if treatment not in NAN_TREATMENTS:
            raise CatBoostFormatError(f"unknown nan_value_treatment {treatment!r}")
        column.append(int(ff["flat_feature_index"]))
        nan_left.append(treatment != "AsTrue")
    scale, bias = doc.get("scale_and_bias", [1.0, [0.0]])
    if float(scale) != 1.0:
        raise CatBoostFormatError(f"scale_and_bias scale {scale} != 1 is not served (folding it "
                                  "into the leaves would change the rounding)")
    bias = np.atleast_1d(np.asarray(bias, dtype=np.float64))
    loss = _loss_name(doc)
    if loss not in LOSS_TRANSFORM:
        raise CatBoostFormatError(f"loss function {loss!r} is not served")
    trees = doc["oblivious_trees"]
    if not trees:
        raise CatBoostFormatError("the model has no trees")
    depths = [len(t.get("splits") or []) for t in trees]
    total = sum((2 << d) - 1 for d in depths)
    if total > MAX_NODES:
        raise CatBoostFormatError(f"the expanded model has {total} nodes, more than 2^26 "
                                  f"(deepest tree: depth {max(depths)})")
    dim = None
    for t, d in zip(trees, depths):
        n, rem = divmod(len(t["leaf_values"]), 1 << d)
        if rem or n < 1 or (dim is not None and n != dim):
            raise CatBoostFormatError("leaf_values is not 2^depth * dimension values in every tree")
        dim = n
    if bias.shape[0] == 1 and dim > 1:
        bias = np.repeat(bias, dim)
    if bias.shape[0] != dim:
        raise CatBoostFormatError(f"{bias.shape[0]} bias values for dimension {dim}")
    with_covers = all("leaf_weights" in t for t in trees)

    feature = np.full(total, -1, dtype=np.int32)
    threshold = np.zeros(total, dtype=np.float64)
    flags = np.zeros(total, dtype=np.uint8)
    left = np.full(total, -1, dtype=np.int32)
    right = np.full(total, -1, dtype=np.int32)
    leaf_id = np.zeros(total, dtype=np.int32)
    leaf_value = np.zeros((total, dim), dtype=np.float64)
    cover = np.zeros(total, dtype=np.float64) if with_covers else None
    offset = np.zeros(len(trees) + 1, dtype=np.int64)
    at = 0
    for ti, (t, D) in enumerate(zip(trees, depths)):
        n_int, n_leaf = (1 << D) - 1, 1 << D
        for level in range(D):   # heap order; the root tests the last split
            s = t["splits"][D - 1 - level]
            if s.get("split_type", "FloatFeature") != "FloatFeature":
                raise CatBoostFormatError(f"split type {s.get('split_type')!r} is not served "
                                          "(only FloatFeature splits)")
            fi = int(s["float_feature_index"])
            if not 0 <= fi < len(floats):
                raise CatBoostFormatError(f"split on float feature {fi}, the model has {len(floats)}")
            lo, hi = at + (1 << level) - 1, at + (2 << level) - 1
            feature[lo:hi] = column[fi]
            threshold[lo:hi] = float(np.float32(s["border"]))
            flags[lo:hi] = NODE_NAN_LEFT if nan_left[fi] else 0
        heap = np.arange(n_int, dtype=np.int32)
        left[at:at + n_int] = 2 * heap + 1
        right[at:at + n_int] = 2 * heap + 2
        leaves = slice(at + n_int, at + n_int + n_leaf)
        leaf_id[leaves] = np.arange(n_leaf, dtype=np.int32)
        leaf_value[leaves] = np.asarray(t["leaf_values"], dtype=np.float64).reshape(n_leaf, dim)
        if with_covers:
            w = np.asarray(t["leaf_weights"], dtype=np.float64)
            if w.shape[0] != n_leaf:
                raise CatBoostFormatError("leaf_weights is not 2^depth values in every tree")
            cover[leaves] = w
            for level in range(D - 1, -1, -1):   # a node's cover: the sum of its children's
                lo, hi = at + (1 << level) - 1, at + (2 << level) - 1
                kids = cover[at + (2 << level) - 1:at + (4 << level) - 1]
                cover[lo:hi] = kids[0::2] + kids[1::2]
        at += n_int + n_leaf
        offset[ti + 1] = at
    n_features = (max(column) + 1) if column else 1
    forest = Forest(
        n_features=n_features, n_groups=dim, leaf_width=dim, accum_dtype=TI_F64,
        base_first=False, lgb_zero_map=False, tree_offset=offset,
        tree_group=np.zeros(len(trees), dtype=np.int32), feature=feature, threshold=threshold,
        flags=flags, left=left, right=right, leaf_id=leaf_id, leaf_value=leaf_value,
        base_margin=bias, transform=LOSS_TRANSFORM[loss], input_dtype=TI_F32, cover=cover,
        library="catboost", objective=loss)
    forest.validate()
    return forest


def load_catboost_model(path: str) -> Forest:
    with open(path, "rb") as fh:
        raw = fh.read()
    if raw[:4] == b"CBM1":
        raise CatBoostFormatError("this is CatBoost's binary .cbm format; export the model with "
                                  'model.save_model(path, format="json")')
    try:
        doc = json.loads(raw)
    except ValueError as e:
        raise CatBoostFormatError(f"not a CatBoost JSON model ({e}); export the model with "
                                  'model.save_model(path, format="json")')
    return forest_from_catboost_doc(doc)


def json_model_doc(n_trees: int, depth: Union[int, Sequence[int]], n_features: int, dim: int = 1,
                   loss: str = "RMSE", seed: int = 0, borders: int = 16,
                   nan_treatment: Union[str, Sequence[str]] = "cycle",
                   leaf_weights: bool = False) -> Dict:
    """A seeded model document of the shape CatBoost exports (the subset the
    loader reads).  ``depth`` is one depth or one per tree; every feature gets
    ``borders`` sorted float32 borders that the trees' splits draw from, as
    CatBoost's quantisation makes them share; ``nan_treatment`` is one
    treatment, one per feature, or "cycle" through the three."""
    rng = np.random.default_rng(seed)
    depths = [int(depth)] * n_trees if np.isscalar(depth) else [int(d) for d in depth]
    if isinstance(nan_treatment, str):
        nan_treatment = ([NAN_TREATMENTS[i % 3] for i in range(n_features)]
                         if nan_treatment == "cycle" else [nan_treatment] * n_features)
    floats = []
    for i in range(n_features):
        b = np.unique(rng.standard_normal(borders).astype(np.float32))
        floats.append({"flat_feature_index": i, "feature_index": i, "has_nans": True,
                       "borders": [float(v) for v in b], "nan_value_treatment": nan_treatment[i]})
    trees = []
    for D in depths:
        splits = []
        for _ in range(D):
            fi = int(rng.integers(n_features))
            b = floats[fi]["borders"]
            splits.append({"float_feature_index": fi, "border": b[int(rng.integers(len(b)))],
                           "split_type": "FloatFeature"})
        tree = {"splits": splits,
                "leaf_values": [float(v) for v in rng.standard_normal((1 << D) * dim) * 0.1]}
        if leaf_weights:
            tree["leaf_weights"] = [float(v) for v in rng.integers(1, 50, 1 << D)]
        trees.append(tree)
    return {
        "features_info": {"float_features": floats},
        "model_info": {"params": {"loss_function": {"type": loss}}},
        "oblivious_trees": trees,
        "scale_and_bias": [1.0, [float(v) for v in rng.standard_normal(dim) * 0.5]],
    }
