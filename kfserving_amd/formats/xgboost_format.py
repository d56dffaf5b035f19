"""XGBoost model files -> canonical :class:`~kfserving_amd.forest.Forest`.

Replaces ``xgb.Booster(params={"nthread": n}, model_file=.../model.bst)`` at
python/xgbserver/xgbserver/model.py:38-39 without importing xgboost.  Reads:

* the legacy binary written by xgboost <= 0.90 (the reference pins 0.82,
  python/xgbserver/setup.py:37; fixture python/xgbserver/xgbserver/
  example_model/model/model.bst),
* the 1.x binary with the ``binf`` magic (fixture docs/samples/v1beta1/
  xgboost/model.bst), and
* the JSON model (xgboost >= 1.0 ``save_model("*.json")``) and its UBJSON
  form (xgboost >= 1.6 default ``.ubj``).

Predict semantics encoded (upstream xgboost 0.82 ``RegTree::GetNext`` /
``CPUPredictor::PredValue``): go left iff ``x < split`` in float32, a missing
value takes the node's default child, leaves summed in float32 in tree order
per output group from 0 and then added to the base margin.

Categorical nodes of JSON / UBJSON models (``split_type == 1``, xgboost >= 1.7
``common::Decision`` / ``GetNextNode``): a missing value takes the default
child; a value below 0 or at or above 2^24 is an invalid category and goes
left; otherwise the value truncated to an integer goes right iff it is in the
node's category set (include/treeinfer.h, TI_NODE_CAT_XGB).
"""
from __future__ import annotations

import base64
import json
import struct
from typing import List, Optional, Tuple

import numpy as np

from ..forest import (Forest, NODE_CAT_XGB, NODE_CATEGORICAL, NODE_NAN_LEFT, TI_F32, T_ARGMAX,
                      T_EXP, T_HINGE, T_IDENTITY, T_SIGMOID, T_SOFTMAX, concat_trees)

MAX_CATEGORY = 1 << 24      # xgboost's kMaxCat: category codes are in [0, 2^24)
_CAT_MIN_VERSION = (1, 7, 0)   # 1.5 / 1.6 sent invalid categories to the default child

# on-disk structs of the legacy / binf binary (little endian)
_LEARNER_PARAM = 136       # LearnerModelParam
_GBTREE_PARAM = 160        # GBTreeModelParam
_TREE_PARAM = 148          # TreeParam
_NODE_DTYPE = np.dtype([("parent", "<i4"), ("cleft", "<i4"), ("cright", "<i4"),
                        ("sindex", "<u4"), ("info", "<f4")])        # 20 B
_STAT_BYTES = 16           # RTreeNodeStat
_DELETED = 0xFFFFFFFF

_SIGMOID_OBJ = ("binary:logistic", "reg:logistic")
_LOGIT_BASE_OBJ = ("binary:logistic", "reg:logistic", "binary:logitraw")
_EXP_OBJ = ("count:poisson", "reg:gamma", "reg:tweedie", "survival:cox", "survival:aft")


class XGBoostFormatError(ValueError):
    pass


class _Reader:
    def __init__(self, buf: bytes, pos: int = 0):
        self.buf = buf
        self.pos = pos

    def take(self, n: int) -> bytes:
        if self.pos + n > len(self.buf):
            raise XGBoostFormatError(f"truncated model: need {n} bytes at offset {self.pos}")
        b = self.buf[self.pos:self.pos + n]
        self.pos += n
        return b

    def unpack(self, fmt: str):
        return struct.unpack(fmt, self.take(struct.calcsize(fmt)))

    def string(self) -> str:
        (n,) = self.unpack("<Q")
        if n > len(self.buf):
            raise XGBoostFormatError("implausible string length")
        return self.take(n).decode("utf-8", "replace")


def objective_transform(objective: str) -> int:
    if objective in _SIGMOID_OBJ:
        return T_SIGMOID
    if objective == "multi:softmax":
        return T_ARGMAX
    if objective == "multi:softprob":
        return T_SOFTMAX
    if objective == "binary:hinge":
        return T_HINGE
    if objective in _EXP_OBJ:
        return T_EXP
    return T_IDENTITY


def prob_to_margin(objective: str, base_score: float) -> float:
    """ObjFunction::ProbToMargin in float32 (applied to xgboost >= 1.0 models)."""
    b = np.float32(base_score)
    with np.errstate(divide="ignore", invalid="ignore"):
        if objective in _LOGIT_BASE_OBJ:
            return float(-np.log(np.float32(1.0) / b - np.float32(1.0)))
        if objective in ("count:poisson", "reg:gamma", "reg:tweedie"):
            return float(np.log(b))
    return float(b)


def xgb_threshold(split: np.ndarray) -> np.ndarray:
    """x < t (float32)  <=>  x <= nextafterf(t, -inf); t = -inf never goes left."""
    s = np.asarray(split, dtype=np.float32)
    t = np.nextafter(s, np.float32(-np.inf)).astype(np.float64)
    t[np.isneginf(s)] = np.nan
    t[np.isnan(s)] = np.nan
    return t


_STAT_DTYPE = np.dtype([("loss_chg", "<f4"), ("sum_hess", "<f4"), ("base_weight", "<f4"),
                        ("leaf_child_cnt", "<i4")])


def _tree_from_arrays(cleft, cright, sindex, value, deleted=None, sum_hess=None) -> dict:
    cleft = np.asarray(cleft, dtype=np.int32)
    cright = np.asarray(cright, dtype=np.int32)
    sindex = np.asarray(sindex, dtype=np.uint32)
    value = np.asarray(value, dtype=np.float32)
    n = cleft.shape[0]
    leaf = cleft == -1
    if deleted is not None:
        leaf = leaf | deleted
    feature = np.where(leaf, -1, (sindex & 0x7FFFFFFF).astype(np.int64)).astype(np.int32)
    default_left = (sindex >> 31) != 0
    threshold = np.where(leaf, 0.0, xgb_threshold(value))
    flags = np.where(~leaf & default_left, NODE_NAN_LEFT, 0).astype(np.uint8)
    return {
        "feature": feature,
        "threshold": threshold,
        "flags": flags,
        "left": np.where(leaf, -1, cleft).astype(np.int32),
        "right": np.where(leaf, -1, cright).astype(np.int32),
        "leaf_id": np.arange(n, dtype=np.int32),
        "leaf_value": np.where(leaf, value, np.float32(0)).astype(np.float64).reshape(n, 1),
        # RTreeNodeStat::sum_hess, the cover TreeSHAP weights children by
        "cover": None if sum_hess is None else np.asarray(sum_hess, dtype=np.float32)
        .astype(np.float64),
    }


def _category_codes(codes) -> np.ndarray:
    """One node's category set as validated int64 codes in [0, 2^24)."""
    try:
        raw = np.asarray(codes, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise XGBoostFormatError(f"malformed category set: {e}") from e
    if raw.size and not (np.all(np.isfinite(raw)) and np.all(raw == np.floor(raw))):
        raise XGBoostFormatError("category codes must be integers")
    if raw.size and (raw.min() < 0 or raw.max() >= MAX_CATEGORY):
        raise XGBoostFormatError(f"category code outside [0, {MAX_CATEGORY})")
    return raw.astype(np.int64)


def _set_categorical(t: dict, cats) -> None:
    """Make the nodes ``cats`` names (node id -> category codes) of canonical
    tree ``t`` XGBoost-rule categorical nodes: threshold unused (0), the
    default child kept in NAN_LEFT, one bitset per node just long enough for
    its highest category."""
    n = t["feature"].shape[0]
    off = np.full(n, -1, dtype=np.int64)
    nw = np.zeros(n, dtype=np.int32)
    words, total = [], 0
    cats = {int(k): v for k, v in cats.items()}
    for node in sorted(cats):
        if not (0 <= node < n) or t["feature"][node] < 0:
            raise XGBoostFormatError(f"categorical node {node} is not a split node")
        codes = _category_codes(cats[node])
        bits = np.zeros(int(codes.max()) // 32 + 1 if codes.size else 0, dtype=np.uint32)
        np.bitwise_or.at(bits, codes // 32, np.uint32(1) << (codes % 32).astype(np.uint32))
        off[node], nw[node] = total, bits.size
        words.append(bits)
        total += bits.size
        t["threshold"][node] = 0.0
        t["flags"][node] = NODE_CATEGORICAL | NODE_CAT_XGB | (int(t["flags"][node]) & NODE_NAN_LEFT)
    t["cat_offset"], t["cat_nwords"] = off, nw
    t["cat_words"] = np.concatenate(words) if words else np.zeros(0, dtype=np.uint32)


def _concat_categories(trees: List[dict]):
    """cat_bits / cat_offset / cat_nwords of the forest from the per-tree
    bitsets (node offsets become offsets into the forest's words)."""
    if not any("cat_words" in t for t in trees):
        return None, None, None
    base, words, offs, nws = 0, [], [], []
    for t in trees:
        n = t["feature"].shape[0]
        o = t.get("cat_offset", np.full(n, -1, dtype=np.int64)).copy()
        o[o >= 0] += base
        offs.append(o)
        nws.append(t.get("cat_nwords", np.zeros(n, dtype=np.int32)))
        w = t.get("cat_words", np.zeros(0, dtype=np.uint32))
        words.append(w)
        base += w.size
    bits = np.concatenate(words).astype(np.uint32)
    if bits.size == 0:          # only empty sets: the ABI still wants a words array
        bits = np.zeros(1, dtype=np.uint32)
    return bits, np.concatenate(offs), np.concatenate(nws).astype(np.int32)


def _assemble(trees: List[dict], tree_info: np.ndarray, num_feature: int, num_group: int,
              base_score, objective: str, base_is_margin: bool, base_first: bool,
              version: Tuple[int, int, int], feature_names=None, fmt: str = "") -> Forest:
    """``base_score``: one value, or one per output group (xgboost >= 2 vector)."""
    cat = concat_trees(trees, 1)
    cat_bits, cat_offset, cat_nwords = _concat_categories(trees)
    used = cat["feature"][cat["feature"] >= 0]
    n_features = max(int(num_feature), int(used.max()) + 1 if used.size else 1)
    K = max(1, int(num_group))
    scores = np.atleast_1d(np.asarray(base_score, dtype=np.float64))
    margins = [s if base_is_margin else prob_to_margin(objective, s) for s in scores]
    base = np.empty(K, dtype=np.float64)
    base[:] = [float(np.float32(m)) for m in margins]     # one value broadcasts over K
    if scores.size == 1:
        base_score = float(scores[0])
    else:
        base_score = [float(s) for s in scores]
    tinfo = np.asarray(tree_info, dtype=np.int32)
    if tinfo.shape[0] != len(trees):
        raise XGBoostFormatError("tree_info length does not match the number of trees")
    return Forest(
        n_features=n_features, n_groups=K, leaf_width=1, accum_dtype=TI_F32,
        base_first=base_first, lgb_zero_map=False,
        tree_offset=cat["tree_offset"], tree_group=tinfo,
        feature=cat["feature"], threshold=cat["threshold"], flags=cat["flags"],
        left=cat["left"], right=cat["right"], leaf_id=cat["leaf_id"],
        leaf_value=cat["leaf_value"], base_margin=base, cover=cat["cover"],
        transform=objective_transform(objective), transform_param=1.0,
        input_dtype=TI_F32, library="xgboost", objective=objective,
        feature_names=feature_names,
        meta={"format": fmt, "version": version, "base_score": base_score},
        cat_bits=cat_bits, cat_offset=cat_offset, cat_nwords=cat_nwords,
    ).contiguous()


def _parse_binary(buf: bytes, pos: int, fmt: str) -> Forest:
    r = _Reader(buf, pos)
    lp = r.take(_LEARNER_PARAM)
    base_score, num_feature, num_class, extra_attrs, eval_metrics, major, minor = \
        struct.unpack_from("<fIiiiii", lp, 0)
    objective = r.string()
    gbm = r.string()
    if gbm not in ("gbtree", "dart"):
        raise XGBoostFormatError(f"booster '{gbm}' is not a tree ensemble")
    gp = r.take(_GBTREE_PARAM)
    num_trees, num_roots, g_num_feature, _pad, _pbuf, num_output_group, size_leaf_vector = \
        struct.unpack_from("<iiiiqii", gp, 0)
    if size_leaf_vector != 0:
        raise XGBoostFormatError("size_leaf_vector != 0 is not supported")
    trees = []
    for _ in range(num_trees):
        tp = r.take(_TREE_PARAM)
        t_roots, num_nodes, num_deleted, _max_depth, _nf, t_slv = struct.unpack_from("<6i", tp, 0)
        if num_nodes <= 0:
            raise XGBoostFormatError("tree with no nodes")
        nodes = np.frombuffer(r.take(_NODE_DTYPE.itemsize * num_nodes), dtype=_NODE_DTYPE)
        stats = np.frombuffer(r.take(_STAT_BYTES * num_nodes), dtype=_STAT_DTYPE)
        if t_slv != 0:
            (nlv,) = r.unpack("<Q")
            r.take(4 * nlv)
        deleted = nodes["sindex"] == _DELETED
        trees.append(_tree_from_arrays(nodes["cleft"], nodes["cright"], nodes["sindex"],
                                       nodes["info"], deleted, stats["sum_hess"]))
    tree_info = np.frombuffer(r.take(4 * num_trees), dtype="<i4") if num_trees else np.zeros(0)
    if gbm == "dart":
        (nw,) = r.unpack("<Q")
        weights = np.frombuffer(r.take(4 * nw), dtype="<f4")
        for t, w in zip(trees, weights):     # Dart::Pred: weight_drop[i] * leaf (float32)
            lv = t["leaf_value"][:, 0].astype(np.float32) * np.float32(w)
            t["leaf_value"] = lv.astype(np.float64).reshape(-1, 1)
    attrs = {}
    if extra_attrs != 0 and r.pos < len(buf):
        (na,) = r.unpack("<Q")
        for _ in range(na):
            k = r.string()
            attrs[k] = r.string()
    version = (major, minor, 0)
    # xgboost < 1.0 stores base_score already in margin space; >= 1.0 stores the
    # user value and applies ProbToMargin at load (LearnerIO::LoadModel).
    base_is_margin = major < 1
    # xgboost >= 1.0 deprecates num_output_group in favour of the learner's num_class
    num_group = max(1, num_output_group, num_class)
    f = _assemble(trees, tree_info, num_feature, num_group, base_score, objective,
                  base_is_margin=base_is_margin, base_first=False, version=version, fmt=fmt)
    f.meta["attributes"] = attrs
    f.meta["trailing_bytes"] = len(buf) - r.pos
    return f


def _json_num(v) -> float:
    if isinstance(v, list):
        v = v[0]
    return float(v)


def _json_base_score(v, num_class: int):
    """learner_model_param.base_score: a number (or its string), or the
    bracketed list recent xgboost writes (``"[5E-1]"``, or one value per
    class): one value, or exactly ``num_class`` of them."""
    if isinstance(v, str) and v.strip().startswith("["):
        body = v.strip()
        if not body.endswith("]"):
            raise XGBoostFormatError(f"malformed base_score {v!r}")
        try:
            vals = [float(p) for p in body[1:-1].split(",")]
        except ValueError as e:
            raise XGBoostFormatError(f"malformed base_score {v!r}") from e
        if len(vals) != 1 and len(vals) != max(1, num_class):
            raise XGBoostFormatError(f"base_score holds {len(vals)} values, expected 1 or "
                                     f"num_class = {max(1, num_class)}")
        return vals[0] if len(vals) == 1 else vals
    try:
        return _json_num(v)
    except (TypeError, ValueError) as e:
        raise XGBoostFormatError(f"malformed base_score {v!r}") from e


def _int_array(jt: dict, key: str) -> np.ndarray:
    try:
        a = np.asarray(jt.get(key, []), dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise XGBoostFormatError(f"malformed {key}: {e}") from e
    if a.size and not (np.all(np.isfinite(a)) and np.all(a == np.floor(a))):
        raise XGBoostFormatError(f"{key} must hold integers")
    return a.astype(np.int64)


def _json_categories(jt: dict, n_nodes: int, version) -> dict:
    """The categorical nodes of one JSON tree as {node id: category codes},
    from split_type / categories / categories_nodes / categories_segments /
    categories_sizes; every inconsistency is an XGBoostFormatError."""
    split_type = _int_array(jt, "split_type")
    nodes = _int_array(jt, "categories_nodes")
    if not split_type.any() and nodes.size == 0:
        return {}
    if tuple(version) < _CAT_MIN_VERSION:
        raise XGBoostFormatError(
            "categorical splits of xgboost version %s are not supported (invalid categories "
            "took the default child before 1.7.0)" % ".".join(str(v) for v in version))
    if split_type.size != n_nodes:
        raise XGBoostFormatError("split_type length does not match the number of nodes")
    if np.any((split_type != 0) & (split_type != 1)):
        raise XGBoostFormatError("unknown split_type")
    segments = _int_array(jt, "categories_segments")
    sizes = _int_array(jt, "categories_sizes")
    categories = _int_array(jt, "categories")
    if segments.size != nodes.size or sizes.size != nodes.size:
        raise XGBoostFormatError("categories_nodes / _segments / _sizes differ in length")
    if nodes.size and (nodes.min() < 0 or nodes.max() >= n_nodes or np.any(np.diff(nodes) <= 0)):
        raise XGBoostFormatError("categories_nodes must be strictly increasing node ids")
    named = np.zeros(n_nodes, dtype=bool)
    named[nodes] = True
    if np.any(named != (split_type == 1)):
        raise XGBoostFormatError("categories_nodes does not name exactly the split_type == 1 nodes")
    if np.any(segments < 0) or np.any(sizes < 0) or np.any(segments + sizes > categories.size):
        raise XGBoostFormatError("category segment outside the categories array")
    return {int(nd): categories[b:b + s] for nd, b, s in zip(nodes, segments, sizes)}


def _parse_json(doc: dict) -> Forest:
    learner = doc["learner"]
    lmp = learner["learner_model_param"]
    num_class = int(_json_num(lmp.get("num_class", 0)))
    base_score = _json_base_score(lmp.get("base_score", 0.5), num_class)
    num_feature = int(_json_num(lmp.get("num_feature", 0)))
    objective = learner["objective"]["name"]
    gb = learner["gradient_booster"]
    name = gb["name"]
    weights = None
    if name == "gbtree":
        model = gb["model"]
    elif name == "dart":
        model = gb["gbtree"]["model"]
        weights = np.asarray(gb["weight_drop"], dtype=np.float32)
    else:
        raise XGBoostFormatError(f"booster '{name}' is not a tree ensemble")
    version = tuple(int(v) for v in doc.get("version", [1, 0, 0]))
    trees = []
    for i, jt in enumerate(model["trees"]):
        cleft = np.asarray(jt["left_children"], dtype=np.int32)
        dl = np.asarray(jt["default_left"], dtype=np.uint32) & 1
        sindex = np.asarray(jt["split_indices"], dtype=np.uint32) | (dl << 31)
        t = _tree_from_arrays(cleft, jt["right_children"], sindex, jt["split_conditions"],
                              sum_hess=jt.get("sum_hessian"))
        cats = _json_categories(jt, cleft.shape[0], version)
        if cats:
            _set_categorical(t, cats)
        if weights is not None:
            lv = t["leaf_value"][:, 0].astype(np.float32) * weights[i]
            t["leaf_value"] = lv.astype(np.float64).reshape(-1, 1)
        trees.append(t)
    K = max(1, num_class)
    names = learner.get("feature_names") or None
    return _assemble(trees, model["tree_info"], num_feature, K, base_score, objective,
                     base_is_margin=False, base_first=version >= (1, 4, 0), version=version,
                     feature_names=names, fmt="json")


def parse_xgboost_bytes(buf: bytes) -> Forest:
    if buf[:4] == b"binf":
        return _parse_binary(buf, 4, "binf")
    if buf[:4] == b"bs64":
        return _parse_binary(base64.b64decode(buf[4:]), 0, "legacy-b64")
    head = buf.lstrip()[:1]
    if head == b"{":
        # JSON text continues with whitespace or a quoted key; UBJSON with a
        # length marker ('U', 'i', 'l', ...) or a container header ('$', '#')
        if buf[1:2] in (b'"', b" ", b"\n", b"\r", b"\t", b"}"):
            try:
                doc = json.loads(buf.decode("utf-8"))
            except (UnicodeDecodeError, json.JSONDecodeError) as e:
                raise XGBoostFormatError(f"malformed JSON model: {e}") from e
            return _parse_json(doc)
        from . import ubjson
        try:
            doc = ubjson.loads(buf)
        except (ubjson.UBJSONError, KeyError, UnicodeDecodeError) as e:
            raise XGBoostFormatError(f"malformed UBJSON model: {e}") from e
        f = _parse_json(doc)
        f.meta["format"] = "ubj"
        return f
    return _parse_binary(buf, 0, "legacy")


def load_xgboost_model(path: str) -> Forest:
    with open(path, "rb") as fh:
        return parse_xgboost_bytes(fh.read())


# ------------------------------------------------------------------ writers
def write_legacy_binary(path: str, trees: List[dict], tree_info, num_feature: int,
                        num_class: int, base_score: float, objective: str) -> None:
    """Write an xgboost-0.82 legacy binary model.

    ``trees`` hold XGBoost RegTree arrays: ``cleft, cright, sindex`` (bit 31 =
    default_left) and ``value`` (split condition or leaf value).  Used for the
    synthetic benchmark models; the layout is the one
    the loader above reads and that fixture #1 follows.
    """
    out = bytearray()
    lp = bytearray(_LEARNER_PARAM)
    struct.pack_into("<fIiii", lp, 0, base_score, num_feature, num_class, 0, 0)
    out += lp
    for s in (objective, "gbtree"):
        b = s.encode()
        out += struct.pack("<Q", len(b)) + b
    num_group = max(1, num_class)
    gp = bytearray(_GBTREE_PARAM)
    struct.pack_into("<iiiiqii", gp, 0, len(trees), 1, num_feature, 0, 0, num_group, 0)
    out += gp
    for t in trees:
        n = len(t["cleft"])
        tp = bytearray(_TREE_PARAM)
        struct.pack_into("<6i", tp, 0, 1, n, 0, 0, num_feature, 0)
        out += tp
        nodes = np.zeros(n, dtype=_NODE_DTYPE)
        nodes["cleft"] = t["cleft"]
        nodes["cright"] = t["cright"]
        nodes["sindex"] = t["sindex"]
        nodes["info"] = t["value"]
        parent = np.full(n, -1, dtype=np.int64)
        for i in range(n):
            if t["cleft"][i] != -1:
                parent[t["cleft"][i]] = i | (1 << 31)
                parent[t["cright"][i]] = i
        nodes["parent"] = parent.astype(np.uint32).view(np.int32)
        out += nodes.tobytes()
        stats = np.zeros(n, dtype=_STAT_DTYPE)
        if "sum_hess" in t:
            stats["sum_hess"] = t["sum_hess"]
        out += stats.tobytes()
    out += np.asarray(tree_info, dtype="<i4").tobytes()
    with open(path, "wb") as fh:
        fh.write(bytes(out))


def json_model_doc(trees: List[dict], tree_info, num_feature: int, num_class: int,
                   base_score: float, objective: str, version=(1, 3, 0), arrays=False) -> dict:
    """The xgboost >= 1.0 JSON model document (subset the loader reads);
    ``arrays=True`` keeps numpy arrays (for the UBJSON writer).  A tree may
    carry ``cats``, a mapping of node id to category codes: those nodes are
    written as categorical splits (split_type 1 and the four categories_*
    arrays of xgboost >= 1.5; the loader takes them from version 1.7.0 on)."""
    jt = []
    for i, t in enumerate(trees):
        n = len(t["cleft"])
        conv = (lambda a, dt: np.asarray(a, dtype=dt)) if arrays else \
            (lambda a, dt: [dt(v).item() for v in np.asarray(a, dtype=dt)])
        extra = {}
        if t.get("cats"):
            cats = {int(k): np.asarray(v, dtype=np.int64).reshape(-1) for k, v in t["cats"].items()}
            nodes = sorted(cats)
            sizes = [cats[k].size for k in nodes]
            split_type = np.zeros(n, dtype=np.uint8)
            split_type[nodes] = 1
            extra = {
                "split_type": conv(split_type, np.uint8),
                "categories": conv(np.concatenate([cats[k] for k in nodes]), np.int32),
                "categories_nodes": conv(nodes, np.int32),
                "categories_segments": conv(np.cumsum([0] + sizes[:-1]), np.int64),
                "categories_sizes": conv(sizes, np.int64),
            }
        jt.append({
            "id": i,
            "left_children": conv(t["cleft"], np.int32),
            "right_children": conv(t["cright"], np.int32),
            "split_indices": conv(np.asarray(t["sindex"]) & 0x7FFFFFFF, np.int32),
            "default_left": conv(np.asarray(t["sindex"]) >> 31, np.uint8),
            "split_conditions": conv(t["value"], np.float32),
            "sum_hessian": conv(t.get("sum_hess", np.zeros(n)), np.float32),
            "tree_param": {"num_nodes": str(n), "num_feature": str(num_feature),
                           "size_leaf_vector": "0"},
            **extra,
        })
    return {
        "version": list(version),
        "learner": {
            "attributes": {},
            "feature_names": [],
            "learner_model_param": {"base_score": repr(float(base_score)),
                                    "num_class": str(num_class),
                                    "num_feature": str(num_feature)},
            "objective": {"name": objective},
            "gradient_booster": {"name": "gbtree", "model": {
                "gbtree_model_param": {"num_trees": str(len(trees)), "size_leaf_vector": "0"},
                "tree_info": np.asarray(tree_info, dtype=np.int32) if arrays
                else [int(v) for v in tree_info],
                "trees": jt}},
        },
    }


def write_ubj_model(path: str, trees: List[dict], tree_info, num_feature: int, num_class: int,
                    base_score: float, objective: str, version=(1, 6, 0)) -> None:
    """Write the model as xgboost >= 1.6 UBJSON."""
    from . import ubjson
    doc = json_model_doc(trees, tree_info, num_feature, num_class, base_score, objective,
                         version, arrays=True)
    with open(path, "wb") as fh:
        fh.write(ubjson.dumps(doc))


def write_json_model(path: str, trees: List[dict], tree_info, num_feature: int, num_class: int,
                     base_score: float, objective: str, version=(1, 3, 0)) -> None:
    """Write the same model as xgboost >= 1.0 JSON (subset the loader reads)."""
    doc = json_model_doc(trees, tree_info, num_feature, num_class, base_score, objective, version)
    with open(path, "w") as fh:
        json.dump(doc, fh)


def synthetic_complete_trees(n_trees: int, depth: int, n_features: int, seed: int,
                             num_class: int = 0, max_bin: int = 0) -> Tuple[List[dict], np.ndarray]:
    """Seeded complete depth-``depth`` XGBoost trees.

    feature ~ U{0..F-1}, threshold ~ N(0,1) rounded to float32, default_left ~
    Bernoulli(1/2), leaf ~ U(-0.05, 0.05) float32; nodes numbered in heap order;
    sum_hess (the covers) from a seeded N(0,1) sample.  ``max_bin`` > 0 snaps
    every threshold to the nearest of the max_bin - 1 N(0,1) quantile edges
    Phi^-1(k / max_bin), as xgboost's hist / approx tree methods place splits
    on histogram bin bounds (at most max_bin - 1 distinct thresholds a
    feature: u8 bins in the engine); the draws are the same either way.
    """
    edges = None
    if max_bin > 0:
        from statistics import NormalDist
        nd = NormalDist()
        edges = np.array([nd.inv_cdf(k / max_bin) for k in range(1, max_bin)], dtype=np.float32)
    rng = np.random.default_rng(seed)
    crng = np.random.default_rng([seed, 7919])   # covers: own stream, trees unchanged
    n_int = (1 << depth) - 1
    n = 2 * n_int + 1
    trees = []
    for _ in range(n_trees):
        cleft = np.full(n, -1, dtype=np.int32)
        cright = np.full(n, -1, dtype=np.int32)
        idx = np.arange(n_int)
        cleft[:n_int] = 2 * idx + 1
        cright[:n_int] = 2 * idx + 2
        feat = rng.integers(0, n_features, size=n_int).astype(np.uint32)
        dl = rng.integers(0, 2, size=n_int).astype(np.uint32)
        sindex = np.zeros(n, dtype=np.uint32)
        sindex[:n_int] = feat | (dl << 31)
        value = np.zeros(n, dtype=np.float32)
        value[:n_int] = rng.standard_normal(n_int).astype(np.float32)
        if edges is not None:
            value[:n_int] = edges[np.abs(value[:n_int, None] - edges[None, :]).argmin(axis=1)]
        value[n_int:] = rng.uniform(-0.05, 0.05, size=n - n_int).astype(np.float32)
        # covers as training on N(0,1) rows leaves them: the logistic hessian
        # sum p(1 - p) ~ 0.25 per row of a seeded N(0,1) sample reaching each
        # leaf (+ 1 row: no empty leaf), a parent the float32 sum of its
        # children; from the covers' own stream (the trees are unchanged)
        Xs = crng.standard_normal((2000, n_features)).astype(np.float32)
        node = np.zeros(Xs.shape[0], dtype=np.int64)
        for _ in range(depth):
            go_left = ~(Xs[np.arange(Xs.shape[0]), feat[node]] >= value[node])   # x < t or NaN
            node = np.where(go_left, cleft[node], cright[node])
        hess = np.zeros(n, dtype=np.float32)
        hess[n_int:] = (0.25 * (np.bincount(node - n_int, minlength=n - n_int) + 1)).astype(np.float32)
        for i in range(n_int - 1, -1, -1):
            hess[i] = hess[2 * i + 1] + hess[2 * i + 2]
        trees.append({"cleft": cleft, "cright": cright, "sindex": sindex, "value": value,
                      "sum_hess": hess})
    K = max(1, num_class)
    tree_info = (np.arange(n_trees) % K).astype(np.int32)
    return trees, tree_info


def edge_category_sets(n_categories: int) -> List[np.ndarray]:
    """The category sets at the edges of a bitset over ``n_categories`` values
    (its last word is word (n - 1) // 32): only bit 31 of the last word, every
    category, only bit 0 of the last word, {n - 1} and {0}."""
    n = int(n_categories)
    last = 32 * ((n - 1) // 32)
    return [np.array([last + 31], dtype=np.int32), np.arange(n, dtype=np.int32),
            np.array([last], dtype=np.int32), np.array([n - 1], dtype=np.int32),
            np.array([0], dtype=np.int32)]


def add_categorical_splits(trees: List[dict], cat_features, n_categories: int, seed: int,
                           frac: float = 0.5, edge_frac: float = 0.0,
                           root_trees: int = 0) -> List[dict]:
    """Turn a seeded fraction of the splits on ``cat_features`` of XGBoost raw
    trees into categorical nodes (``cats``: node id -> category codes) with
    random non-empty sets over ``n_categories`` values; the sibling of
    lightgbm_format.add_categorical_splits.  The nodes keep their feature,
    children and default direction; their split condition is unused.

    For tests of the bitset edges (both default to off, and draw from a stream
    of their own, so the plain output is the same with or without them):
    ``edge_frac`` of the categorical nodes take one of edge_category_sets in
    turn instead of their random set, and the roots of the first
    ``root_trees`` trees become categorical nodes on ``cat_features[i % n]``
    with edge set ``i % 5`` (tree i), so every row meets a categorical node."""
    rng = np.random.default_rng(seed)
    erng = np.random.default_rng([seed, 24])
    edge = edge_category_sets(n_categories)
    n_edge = 0
    cat_features = np.asarray(cat_features, dtype=np.int64)
    for ti, t in enumerate(trees):
        cleft = np.asarray(t["cleft"])
        feat = (np.asarray(t["sindex"], dtype=np.uint32) & 0x7FFFFFFF).astype(np.int64)
        cats = dict(t.get("cats") or {})
        for i in np.nonzero((cleft != -1) & np.isin(feat, cat_features))[0]:
            if rng.random() >= frac:
                continue
            members = np.nonzero(rng.random(n_categories) < 0.4)[0]
            if members.size == 0:
                members = np.array([int(rng.integers(0, n_categories))])
            if edge_frac > 0 and erng.random() < edge_frac:
                members = edge[n_edge % len(edge)]
                n_edge += 1
            cats[int(i)] = members.astype(np.int32)
        if ti < root_trees and cleft[0] != -1:
            sindex = np.array(t["sindex"], dtype=np.uint32)
            sindex[0] = (sindex[0] & np.uint32(0x80000000)) | \
                np.uint32(cat_features[ti % cat_features.shape[0]])
            t["sindex"] = sindex
            cats[0] = edge[ti % len(edge)]
        if cats:
            t["cats"] = cats
    return trees


def forest_from_raw_trees(trees: List[dict], tree_info, num_feature: int, num_class: int,
                          base_score: float, objective: str, legacy: bool = True) -> Forest:
    """Canonical forest straight from RegTree arrays (what the writers store)."""
    canon = [_tree_from_arrays(t["cleft"], t["cright"], t["sindex"], t["value"],
                              sum_hess=t.get("sum_hess")) for t in trees]
    for c, t in zip(canon, trees):
        if t.get("cats"):
            _set_categorical(c, t["cats"])
    return _assemble(canon, tree_info, num_feature, max(1, num_class), base_score, objective,
                     base_is_margin=legacy, base_first=False,
                     version=(0, 82, 0) if legacy else (1, 3, 0), fmt="raw")
