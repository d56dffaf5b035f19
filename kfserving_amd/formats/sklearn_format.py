"""sklearn tree ensembles -> canonical :class:`~kfserving_amd.forest.Forest`.

Replaces the estimator the reference unpickles at
python/sklearnserver/sklearnserver/model.py:38 (``joblib.load``) and calls at
:50 (``self._model.predict``).  Supported: DecisionTree{Regressor,Classifier},
RandomForest{Regressor,Classifier}, ExtraTrees{Regressor,Classifier} with one
output, GradientBoosting{Regressor,Classifier} (forest_from_gradient_boosting)
and HistGradientBoosting{Regressor,Classifier}
(forest_from_hist_gradient_boosting), and a Pipeline of SimpleImputer /
StandardScaler / MinMaxScaler / MaxAbsScaler / RobustScaler steps in front of
any of these but HistGradientBoosting (forest_from_pipeline).

Predict semantics encoded (installed sklearn 1.7.2,
sklearn/tree/_tree.pyx:979-997 and sklearn/ensemble/_forest.py:723-736,
882-962, 1044-1085): X converted to float32; at a node, NaN goes to
``missing_go_to_left``'s side, otherwise left iff ``(double)x <= threshold``;
regressors sum ``value[leaf]`` in float64 in estimator order and divide by
n_estimators; classifiers do the same with the per-leaf class-fraction
vector and take the first argmax.

HistGradientBoosting is the one family that keeps X in float64 and carries
categorical splits (ensemble/_hist_gradient_boosting/gradient_boosting.py,
_predictor.pyx, common.pyx): its forests declare ``input_dtype`` TI_F64 and
restate sklearn's categorical node as the XGBoost-rule node the kernels
already evaluate -- see forest_from_hist_gradient_boosting.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from ..forest import (Forest, NODE_NAN_LEFT, PRE_ADD, PRE_DIV, PRE_FILL_NAN, PRE_MAX_STEPS, PRE_MUL,
                      PRE_SUB, TI_F32, TI_F64, T_ARGMAX, T_EXP, T_HINGE, T_IDENTITY, T_STEP,
                      concat_trees)

TREE_LEAF = -1


def tree_arrays_from_sklearn(tree_) -> dict:
    """Raw arrays of a fitted ``sklearn.tree._tree.Tree``."""
    mgl = getattr(tree_, "missing_go_to_left", None)
    n = int(tree_.node_count)
    return {
        "children_left": np.asarray(tree_.children_left, dtype=np.int64),
        "children_right": np.asarray(tree_.children_right, dtype=np.int64),
        "feature": np.asarray(tree_.feature, dtype=np.int64),
        "threshold": np.asarray(tree_.threshold, dtype=np.float64),
        "missing_go_to_left": (np.asarray(mgl, dtype=np.uint8) if mgl is not None
                               else np.zeros(n, dtype=np.uint8)),
        "value": np.asarray(tree_.value, dtype=np.float64),
        "cover": np.asarray(tree_.weighted_n_node_samples, dtype=np.float64),
    }


def _canon_tree(arr: dict, classifier: bool, n_classes: int) -> dict:
    cl = arr["children_left"]
    cr = arr["children_right"]
    leaf = cl == TREE_LEAF
    n = cl.shape[0]
    value = arr["value"]
    if value.ndim != 3 or value.shape[1] != 1:
        raise ValueError("multi-output sklearn trees are not supported")
    lv = value[:, 0, :n_classes] if classifier else value[:, 0, :1]
    return {
        "feature": np.where(leaf, -1, arr["feature"]),
        "threshold": np.where(leaf, 0.0, arr["threshold"]),
        "flags": np.where(~leaf & (arr["missing_go_to_left"] != 0), NODE_NAN_LEFT, 0),
        "left": np.where(leaf, -1, cl),
        "right": np.where(leaf, -1, cr),
        "leaf_id": np.arange(n),
        "leaf_value": np.where(leaf[:, None], lv, 0.0),
        "cover": arr.get("cover"),
    }


def forest_from_tree_arrays(trees, n_features: int, classifier: bool, n_classes: int = 1,
                            average: bool = True, classes=None, kind: str = "") -> Forest:
    K = n_classes if classifier else 1
    canon = [_canon_tree(a, classifier, K) for a in trees]
    cat = concat_trees(canon, K)
    return Forest(
        n_features=int(n_features), n_groups=K, leaf_width=K, accum_dtype=TI_F64,
        base_first=True, lgb_zero_map=False,
        tree_offset=cat["tree_offset"], tree_group=np.zeros(len(trees), dtype=np.int32),
        feature=cat["feature"], threshold=cat["threshold"], flags=cat["flags"],
        left=cat["left"], right=cat["right"], leaf_id=cat["leaf_id"],
        leaf_value=cat["leaf_value"], base_margin=np.zeros(K), cover=cat["cover"],
        average_divisor=float(len(trees)) if average else 1.0,
        transform=T_ARGMAX if classifier else T_IDENTITY, transform_param=1.0,
        input_dtype=TI_F32, library="sklearn", objective=kind,
        meta={"classes": None if classes is None else np.asarray(classes)},
    ).contiguous()


def _estimators(est) -> Tuple[list, bool]:
    name = type(est).__name__
    if name in ("RandomForestRegressor", "ExtraTreesRegressor"):
        return list(est.estimators_), True
    if name in ("RandomForestClassifier", "ExtraTreesClassifier"):
        return list(est.estimators_), True
    if name in ("DecisionTreeRegressor", "DecisionTreeClassifier", "ExtraTreeRegressor",
                "ExtraTreeClassifier"):
        return [est], False
    raise TypeError(f"sklearn estimator {name} is not a supported tree ensemble "
                    "(RandomForest / ExtraTrees / DecisionTree)")


def forest_from_gradient_boosting(est) -> Forest:
    """GradientBoosting{Regressor,Classifier} (installed sklearn 1.7.2,
    ensemble/_gb.py:948-967 and _gradient_boosting.pyx:56-75, 164-205):

        raw[:, k] = init_raw[k];  for stage i, for k: raw[:, k] += learning_rate * value[leaf]

    in float64 with X converted to float32 and ``x <= threshold`` (NaN input is
    rejected by validate_data).  Each stage's K trees are output groups 0..K-1
    in stage order, and the leaf payload is ``learning_rate * value`` (the same
    double product the Cython loop forms), so the sums are bit-identical.  The
    init estimator must be 'zero' or a Dummy{Regressor,Classifier} (the
    default): its raw prediction is a constant per output, taken from the
    estimator itself.  predict: regressor raw; binary classifier raw >= 0
    (_gb.py:1612-1632, T_STEP); multiclass first argmax."""
    from sklearn.dummy import DummyClassifier, DummyRegressor
    init = est.init_
    if not (isinstance(init, str) and init == "zero") and \
            not isinstance(init, (DummyRegressor, DummyClassifier)):
        raise TypeError("GradientBoosting with a non-constant init estimator "
                        f"({type(init).__name__}) is not supported")
    stages = est.estimators_                       # [n_stages, K] DecisionTreeRegressor
    n_stages, K = stages.shape
    F = int(est.n_features_in_)
    base = np.asarray(est._raw_predict_init(np.zeros((1, F), dtype=np.float32))[0],
                      dtype=np.float64)
    lr = float(est.learning_rate)
    canon, groups = [], []
    for i in range(n_stages):
        for k in range(K):
            arr = tree_arrays_from_sklearn(stages[i, k].tree_)
            t = _canon_tree(arr, False, 1)
            t["flags"] = np.zeros_like(t["flags"])      # the GB traversal ignores missing_go_to_left
            leaf = t["feature"] < 0
            t["leaf_value"] = np.where(leaf[:, None], lr * arr["value"][:, 0, :1], 0.0)
            canon.append(t)
            groups.append(k)
    cat = concat_trees(canon, 1)
    classifier = hasattr(est, "classes_")
    if classifier:
        transform = T_STEP if K == 1 else T_ARGMAX
    else:
        transform = T_IDENTITY
    return Forest(
        n_features=F, n_groups=K, leaf_width=1, accum_dtype=TI_F64,
        base_first=True, lgb_zero_map=False,
        tree_offset=cat["tree_offset"], tree_group=np.asarray(groups, dtype=np.int32),
        feature=cat["feature"], threshold=cat["threshold"], flags=cat["flags"],
        left=cat["left"], right=cat["right"], leaf_id=cat["leaf_id"],
        leaf_value=cat["leaf_value"], base_margin=base, average_divisor=1.0, cover=cat["cover"],
        transform=transform, transform_param=1.0,
        input_dtype=TI_F32, library="sklearn", objective=type(est).__name__,
        meta={"classes": np.asarray(est.classes_) if classifier else None,
              "allow_nan": False},
    ).contiguous()


_HGB_NAMES = ("HistGradientBoostingRegressor", "HistGradientBoostingClassifier")
_HGB_NODE_FIELDS = ("value", "count", "feature_idx", "num_threshold", "missing_go_to_left",
                    "left", "right", "is_leaf", "is_categorical", "bitset_idx")
_HGB_MAX_CATEGORY = 1 << 24     # the XGBoost rule reads [0, 2^24) as categories


def _hgb_categories(est, is_cat: np.ndarray) -> dict:
    """Raw column -> the sorted raw categories the estimator's ordinal encoder
    learned (a trailing NaN dropped): a value's code is its index here.  They
    become bit positions of the canonical bitsets, so they must be integers in
    [0, 2^24) -- the range the XGBoost rule reads as categories at all."""
    enc = est._preprocessor.named_transformers_["encoder"]
    cols = np.flatnonzero(is_cat)
    if len(enc.categories_) != cols.size:
        raise TypeError("HistGradientBoosting encoder and is_categorical_ disagree "
                        "(a pickle of another sklearn version?)")
    out = {}
    for col, c in zip(cols, enc.categories_):
        c = np.asarray(c)
        if c.dtype.kind not in "fiub":
            raise ValueError(f"categorical feature {int(col)}: categories of dtype {c.dtype} are "
                             "not numeric (string categories are not supported)")
        c = c.astype(np.float64)
        c = c[~np.isnan(c)]
        if c.size and c.min() < 0:
            raise ValueError(f"categorical feature {int(col)}: negative category {c.min():g} "
                             "(categories must be integers in [0, 2^24))")
        if not np.all(c == np.floor(c)):
            bad = c[c != np.floor(c)][0]
            raise ValueError(f"categorical feature {int(col)}: non-integer category {bad:g} "
                             "(categories must be integers in [0, 2^24))")
        if c.size and c.max() >= _HGB_MAX_CATEGORY:
            raise ValueError(f"categorical feature {int(col)}: category {c.max():g} >= 2^24 "
                             "(categories must be integers in [0, 2^24))")
        out[int(col)] = c.astype(np.int64)
    return out



def _bitset_members(words: np.ndarray, n: int) -> np.ndarray:
    """Bits 0..n-1 of a uint32 bitset as booleans."""
    j = np.arange(n)
    return ((np.asarray(words, dtype=np.uint32)[j // 32] >> (j % 32).astype(np.uint32)) & 1) != 0


def forest_from_hist_gradient_boosting(est) -> Forest:
    """HistGradientBoosting{Regressor,Classifier} (installed sklearn 1.7.2,
    ensemble/_hist_gradient_boosting/gradient_boosting.py ``_raw_predict`` /
    ``_predict_iterations``, _predictor.pyx ``_predict_one_from_raw_data``):

        raw[:, k] = _baseline_prediction[0, k]
        for each iteration, for k: raw[:, k] += value[leaf]          (float64)

    with X kept in float64 (NaN and, on numerical columns, infinity allowed).
    A numerical node sends NaN to ``missing_go_to_left``'s side and otherwise
    goes left iff ``x <= num_threshold`` -- the canonical compare, +inf
    thresholds included.  The leaf payload is ``value`` (the learning rate is
    already in it), an iteration's K trees are output groups 0..K-1 in
    iteration order, so the sums are bit-identical.  predict: regressor the
    inverse link (identity, or exp for poisson / gamma); binary classifier
    ``raw > 0`` (T_HINGE, not GradientBoosting's ``>= 0``); multiclass first
    argmax.

    Categorical features: the estimator ordinal-encodes them (``_preprocessor``)
    and moves them to the front, so ``feature_idx`` is mapped back to the raw
    column and the code-space bitsets to raw-value space (bit C[j] for code j
    of the feature's sorted categories C).  sklearn's node goes left iff the
    code is in the node's left set, else right iff the category is known, else
    (NaN, unknown) to ``missing_go_to_left``'s side.  Both cases are the
    XGBoost rule (NaN by flag; x < 0 or x >= 2^24 left; in set right):

    * ``missing_go_to_left`` = 1: set = known & ~left, NAN_LEFT; left-set,
      unknown and invalid values all go left, where missing goes.
    * ``missing_go_to_left`` = 0: children swapped, set = left, NAN_LEFT; in
      set is the new right (old left), everything else the new left (old right).

    Categories must therefore be integers in [0, 2^24): a node's bitset is as
    long as its largest chosen category needs (at most 2 MiB), and no layout
    asks for a lower cap (a forest whose sets do not fit the categorical heap
    runs on the explicit kernel).  Anything else is refused here.

    One gap: a non-integer value on a categorical column (3.5) is an unknown
    category to sklearn, while the canonical rule truncates it (category 3).
    The serving layer replaces such values by NaN before the walk
    (SKLearnModel.request_matrix); callers of the engine itself must do the
    same.  TreeSHAP contributions (OUT_CONTRIB) of a model with categorical
    splits stay refused like every XGBoost-rule forest; OUT_CONTRIB_APPROX
    serves them."""
    from .xgboost_format import _concat_categories, _set_categorical
    try:
        predictors = est._predictors
        baseline = np.asarray(est._baseline_prediction, dtype=np.float64)
        pre = est._preprocessor
        is_cat = est.is_categorical_
        F = int(est.n_features_in_)
        K = int(est.n_trees_per_iteration_)
        classifier = hasattr(est, "classes_")
        link = None if classifier else type(est._loss.link).__name__
        known_sets = f_idx_map = None
        if pre is not None:
            known_sets, f_idx_map = est._bin_mapper.make_known_categories_bitsets()
        for it in predictors:
            for p in it:
                missing = [n for n in _HGB_NODE_FIELDS if n not in p.nodes.dtype.names]
                if missing:
                    raise AttributeError(f"predictor nodes lack {missing}")
                getattr(p, "raw_left_cat_bitsets")
    except AttributeError as e:
        raise TypeError(f"{type(est).__name__} lacks the private attributes of sklearn 1.7 "
                        f"this loader reads (a pickle of another sklearn version?): {e}") from e
    if baseline.shape != (1, K) or any(len(it) != K for it in predictors):
        raise TypeError(f"{type(est).__name__}: unexpected baseline / predictor shapes "
                        "(a pickle of another sklearn version?)")
    if pre is None:
        perm = np.arange(F)
        cats = {}
    else:
        is_cat = np.asarray(is_cat, dtype=bool)
        perm = np.concatenate([np.flatnonzero(is_cat), np.flatnonzero(~is_cat)])
        cats = _hgb_categories(est, is_cat)
    if classifier:
        transform = T_HINGE if K == 1 else T_ARGMAX
    elif link == "IdentityLink":
        transform = T_IDENTITY
    elif link == "LogLink":
        transform = T_EXP
    else:
        raise TypeError(f"{type(est).__name__} with link {link} is not supported")

    canon, groups = [], []
    for it in predictors:
        for k, p in enumerate(it):
            nd = p.nodes
            n = nd.shape[0]
            leaf = nd["is_leaf"] != 0
            mgl = nd["missing_go_to_left"] != 0
            iscat = ~leaf & (nd["is_categorical"] != 0)
            if iscat.any() and pre is None:
                raise TypeError("categorical nodes in an estimator without a preprocessor")
            fidx = np.where(leaf, 0, nd["feature_idx"]).astype(np.int64)
            if fidx.size and (fidx.min() < 0 or fidx.max() >= F):
                raise ValueError("split feature index outside the estimator's features")
            left = np.where(leaf, -1, nd["left"].astype(np.int64))
            right = np.where(leaf, -1, nd["right"].astype(np.int64))
            swap = iscat & ~mgl
            t = {
                "feature": np.where(leaf, -1, perm[fidx]),
                "threshold": np.where(leaf | iscat, 0.0, nd["num_threshold"]),
                "flags": np.where(~leaf & (mgl | iscat), NODE_NAN_LEFT, 0).astype(np.uint8),
                "left": np.where(swap, right, left),
                "right": np.where(swap, left, right),
                "leaf_id": np.arange(n),
                "leaf_value": np.where(leaf, nd["value"], 0.0)[:, None],
                "cover": nd["count"].astype(np.float64),
            }
            sets = {}
            for i in np.flatnonzero(iscat):
                C = cats[int(perm[fidx[i]])]
                chosen = _bitset_members(p.raw_left_cat_bitsets[int(nd["bitset_idx"][i])], C.size)
                if mgl[i]:
                    known = _bitset_members(known_sets[int(f_idx_map[fidx[i]])], C.size)
                    chosen = known & ~chosen
                sets[int(i)] = C[chosen]
            if sets:
                _set_categorical(t, sets)
            canon.append(t)
            groups.append(k)
    cat = concat_trees(canon, 1)
    cat_bits, cat_offset, cat_nwords = _concat_categories(canon)
    return Forest(
        n_features=F, n_groups=K, leaf_width=1, accum_dtype=TI_F64,
        base_first=True, lgb_zero_map=False,
        tree_offset=cat["tree_offset"], tree_group=np.asarray(groups, dtype=np.int32),
        feature=cat["feature"], threshold=cat["threshold"], flags=cat["flags"],
        left=cat["left"], right=cat["right"], leaf_id=cat["leaf_id"],
        leaf_value=cat["leaf_value"], base_margin=baseline[0].copy(), average_divisor=1.0,
        cover=cat["cover"], transform=transform, transform_param=1.0,
        input_dtype=TI_F64, library="sklearn", objective=type(est).__name__,
        cat_bits=cat_bits, cat_offset=cat_offset, cat_nwords=cat_nwords,
        meta={"classes": np.asarray(est.classes_) if classifier else None,
              "hist_gradient_boosting": True,
              # who validates the width: the ColumnTransformer when there is one
              "validator": type(est).__name__ if pre is None else type(pre).__name__,
              "categorical_features": np.flatnonzero(is_cat) if pre is not None
              else np.zeros(0, dtype=np.int64)},
    ).contiguous()


def _pipeline_step_ops(name: str, step, F: int) -> list:
    """(op, constants [F]) of one fitted Pipeline step, in the order the
    installed sklearn 1.7.2 applies them in ``transform`` (in place, on a copy
    of X in X's own float type):

        SimpleImputer   (impute/_base.py)       X[isnan(X)] = statistics_
        StandardScaler  (preprocessing/_data.py) X -= mean_ ; X /= scale_
        MinMaxScaler                             X *= scale_ ; X += min_
        MaxAbsScaler                             X /= scale_
        RobustScaler                             X -= center_ ; X /= scale_

    Anything the per-column op chain cannot restate is a TypeError naming the
    step."""
    cls = type(step).__name__
    where = f"Pipeline step '{name}' ({cls})"

    def const(a, what):
        a = np.asarray(a, dtype=np.float64)
        if a.shape != (F,):
            raise TypeError(f"{where}: {what} has shape {a.shape}, expected ({F},)")
        return a

    if getattr(step, "n_features_in_", F) != F:
        raise TypeError(f"{where} was fitted on {step.n_features_in_} columns, the final "
                        f"estimator on {F}")
    if cls == "SimpleImputer":
        mv = step.missing_values
        if not (isinstance(mv, float) and mv != mv):
            raise TypeError(f"{where}: missing_values={mv!r} is not supported (NaN only)")
        if step.add_indicator:
            raise TypeError(f"{where}: add_indicator=True adds columns and is not supported")
        stats = np.asarray(step.statistics_)
        if stats.dtype.kind not in "fiu" or stats.shape != (F,) or \
                not np.all(np.isfinite(stats.astype(np.float64))):
            raise TypeError(f"{where}: statistics_ must be {F} finite numbers (an imputer that "
                            "drops an all-missing column changes the column count)")
        return [(PRE_FILL_NAN, const(stats, "statistics_"))]
    if cls == "StandardScaler":
        ops = []
        if step.with_mean:
            ops.append((PRE_SUB, const(step.mean_, "mean_")))
        if step.with_std:
            ops.append((PRE_DIV, const(step.scale_, "scale_")))
        return ops
    if cls == "MinMaxScaler":
        if step.clip:
            raise TypeError(f"{where}: clip=True is not supported")
        return [(PRE_MUL, const(step.scale_, "scale_")), (PRE_ADD, const(step.min_, "min_"))]
    if cls == "MaxAbsScaler":
        return [(PRE_DIV, const(step.scale_, "scale_"))]
    if cls == "RobustScaler":
        ops = []
        if step.with_centering:
            ops.append((PRE_SUB, const(step.center_, "center_")))
        if step.with_scaling:
            ops.append((PRE_DIV, const(step.scale_, "scale_")))
        return ops
    raise TypeError(f"{where} is not a supported transformer (SimpleImputer / StandardScaler / "
                    "MinMaxScaler / MaxAbsScaler / RobustScaler)")


def forest_from_pipeline(pipe) -> Forest:
    """A fitted ``sklearn.pipeline.Pipeline`` of imputer / scaler steps in front
    of a tree ensemble this module flattens (HistGradientBoosting excepted):
    the final estimator's forest with the steps attached as pre-steps
    (include/treeinfer.h), which the engine applies on the device where X
    enters.  ``None`` / ``"passthrough"`` steps are skipped.

    The scalers keep float64 rows as float64 and float32 rows as float32 and
    work in that type, so the forest declares ``input_dtype`` TI_F64
    (prepare_input then keeps both) and each pre-step rounds to the element
    type; the final estimator's own float32 cast is the pre-pass's last
    conversion.  ``meta["validator"]`` names the first real step: it is the one
    whose width check answers a request of the wrong shape."""
    steps = list(pipe.steps)
    if not steps:
        raise TypeError("Pipeline has no steps")
    last_name, last = steps[-1]
    lcls = type(last).__name__
    if last is None or isinstance(last, str):
        raise TypeError(f"Pipeline final step '{last_name}' is {last!r}, not an estimator")
    if lcls == "Pipeline":
        raise TypeError(f"Pipeline final step '{last_name}' (Pipeline): nested pipelines are not "
                        "supported")
    if lcls in _HGB_NAMES:
        raise TypeError(f"Pipeline final step '{last_name}' ({lcls}): HistGradientBoosting keeps "
                        "float64 input and is not supported behind pipeline steps")
    try:
        forest = forest_from_sklearn(last)
    except TypeError as e:
        raise TypeError(f"Pipeline final step '{last_name}' ({lcls}): {e}") from e
    F = forest.n_features
    ops, first = [], None
    for name, step in steps[:-1]:
        if step is None or (isinstance(step, str) and step == "passthrough"):
            continue
        if first is None:
            first = type(step).__name__
        ops += _pipeline_step_ops(name, step, F)
    if len(ops) > PRE_MAX_STEPS:
        raise TypeError(f"Pipeline flattens to {len(ops)} per-column operations, at most "
                        f"{PRE_MAX_STEPS} are supported")
    if ops:
        forest.pre_ops = np.asarray([o for o, _ in ops], dtype=np.int32)
        forest.pre_consts = np.stack([c for _, c in ops])
        forest.input_dtype = TI_F64
    # no real step: the final estimator's own float32 cast is all there is
    forest.meta["pipeline"] = True
    forest.meta["validator"] = first if first is not None else forest.objective
    forest.meta["imputes"] = any(o == PRE_FILL_NAN for o, _ in ops)
    return forest.contiguous()


def forest_from_sklearn(est) -> Forest:
    """Flatten a fitted sklearn tree ensemble, or a Pipeline that ends in one."""
    if type(est).__name__ == "Pipeline":
        return forest_from_pipeline(est)
    if type(est).__name__ in _HGB_NAMES:
        return forest_from_hist_gradient_boosting(est)
    if type(est).__name__ in ("GradientBoostingRegressor", "GradientBoostingClassifier"):
        return forest_from_gradient_boosting(est)
    members, average = _estimators(est)
    if getattr(est, "n_outputs_", 1) != 1:
        raise ValueError("multi-output sklearn models are not supported")
    classifier = hasattr(est, "classes_")
    n_classes = int(est.n_classes_) if classifier else 1
    trees = [tree_arrays_from_sklearn(m.tree_) for m in members]
    return forest_from_tree_arrays(trees, est.n_features_in_, classifier, n_classes,
                                   average=average,
                                   classes=getattr(est, "classes_", None),
                                   kind=type(est).__name__)


def save_tree_arrays(path: str, est) -> None:
    """Store a fitted ensemble's raw tree arrays as .npz (no pickle)."""
    members, average = _estimators(est)
    classifier = hasattr(est, "classes_")
    payload = {
        "n_trees": np.int64(len(members)),
        "n_features": np.int64(est.n_features_in_),
        "classifier": np.int64(classifier),
        "average": np.int64(average),
        "n_classes": np.int64(est.n_classes_ if classifier else 1),
        "kind": np.array(type(est).__name__),
    }
    if classifier:
        payload["classes"] = np.asarray(est.classes_)
    for i, m in enumerate(members):
        for k, v in tree_arrays_from_sklearn(m.tree_).items():
            payload[f"t{i}_{k}"] = v
    np.savez_compressed(path, **payload)


def load_tree_arrays(path: str) -> Forest:
    """Inverse of :func:`save_tree_arrays` (numpy.load, allow_pickle=False)."""
    z = np.load(path, allow_pickle=False)
    T = int(z["n_trees"])
    keys = ("children_left", "children_right", "feature", "threshold", "missing_go_to_left",
            "value", "cover")
    trees = [{k: z[f"t{i}_{k}"] for k in keys if f"t{i}_{k}" in z.files} for i in range(T)]
    classifier = bool(int(z["classifier"]))
    return forest_from_tree_arrays(trees, int(z["n_features"]), classifier,
                                   int(z["n_classes"]), average=bool(int(z["average"])),
                                   classes=z["classes"] if "classes" in z.files else None,
                                   kind=str(z["kind"]))
