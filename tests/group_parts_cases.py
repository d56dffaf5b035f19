"""The forests, batches and references on which forests of more than 16 output
groups ("group parts": create_chunked / launch_chunked in treeinfer.hip) are
held to their references on repeated calls of one handle: shared by
tests/test_group_parts_cases.py (CPU: the conditions that keep the GPU tests
from passing by accident) and tests/test_gpu_group_parts.py.

A case is named by what it reaches:

    k17-design     xgb(17, 2, 5, seed=6, K=17), the forest DESIGN.md recorded
                   wrong contributions on.  Parts of 16 + 1 groups; a part's
                   row is 96 columns: contrib_reg_kernel, 64 paths, no slices.
    k20-sliced     XGBoost float32, K = 20, F = 6, 3 depth-4 trees a group.
                   Parts of 16 + 4; 112 columns; the first part has 768 paths,
                   so it can take path slices (TI_SHAP_SLICES).
    k33-generic    XGBoost float32, K = 33, F = 8, 2 depth-4 trees a group.
                   Parts of 16 + 16 + 1; 144 columns > kShapLdsW, so the
                   16-group parts take the generic contrib_kernel (its own
                   accumulator scratch and memset).
    lgb-k18-f64    LightGBM multiclass, K = 18, F = 6, 2 trees of 15 leaves a
                   class: float64 accumulators, 8-byte columns, the zero and
                   NaN missing types.  Parts of 16 + 2.
    sk-k20-vector  sklearn RandomForestClassifier, 20 classes, F = 6, 16 trees of
                   15 leaves: vector leaves, so every part holds every tree and
                   TI_OUTPUT_LEAF takes launch_chunked's early return.  Parts
                   of 16 + 4.

Rows are float64 values that float32 holds exactly (as in
tests/shap_interact_cases.py), so one reference serves the float32 and the
float64 input of a case.  A call sequence is SIZES with one seed a call: the
batches of a sequence all differ, because with the same batch the previous
call's output left in a buffer cannot be told from a right answer.

k16-one-part is k20-sliced's shape with 16 groups, one part: the torch-free
child (tests/group_parts_child.py) runs it on successive handles of a process.
Calls go through shap_interact_cases.predict (`ic.predict`).

References are computed once per (case, kind, batch) and cached read-only:
margins, predictions and leaf ids by the library restatements (oracle/xgb_ref,
oracle/lgb_ref) or sklearn itself, which tests/test_group_parts_cases.py holds
equal to tests/canon_eval.py; contributions by oracle/shap_ref, approximate
contributions by tests/saabas_eval, interactions by tests/shap_interact_eval.
No batch is larger than 257 rows."""
from __future__ import annotations

import dataclasses
import functools
import os
import tempfile

import numpy as np

from kfserving_amd.forest import (OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_INTERACT, OUT_LEAF,
                                  OUT_MARGIN, OUT_PREDICT, TI_F32, TI_F64)
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from oracle import lgb_ref, shap_ref, xgb_ref
from tests import saabas_eval as sa
from tests import shap_cat_eval as sc
from tests import shap_interact_eval as si

MAX_GROUPS = 16                               # ti::kMaxGroups: the groups of one part
LDS_W = 128                                   # kShapLdsW: the widest row contrib_reg_kernel takes
SIZES = (70, 6, 70, 1, 257, 8, 64, 65)        # DESIGN's failing sizes, a big one, the 64-row wave edge

GENERATED = ["k20-sliced", "k33-generic", "lgb-k18-f64", "sk-k20-vector"]
CASES = ["k17-design"] + GENERATED


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    forest: object
    lib: str            # "xgb", "lgb" or "sk": whose restatement `model` is
    model: object       # XGBRefModel, LGBRefModel or the fitted estimator
    seeds: tuple        # the batch seed of each call of SIZES (chosen: test_group_parts_cases.py)
    split: tuple        # the groups of each part, as the case states them


def _xgb_case(name, n_trees, depth, F, seed, K, seeds, split, objective="multi:softprob"):
    trees, ti = xf.synthetic_complete_trees(n_trees, depth, F, seed=seed, num_class=K)
    f = xf.forest_from_raw_trees(trees, ti, F, K, 0.5, objective)
    return Case(name, f, "xgb", xgb_ref.from_raw_trees(trees, ti, F, K, 0.5, objective), seeds, split)


def _lgb_case(name, K, per_class, leaves, F, seed, seeds, split):
    trees = lf.synthetic_leafwise_trees(K * per_class, leaves, F, seed=seed)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.txt")
        lf.write_lightgbm_text(p, trees, F, f"multiclass num_class:{K}", num_class=K)
        return Case(name, lf.load_lightgbm_model(p), "lgb", lgb_ref.read_lgb_text(p), seeds, split)


def _sk_case(name, seeds, split):
    from sklearn.ensemble import RandomForestClassifier
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    rng = np.random.default_rng(7)
    X = rng.standard_normal((2000, 6)).astype(np.float32)
    # 20 equal classes along a direction every feature has a share in, and one
    # candidate feature a split: balanced leaves on all six features.  16
    # estimators, not 5: the margins of a row are its leaf in every tree, and 5
    # trees of 15 leaves give 257 rows about 100 distinct rows of margins (16
    # give 254-257, so seeds exist at which every row differs)
    w = rng.standard_normal(6)
    y = np.argsort(np.argsort(X @ w)) * 20 // len(X)
    est = RandomForestClassifier(n_estimators=16, max_leaf_nodes=15, max_features=1,
                                 random_state=0).fit(X, y)
    assert len(est.classes_) == 20
    return Case(name, forest_from_sklearn(est), "sk", est, seeds, split)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    if name == "k17-design":                  # DESIGN's reproducer, exactly (shap_interact_cases.xgb)
        return _xgb_case(name, 17, 2, 5, 6, 17, tuple(range(1700, 1708)), (16, 1))
    if name == "k20-sliced":
        return _xgb_case(name, 60, 4, 6, 51, 20, tuple(range(2001, 2009)), (16, 4))
    if name == "k20-softmax":                 # the same trees behind the argmax transform
        return _xgb_case(name, 60, 4, 6, 51, 20, tuple(range(2001, 2009)), (16, 4), "multi:softmax")
    if name == "k16-one-part":                # 16 groups: no group part, launch_chunked not reached;
        # 112 columns and 768 paths, so contrib_reg_kernel with path slices
        return _xgb_case(name, 48, 4, 6, 51, 16, tuple(range(1600, 1608)), (16,))
    if name == "k33-generic":
        return _xgb_case(name, 66, 4, 8, 66, 33, tuple(range(3300, 3308)), (16, 16, 1))
    if name == "lgb-k18-f64":
        return _lgb_case(name, 18, 2, 15, 6, 9, tuple(range(1800, 1808)), (16, 2))
    if name == "sk-k20-vector":
        return _sk_case(name, (2101, 2102, 2105, 2106, 2109, 2110, 2111, 2112), (16, 4))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def batch(name, n, seed):
    """[n, F] float64 rows holding float32 values (sklearn: no NaN), read-only."""
    c = case(name)
    X = sc.rows(c.forest, n, seed=seed, n_categories=0).astype(np.float32).astype(np.float64)
    if c.lib == "sk":
        X[np.isnan(X)] = 0.25                 # sklearn trees: no missing values
    X.setflags(write=False)
    return X


def sequence(name):
    """The (rows, seed) of the case's call sequence: SIZES, one seed a call, so
    every batch differs.  The seeds are those at which no misplaced block can
    hide (tests/test_group_parts_cases.py holds them to that)."""
    return tuple(zip(SIZES, case(name).seeds))


# DESIGN's reproducer on k17-design: six 70-row batches in whose 16-group part
# every row differs, and six 6-row batches
K17_70 = tuple((70, s) for s in (1700, 1702, 1710, 1711, 1713, 1714))
K17_6 = tuple((6, s) for s in range(1720, 1726))
K17_257 = tuple((257, s) for s in range(1730, 1736))      # the two-slot test's


def reference(name, kind, X):
    """The reference of `kind` on rows X, [rows, width] (labels: [rows])."""
    c = case(name)
    f = c.forest
    X = np.asarray(X, dtype=np.float64)
    if kind == OUT_CONTRIB:
        return shap_ref.contributions(f, X)
    if kind == OUT_CONTRIB_APPROX:
        return sa.contributions(f, X)
    if kind == OUT_INTERACT:
        return si.interactions(f, X).reshape(len(X), -1)
    if c.lib == "xgb":
        X32 = X.astype(np.float32)
        if kind == OUT_LEAF:
            return xgb_ref.leaf_index(c.model, X32)
        return xgb_ref.predict(c.model, X32, output_margin=kind == OUT_MARGIN)
    if c.lib == "lgb":
        if kind == OUT_LEAF:
            return lgb_ref.leaf_index(c.model, X)
        return lgb_ref.predict(c.model, X, raw_score=kind == OUT_MARGIN)
    X32 = X.astype(np.float32)
    if kind == OUT_LEAF:
        return c.model.apply(X32)
    if kind == OUT_MARGIN:
        return c.model.predict_proba(X32)
    return np.searchsorted(f.meta["classes"], c.model.predict(X32)).astype(np.float64)   # class index


@functools.lru_cache(maxsize=None)
def want(name, kind, n, seed):
    w = np.asarray(reference(name, kind, batch(name, n, seed)))
    w.setflags(write=False)
    return w


def parts(f):
    """[(first group, groups)] of the forest's parts: K cut every MAX_GROUPS."""
    return [(k0, min(MAX_GROUPS, f.n_groups - k0)) for k0 in range(0, f.n_groups, MAX_GROUPS)]


def part_columns(f, kind, k0, kc):
    """The output columns of `kind` that the part of groups k0 .. k0 + kc - 1
    writes, or None where the output is not assembled from parts (labels; the
    leaf ids of vector leaves, which the first part alone answers)."""
    cw = {OUT_MARGIN: 1, OUT_PREDICT: 1, OUT_CONTRIB: f.n_features + 1,
          OUT_CONTRIB_APPROX: f.n_features + 1, OUT_INTERACT: (f.n_features + 1) ** 2}
    if kind == OUT_LEAF:
        if f.leaf_width != 1:
            return None
        g = np.asarray(f.tree_group)
        return np.nonzero((g >= k0) & (g < k0 + kc))[0]
    if kind == OUT_PREDICT and f.output_width(kind) == 1:
        return None
    return np.arange(k0 * cw[kind], (k0 + kc) * cw[kind])


def bound(f, kind):
    """The project's bound of a kind: None bit-exact, ("rtol", 1e-5)
    probabilities (tests/test_gpu_many_groups.py), ("scaled", b) contributions
    (tests/test_gpu_shap.py), approximate contributions
    (tests/test_gpu_approx_contrib.py) and interactions
    (tests/test_gpu_shap_interact.py)."""
    f32 = f.accum_dtype == TI_F32
    if kind in (OUT_MARGIN, OUT_LEAF):
        return None
    if kind == OUT_PREDICT:
        return None if f.output_width(kind) == 1 else ("rtol", 1e-5)
    if kind == OUT_INTERACT:
        return ("scaled", 1e-6 if f32 else 1e-14)
    return ("scaled", 1e-6 if f32 else 1e-9)


def wrong_elements(f, kind, got, w):
    """Boolean [rows, width]: the elements of `got` outside the kind's bound."""
    got = np.asarray(got).reshape(len(w), -1)
    w = np.asarray(w).reshape(len(w), -1)
    assert got.shape == w.shape, (got.shape, w.shape)
    b = bound(f, kind)
    if b is None:
        return ~((got == w) | (np.isnan(got.astype(np.float64)) & np.isnan(w.astype(np.float64))))
    g64, w64 = got.astype(np.float64), w.astype(np.float64)
    if b[0] == "rtol":
        return ~(np.abs(g64 - w64) <= b[1] * np.abs(w64))
    scale = np.maximum(np.abs(w64).max(axis=1, keepdims=True), 1.0)
    return ~(np.abs(g64 - w64) / scale <= b[1])


def describe_wrong(f, kind, bad):
    """Where a call went wrong: how many elements, the row range, and the parts
    whose columns hold them."""
    rows = np.nonzero(bad.any(axis=1))[0]
    where = []
    for c, (k0, kc) in enumerate(parts(f)):
        cols = part_columns(f, kind, k0, kc)
        if cols is not None and bad[:, cols].any():
            where.append(f"part {c} (groups {k0}..{k0 + kc - 1})")
    return (f"{int(bad.sum())} of {bad.size} values wrong, rows {rows[0]}..{rows[-1]} "
            f"({len(rows)} rows), in {', '.join(where) or 'the whole row'}")
