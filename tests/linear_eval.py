"""CPU reference for LightGBM linear-tree models (LightGBM 3.2 - 4.x
``Tree::Predict`` with ``is_linear_``), for the tests only.

It works from the model text alone: the ``Tree=`` blocks are read here, the
reached leaves come from ``oracle.lgb_ref``'s scalar walk of the text's own
split arrays, and the linear models are evaluated as upstream does -- one
float64 multiply and one float64 add per term, in file order, vectorised over
rows (numpy does not fuse).  Nothing here knows ``Forest``'s linear arrays.

    out = leaf_const[j]
    for i in 0 .. m_j - 1:
        v = x[leaf_features[j][i]]
        if isnan(v): return leaf_value[j]       # the whole leaf falls back
        out = out + leaf_coeff[j][i] * v
    return out
"""
from __future__ import annotations

import os
import tempfile
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from oracle import lgb_ref


@dataclass
class LinearTree:
    is_linear: bool
    leaf_value: np.ndarray
    leaf_const: Optional[np.ndarray] = None
    leaf_features: Optional[List[np.ndarray]] = None   # per leaf
    leaf_coeff: Optional[List[np.ndarray]] = None      # per leaf


def read_linear_blocks(text: str) -> List[LinearTree]:
    """The linear part of every ``Tree=`` block of a model text."""
    trees: List[LinearTree] = []
    block = None
    blocks = []
    for raw in text.splitlines():
        line = raw.strip()
        if line.startswith("Tree="):
            block = {}
            blocks.append(block)
        elif line == "end of trees":
            break
        elif block is not None and "=" in line:
            k, v = line.split("=", 1)
            block[k] = v
    for b in blocks:
        lv = np.array([float(v) for v in b["leaf_value"].split()], dtype=np.float64)
        if b.get("is_linear", "0").strip() in ("", "0"):
            trees.append(LinearTree(False, lv))
            continue
        const = np.array([float(v) for v in b["leaf_const"].split()], dtype=np.float64)
        counts = [int(v) for v in b["num_features"].split()]
        feats = [int(v) for v in b.get("leaf_features", "").split()]
        coeffs = [float(v) for v in b.get("leaf_coeff", "").split()]
        assert len(const) == len(lv) == len(counts)
        assert len(feats) == len(coeffs) == sum(counts)
        pf, pc, at = [], [], 0
        for m in counts:
            pf.append(np.array(feats[at:at + m], dtype=np.int64))
            pc.append(np.array(coeffs[at:at + m], dtype=np.float64))
            at += m
        trees.append(LinearTree(True, lv, const, pf, pc))
    return trees


def _model_of_text(text: str) -> lgb_ref.LGBRefModel:
    fd, path = tempfile.mkstemp(suffix=".txt")
    try:
        with os.fdopen(fd, "w") as fh:
            fh.write(text)
        return lgb_ref.read_lgb_text(path)
    finally:
        os.remove(path)


def tree_outputs(text: str, X: np.ndarray):
    """(per-tree outputs [rows, T] float64, fallback flags [rows, T] bool,
    leaves [rows, T]) of the model ``text`` on ``X`` ([rows, n_cols]; float32
    is widened exactly; columns the model reads past ``n_cols`` are NaN)."""
    model = _model_of_text(text)
    lin = read_linear_blocks(text)
    assert len(lin) == len(model.trees)
    X = np.asarray(X)
    assert X.ndim == 2
    X = X.astype(np.float64)
    n_feat = int(model.header.get("max_feature_idx", "-1")) + 1
    for t in lin:
        if t.is_linear:
            for f in t.leaf_features:
                if f.size:
                    n_feat = max(n_feat, int(f.max()) + 1)
    if X.shape[1] < n_feat:       # missing columns read as NaN
        X = np.concatenate([X, np.full((X.shape[0], n_feat - X.shape[1]), np.nan)], axis=1)
    leaves = lgb_ref.leaf_index(model, X)
    # the predictor's row fill: |x| <= 1e-35f reads 0.0, NaN stays
    Xz = np.where((np.abs(X) > lgb_ref.K_ZERO_THRESHOLD) | np.isnan(X), X, 0.0)
    rows = X.shape[0]
    out = np.zeros((rows, len(lin)), dtype=np.float64)
    fell = np.zeros((rows, len(lin)), dtype=bool)
    ridx = np.arange(rows)
    for t, tr in enumerate(lin):
        leaf = leaves[:, t]
        if not tr.is_linear:
            out[:, t] = tr.leaf_value[leaf]
            continue
        counts = np.array([f.shape[0] for f in tr.leaf_features], dtype=np.int64)
        mmax = int(counts.max()) if counts.size else 0
        # padded [leaf, term] tables; a row past its leaf's count is masked
        pf = np.zeros((len(counts), max(mmax, 1)), dtype=np.int64)
        pc = np.zeros((len(counts), max(mmax, 1)), dtype=np.float64)
        for j, (f, c) in enumerate(zip(tr.leaf_features, tr.leaf_coeff)):
            pf[j, :f.shape[0]] = f
            pc[j, :c.shape[0]] = c
        acc = tr.leaf_const[leaf].copy()
        nan_found = np.zeros(rows, dtype=bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(mmax):
                on = (i < counts[leaf]) & ~nan_found
                v = Xz[ridx, pf[leaf, i]]
                nan_found |= on & np.isnan(v)
                on &= ~nan_found
                prod = pc[leaf, i] * v             # one multiply ...
                acc = np.where(on, acc + prod, acc)   # ... then one add
        out[:, t] = np.where(nan_found, tr.leaf_value[leaf], acc)
        fell[:, t] = nan_found
    return out, fell, leaves


def raw_scores(text: str, X: np.ndarray):
    """(raw scores [rows, K] float64, fallback flags [rows, T]): the trees'
    outputs summed in tree order into group t mod K (GBDT::PredictRaw)."""
    model = _model_of_text(text)
    K = model.num_tree_per_iteration
    per_tree, fell, _ = tree_outputs(text, X)
    score = np.zeros((per_tree.shape[0], K), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(per_tree.shape[1]):
            score[:, t % K] += per_tree[:, t]
        if model.average_output:
            score /= per_tree.shape[1] // K
    return score, fell


def predict(text: str, X: np.ndarray) -> np.ndarray:
    """Transformed scores (ConvertOutput of the model's objective)."""
    model = _model_of_text(text)
    score, _ = raw_scores(text, X)
    with np.errstate(invalid="ignore", over="ignore"):
        return lgb_ref.convert_output(model.objective, score)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-for-bit equality of two float64 arrays, NaN equal to NaN (the sign
    and payload of 0 * inf differ between x86 and the GPU)."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    if not np.array_equal(an, bn):
        return False
    return np.array_equal(a.view(np.uint64)[~an], b.view(np.uint64)[~an])
