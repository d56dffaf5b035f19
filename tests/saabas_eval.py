"""CPU reference for approximate (Saabas) contributions
(TI_OUTPUT_CONTRIB_APPROX, xgboost's approx_contribs), for the tests only.

Per tree, mean[n] is the leaf value at a leaf and the cover-weighted mean of
the children's means elsewhere (xgboost FillNodeMeanValues, the recursion of
``tests/shap_cat_eval._bias``).  A row that walks root = n0 -> n1 -> ... -> leaf
adds mean[n(i+1)] - mean[n(i)] to column feature[n(i)] and mean[root] to the
bias column; the base margin goes in the bias and everything is divided by the
average divisor, as ``tests/shap_cat_eval.contributions`` does.

The walk takes ``tests/shap_cat_eval.decisions`` (every split rule of
include/treeinfer.h, both categorical ones through ``canon_eval.cat_left``) and
adds node by node in float64.  It never forms the per-leaf lists of merged
terms the device builds, so the two agree only by both being right.
"""
from __future__ import annotations

import numpy as np

from tests import shap_cat_eval as sc


def node_means(f) -> np.ndarray:
    """[N, leaf_width] float64 mean of every node's subtree."""
    LW = f.leaf_width
    mean = np.zeros((f.n_nodes, LW))
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        order = [0]
        for v in order:                       # preorder: parents before children
            g = b + v
            if f.feature[g] >= 0:
                order += [int(f.left[g]), int(f.right[g])]
        for v in reversed(order):
            g = b + v
            if f.feature[g] < 0:
                mean[g] = np.asarray(f.leaf_value[g], dtype=np.float64).reshape(LW)
            else:
                l, r = b + int(f.left[g]), b + int(f.right[g])
                mean[g] = (mean[l] * f.cover[l] + mean[r] * f.cover[r]) / f.cover[g]
    return mean


def contributions(f, X: np.ndarray) -> np.ndarray:
    """[rows, K * (F + 1)] float64, laid out as TI_OUTPUT_CONTRIB."""
    if f.cover is None:
        raise ValueError("forest has no node covers")
    F, K, LW = f.n_features, f.n_groups, f.leaf_width
    X = np.asarray(X, dtype=np.float64)
    left = sc.decisions(f, X)
    mean = node_means(f)
    out = np.zeros((X.shape[0], K, F + 1))
    out[:, :, F] = np.asarray(f.base_margin, dtype=np.float64) * f.average_divisor
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        groups = [int(f.tree_group[t])] if LW == 1 else list(range(K))
        out[:, groups, F] += mean[b]
        for r in range(X.shape[0]):
            v = 0
            while f.feature[b + v] >= 0:
                g = b + v
                c = int(f.left[g]) if left[r, g] else int(f.right[g])
                out[r, groups, int(f.feature[g])] += mean[b + c] - mean[g]
                v = c
    return (out / f.average_divisor).reshape(X.shape[0], K * (F + 1))


def scaled_error(got, want) -> float:
    """max |got - want| / max(largest |want| of the row, 1): the contributions'
    error measure (tests/test_gpu_shap.py)."""
    got = np.asarray(got, dtype=np.float64).reshape(len(want), -1)
    want = np.asarray(want, dtype=np.float64).reshape(len(want), -1)
    scale = np.maximum(np.abs(want).max(axis=1, keepdims=True), 1.0)
    return float((np.abs(got - want) / scale).max()) if want.size else 0.0
