"""CPU reference for interventional TreeSHAP (TI_OUTPUT_CONTRIB_INTERV), tests
only: the definition by brute force over all feature subsets, in float64.

    phi_i(x) = sum_{S in F \\ i} |S|! (F - |S| - 1)! / F!
               mean_z [ f(x_{S+i}, z_rest) - f(x_S, z_rest) ],  bias = mean_z f(z)
A node reads one feature, so the hybrid row's turn at a node is x's when the
node's feature is in S and z's otherwise: the turns come from
tests/shap_cat_eval.decisions (the canonical split rule) and f is a plain
node-by-node walk of the Forest arrays.  No path, merged element or weight
table is formed.  Exponential in F."""
import math

import numpy as np

from tests import shap_cat_eval as sc


def margins(f, left: np.ndarray) -> np.ndarray:
    """[M, K] margins of M rows given their turn at every node ([M, N] bool)."""
    M = left.shape[0]
    idx = np.arange(M)
    out = np.zeros((M, f.n_groups))
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        v = np.zeros(M, dtype=np.int64)
        while True:
            g = b + v
            internal = f.feature[g] >= 0
            if not internal.any():
                break
            nxt = np.where(left[idx, g], f.left[g], f.right[g])
            v = np.where(internal, nxt, v)
        lv = f.leaf_value[b + v]
        if f.leaf_width == 1:
            out[:, int(f.tree_group[t])] += lv[:, 0]
        else:
            out += lv
    return np.asarray(f.base_margin, dtype=np.float64)[None, :] + out / f.average_divisor


def contributions(f, X: np.ndarray, Z: np.ndarray) -> np.ndarray:
    """[rows, K * (F + 1)] float64, laid out as TI_OUTPUT_CONTRIB."""
    F, K = f.n_features, f.n_groups
    X = np.asarray(X, dtype=np.float64)
    Z = np.asarray(Z, dtype=np.float64)
    R, B = X.shape[0], Z.shape[0]
    dx = np.repeat(sc.decisions(f, X), B, axis=0)        # pair (r, b) at r * B + b
    dz = np.tile(sc.decisions(f, Z), (R, 1))
    node_feature = np.maximum(f.feature, 0)
    v = np.empty((1 << F, R, K))                          # v[S] = mean_z f(x_S, z_rest)
    for S in range(1 << F):
        from_x = ((S >> node_feature) & 1).astype(bool)
        v[S] = margins(f, np.where(from_x[None, :], dx, dz)).reshape(R, B, K).mean(axis=1)
    out = np.zeros((R, K, F + 1))
    for i in range(F):
        for S in range(1 << F):
            if (S >> i) & 1:
                continue
            s = bin(S).count("1")
            w = math.factorial(s) * math.factorial(F - s - 1) / math.factorial(F)
            out[:, :, i] += w * (v[S | (1 << i)] - v[S])
    out[:, :, F] = v[0]
    return out.reshape(R, K * (F + 1))
