"""CPU reference for SHAP interaction values (TI_OUTPUT_INTERACT), for the
tests only.

The float64 conditioned recursion of xgboost's ``TreeShap(condition,
condition_feature)`` on the canonical ``Forest``: the recursion of
``tests/shap_cat_eval.py`` (ExtendPath at every node, UnwindPath where a
feature comes back, UnwoundPathSum at the leaves) with one feature conditioned
*on* (+1: its splits follow the row, it never joins the path, the cold subtree
is dropped) or *off* (-1: both children are walked, weighted by their cover
fractions, and it never joins the path).  As ``PredictInteractionContributions``
does, per tree and conditioned feature j,

    Phi[j][i] = (phi_i | j on  -  phi_i | j off) / 2          for i != j
    Phi[j][j] = phi_j - sum over i != j of Phi[j][i]
    Phi[F][F] = bias, the rest of the bias row and column zero

The hot child of a node comes from ``shap_cat_eval.decisions`` (``canon_eval``
at categorical nodes), so LightGBM categorical forests are covered.  It walks
the tree itself and never forms the merged per-feature path elements the
device tables hold.

:func:`brute_force` is the Shapley interaction index of the same
path-dependent value function by subset enumeration (Fujimoto et al. 2006;
Lundberg et al. 2018, eq. 8), for forests of a few features;
tests/test_shap_interact_eval.py pins the recursion to it.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

from tests import shap_cat_eval as sc


def _tree_shap_cond(f, t: int, left, phi: np.ndarray, condition: int, cond_feature: int) -> None:
    """Add tree t's contributions of one row into phi [F, leaf_width], with
    ``cond_feature`` conditioned on (condition = 1), off (-1) or, with
    condition = 0, not at all (the plain contributions)."""
    b = int(f.tree_offset[t])
    feature, lc, rc, cover, leaf_value = f.feature, f.left, f.right, f.cover, f.leaf_value

    def rec(v, fi, zf, of, pw, pz, po, pf, cfrac):
        if cfrac == 0.0:
            return
        if condition == 0 or pf != cond_feature:
            # ExtendPath with (pz, po, pf)
            d = len(fi)
            fi = fi + [pf]
            zf = zf + [pz]
            of = of + [po]
            pw = pw + [1.0 if d == 0 else 0.0]
            for i in range(d - 1, -1, -1):
                pw[i + 1] += po * pw[i] * (i + 1) / (d + 1)
                pw[i] = pz * pw[i] * (d - i) / (d + 1)
        d = len(fi) - 1                      # unique depth
        g = b + v
        if feature[g] < 0:
            lv = leaf_value[g]
            for k in range(1, d + 1):
                o, z = of[k], zf[k]
                nxt = pw[d]
                total = 0.0
                for i in range(d - 1, -1, -1):
                    if o != 0:
                        tmp = nxt * (d + 1) / ((i + 1) * o)
                        total += tmp
                        nxt = pw[i] - tmp * z * (d - i) / (d + 1)
                    else:
                        total += (pw[i] / z) / ((d - i) / (d + 1))
                phi[fi[k]] += total * (o - z) * cfrac * lv
            return
        fe = int(feature[g])
        l, r = int(lc[g]), int(rc[g])
        hot, cold = (l, r) if left[g] else (r, l)
        w = cover[g]
        hz, cz = cover[b + hot] / w, cover[b + cold] / w
        iz, io = 1.0, 1.0
        if fe in fi[1:]:
            # UnwindPath: the feature's earlier element leaves the path
            k = fi.index(fe, 1)
            iz, io = zf[k], of[k]
            pw = list(pw)
            nxt = pw[d]
            for i in range(d - 1, -1, -1):
                if io != 0:
                    tmp = pw[i]
                    pw[i] = nxt * (d + 1) / ((i + 1) * io)
                    nxt = tmp - pw[i] * iz * (d - i) / (d + 1)
                else:
                    pw[i] = (pw[i] * (d + 1)) / (iz * (d - i))
            fi = fi[:k] + fi[k + 1:]
            zf = zf[:k] + zf[k + 1:]
            of = of[:k] + of[k + 1:]
            pw = pw[:d]
        hot_c = cold_c = cfrac
        if condition > 0 and fe == cond_feature:
            cold_c = 0.0
        elif condition < 0 and fe == cond_feature:
            hot_c *= hz
            cold_c *= cz
        rec(hot, fi, zf, of, pw, hz * iz, io, fe, hot_c)
        rec(cold, fi, zf, of, pw, cz * iz, 0.0, fe, cold_c)

    # the root's dummy element has feature -1, which is never conditioned
    rec(0, [], [], [], [], 1.0, 1.0, -1, 1.0)


def _used(f, t):
    return sorted({int(v) for v in f.feature[f.tree_slice(t)] if v >= 0})


def contributions(f, X: np.ndarray) -> np.ndarray:
    """The unconditioned recursion, [rows, K * (F + 1)] (a check of this
    module against shap_cat_eval.contributions)."""
    F, K, LW = f.n_features, f.n_groups, f.leaf_width
    X = np.asarray(X, dtype=np.float64)
    left = sc.decisions(f, X)
    out = np.zeros((X.shape[0], K, F + 1))
    for r in range(X.shape[0]):
        row = left[r].tolist()
        for t in range(f.n_trees):
            phi = np.zeros((F, LW))
            _tree_shap_cond(f, t, row, phi, 0, -1)
            if LW == 1:
                out[r, int(f.tree_group[t]), :F] += phi[:, 0]
            else:
                out[r, :, :F] += phi.T
    out[:, :, F] = sc._bias(f)
    return (out / f.average_divisor).reshape(X.shape[0], K * (F + 1))


def _finish(f, out):
    """bias corner and divisor of [rows, K, F + 1, F + 1] feature blocks."""
    F = f.n_features
    out[:, :, F, F] = sc._bias(f)
    return out / f.average_divisor


def interactions(f, X: np.ndarray) -> np.ndarray:
    """[rows, K, F + 1, F + 1] float64 SHAP interaction values."""
    if f.cover is None:
        raise ValueError("forest has no node covers")
    F, K, LW = f.n_features, f.n_groups, f.leaf_width
    X = np.asarray(X, dtype=np.float64)
    left = sc.decisions(f, X)
    out = np.zeros((X.shape[0], K, F + 1, F + 1))
    for r in range(X.shape[0]):
        row = left[r].tolist()
        for t in range(f.n_trees):
            m = np.zeros((F, F, LW))
            phi = np.zeros((F, LW))
            _tree_shap_cond(f, t, row, phi, 0, -1)
            for j in _used(f, t):
                on = np.zeros((F, LW))
                off = np.zeros((F, LW))
                _tree_shap_cond(f, t, row, on, 1, j)
                _tree_shap_cond(f, t, row, off, -1, j)
                m[j] = (on - off) / 2
                m[j, j] = 0.0
                m[j, j] = phi[j] - m[j].sum(axis=0)
            if LW == 1:
                out[r, int(f.tree_group[t]), :F, :F] += m[:, :, 0]
            else:
                out[r, :, :F, :F] += np.moveaxis(m, 2, 0)
    return _finish(f, out)


def brute_force(f, x: np.ndarray) -> np.ndarray:
    """[K, F + 1, F + 1]: for one row, the Shapley interaction index
        sum over S of |S|! (M - |S| - 2)! / (2 (M - 1)!)
                      * [v(S + ij) - v(S + i) - v(S + j) + v(S)]
    of shap_cat_eval._expect off the diagonal, and the Shapley value minus the
    rest of the row on it, by enumerating feature subsets (exponential in F).
    A feature a tree never reads is a null player of that tree."""
    F, K, LW = f.n_features, f.n_groups, f.leaf_width
    left = sc.decisions(f, np.asarray(x, dtype=np.float64)[None, :])[0]
    out = np.zeros((K, F + 1, F + 1))
    for t in range(f.n_trees):
        used = _used(f, t)
        M = len(used)
        val = {S: sc._expect(f, t, left, set(S))
               for s in range(M + 1) for S in itertools.combinations(used, s)}

        def v(S):
            return val[tuple(sorted(S))]
        m = np.zeros((F, F, LW))
        for i in used:
            others = [u for u in used if u != i]
            phi = np.zeros(LW)
            for s in range(len(others) + 1):
                wgt = math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M)
                for S in itertools.combinations(others, s):
                    phi += wgt * (v(S + (i,)) - v(S))
            for j in others:
                rest = [u for u in others if u != j]
                acc = np.zeros(LW)
                for s in range(len(rest) + 1):
                    wgt = (math.factorial(s) * math.factorial(M - s - 2)
                           / (2 * math.factorial(M - 1)))
                    for S in itertools.combinations(rest, s):
                        acc += wgt * (v(S + (i, j)) - v(S + (i,)) - v(S + (j,)) + v(S))
                m[i, j] = acc
            m[i, i] = phi - m[i].sum(axis=0)
        if LW == 1:
            out[int(f.tree_group[t]), :F, :F] += m[:, :, 0]
        else:
            out[:, :F, :F] += np.moveaxis(m, 2, 0)
    return _finish(f, out[None])[0]


def scaled_error(got: np.ndarray, want: np.ndarray) -> float:
    """max |got - want| / max(max |want| of the row, 1), the scaled error of
    tests/test_gpu_shap.py, over [rows, ...] arrays."""
    rows = want.shape[0]
    w = want.reshape(rows, -1)
    g = np.asarray(got, dtype=np.float64).reshape(rows, -1)
    scale = np.maximum(np.abs(w).max(axis=1, keepdims=True), 1.0)
    return float((np.abs(g - w) / scale).max()) if w.size else 0.0
