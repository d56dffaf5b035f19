"""CPU reference for TreeSHAP contributions of forests with LightGBM
categorical splits, for the tests only.

``oracle/shap_ref.contributions`` refuses categorical nodes; this helper is
the same float64 recursion on the canonical ``Forest`` (Lundberg, Erion & Lee
2018, Algorithm 2: ExtendPath at every node, UnwindPath where a feature comes
back, UnwoundPathSum at the leaves, in xgboost's expression order) with one
difference: the hot child of a node comes from :func:`decisions`, which takes
``tests/canon_eval.cat_left`` at categorical nodes (LightGBM
``Tree::Decision`` does the same inside ``Tree::TreeSHAP``).

It walks the tree.  It never forms the merged per-feature path elements (an
interval, a category set) the device builder makes, so the two can only agree
by both being right.  :func:`brute_force` gives the Shapley values of the same
path-dependent value function by subset enumeration, for forests of a few
features; tests/test_shap_cat_eval.py pins the recursion to it.

float32 rows are read as the same doubles and compared with the float64
thresholds, as the device's contributions kernels do.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

from kfserving_amd.forest import NODE_CATEGORICAL, NODE_NAN_LEFT, NODE_ZERO_FLIP
from tests import canon_eval


def decisions(f, X: np.ndarray) -> np.ndarray:
    """[rows, N] bool: whether the row turns left at node n (False at leaves),
    by the canonical split rule of include/treeinfer.h."""
    X = np.asarray(X, dtype=np.float64)
    rows = X.shape[0]
    out = np.zeros((rows, f.n_nodes), dtype=bool)
    g = np.nonzero(f.feature >= 0)[0]
    if g.size == 0:
        return out
    fe = f.feature[g]
    x = np.where(fe[None, :] < X.shape[1], X[:, np.minimum(fe, X.shape[1] - 1)], np.nan)
    if f.lgb_zero_map:
        x = np.where(np.abs(x) <= float(np.float32(1e-35)), 0.0, x)
    t = f.threshold[g][None, :]
    with np.errstate(invalid="ignore"):
        left = x <= t
        zero_left = ~(0 <= t)
    left = np.where(np.isnan(x), ((f.flags[g] & NODE_NAN_LEFT) != 0)[None, :], left)
    flip = (x == 0) & ((f.flags[g] & NODE_ZERO_FLIP) != 0)[None, :]
    left = np.where(flip, zero_left, left)
    cat = (f.flags[g] & NODE_CATEGORICAL) != 0
    if cat.any():
        gc = g[cat]
        left[:, cat] = canon_eval.cat_left(f, np.broadcast_to(gc[None, :], (rows, gc.size)),
                                           x[:, cat])
    out[:, g] = left
    return out


def _tree_shap(f, t: int, left: np.ndarray, phi: np.ndarray) -> None:
    """Add tree t's contributions of one row (``left``: its decision at every
    node of the forest) into phi [F, leaf_width]."""
    b = int(f.tree_offset[t])
    feature, lc, rc, cover, leaf_value = f.feature, f.left, f.right, f.cover, f.leaf_value

    # a path is three parallel lists over its elements: feature, zero
    # fraction, one fraction, and the permutation weights pw
    def rec(v, fi, zf, of, pw, pz, po, pf):
        # ExtendPath with (pz, po, pf)
        d = len(fi)
        fi = fi + [pf]
        zf = zf + [pz]
        of = of + [po]
        pw = pw + [1.0 if d == 0 else 0.0]
        for i in range(d - 1, -1, -1):
            pw[i + 1] += po * pw[i] * (i + 1) / (d + 1)
            pw[i] = pz * pw[i] * (d - i) / (d + 1)
        g = b + v
        if feature[g] < 0:
            lv = leaf_value[g]
            for k in range(1, d + 1):
                # UnwoundPathSum of element k
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
                phi[fi[k]] += total * (o - z) * lv
            return
        fe = int(feature[g])
        l, r = int(lc[g]), int(rc[g])
        hot, cold = (l, r) if left[g] else (r, l)
        w = cover[g]
        hz, cz = cover[b + hot] / w, cover[b + cold] / w
        iz, io = 1.0, 1.0
        if fe in fi:
            # UnwindPath: the feature's earlier element leaves the path
            k = fi.index(fe)
            iz, io = zf[k], of[k]
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
        rec(hot, fi, zf, of, pw, hz * iz, io, fe)
        rec(cold, fi, zf, of, pw, cz * iz, 0.0, fe)

    rec(0, [], [], [], [], 1.0, 1.0, -1)


def _bias(f) -> np.ndarray:
    """base margin + cover-weighted mean leaf value of every tree, per group
    (before the average divisor)."""
    bias = np.asarray(f.base_margin, dtype=np.float64).copy() * f.average_divisor
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])

        def mean(v):
            g = b + v
            if f.feature[g] < 0:
                return np.asarray(f.leaf_value[g], dtype=np.float64)
            l, r = int(f.left[g]), int(f.right[g])
            return (mean(l) * f.cover[b + l] + mean(r) * f.cover[b + r]) / f.cover[g]
        m = mean(0)
        if f.leaf_width == 1:
            bias[int(f.tree_group[t])] += m[0]
        else:
            bias += m
    return bias


def contributions(f, X: np.ndarray) -> np.ndarray:
    """[rows, K * (F + 1)] float64: per group the F feature contributions, then
    the bias, as TI_OUTPUT_CONTRIB lays them out."""
    if f.cover is None:
        raise ValueError("forest has no node covers")
    F, K, LW = f.n_features, f.n_groups, f.leaf_width
    X = np.asarray(X, dtype=np.float64)
    left = decisions(f, X)
    out = np.zeros((X.shape[0], K, F + 1))
    for r in range(X.shape[0]):
        row = left[r].tolist()
        for t in range(f.n_trees):
            phi = np.zeros((F, LW))
            _tree_shap(f, t, row, phi)
            if LW == 1:
                out[r, int(f.tree_group[t]), :F] += phi[:, 0]
            else:
                out[r, :, :F] += phi.T
    out[:, :, F] = _bias(f)
    return (out / f.average_divisor).reshape(X.shape[0], K * (F + 1))


def _expect(f, t: int, left, known) -> np.ndarray:
    """E[tree t | the features in `known` take the row's values]: follow the
    row at their splits, average the children by cover at the others."""
    b = int(f.tree_offset[t])

    def ev(v):
        g = b + v
        if f.feature[g] < 0:
            return np.asarray(f.leaf_value[g], dtype=np.float64)
        l, r = int(f.left[g]), int(f.right[g])
        if int(f.feature[g]) in known:
            return ev(l) if left[g] else ev(r)
        return (ev(l) * f.cover[b + l] + ev(r) * f.cover[b + r]) / f.cover[g]
    return ev(0)


def brute_force(f, x: np.ndarray) -> np.ndarray:
    """[K * (F + 1)] exact Shapley values of :func:`_expect` for one row by
    enumerating feature subsets (exponential in F)."""
    F, K, LW = f.n_features, f.n_groups, f.leaf_width
    left = decisions(f, np.asarray(x, dtype=np.float64)[None, :])[0]
    out = np.zeros((K, F + 1))
    for t in range(f.n_trees):
        used = sorted({int(v) for v in f.feature[f.tree_slice(t)] if v >= 0})
        val = {S: _expect(f, t, left, set(S))
               for s in range(len(used) + 1) for S in itertools.combinations(used, s)}
        groups = [int(f.tree_group[t])] if LW == 1 else list(range(K))
        n = len(used)
        for i in used:        # a feature the tree never reads is a null player
            acc = np.zeros(LW)
            others = [j for j in used if j != i]
            for s in range(len(others) + 1):
                wgt = math.factorial(s) * math.factorial(n - s - 1) / math.factorial(n)
                for S in itertools.combinations(others, s):
                    acc += wgt * (val[tuple(sorted(S + (i,)))] - val[S])
            out[groups, i] += acc if LW > 1 else acc[0]
        out[groups, F] += val[()] if LW > 1 else val[()][0]
    out[:, F] += np.asarray(f.base_margin) * f.average_divisor
    return (out / f.average_divisor).reshape(K * (F + 1))


# ------------------------------------------------------- forests and rows
def lgb_cat_forest(n_trees, num_leaves, n_features, seed, cat_features=(), n_categories=0,
                   K=1, **cat_kw):
    """A seeded leaf-wise LightGBM forest (with counts), a fraction of whose
    splits on ``cat_features`` is categorical, through the text loader."""
    from kfserving_amd.formats import lightgbm_format as lf
    trees = lf.synthetic_leafwise_trees(n_trees, num_leaves, n_features, seed=seed)
    if len(cat_features):
        lf.add_categorical_splits(trees, list(cat_features), n_categories, seed + 1000, **cat_kw)
    return forest_of_trees(trees, n_features, K)


def forest_of_trees(trees, n_features, K=1, feature_names=None, objective=None):
    """LightGBM tree dicts (lightgbm_format.write_lightgbm_text) as a Forest."""
    import os
    import tempfile
    from kfserving_amd.formats import lightgbm_format as lf
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.txt")
        obj = objective or (f"multiclass num_class:{K}" if K > 1 else "binary sigmoid:1")
        lf.write_lightgbm_text(p, trees, n_features, obj, num_class=K,
                               feature_names=feature_names)
        return lf.load_lightgbm_model(p)


def cat_columns(f):
    """The features some categorical node splits on."""
    cat = (f.feature >= 0) & ((f.flags & NODE_CATEGORICAL) != 0)
    return sorted({int(v) for v in f.feature[cat]})


def rows(f, n, seed, n_categories):
    """float64 rows whose every value but one is a float32: N(0,1) with 8 % NaN
    and 8 % exact zeros; the categorical columns hold integers in
    [-5, n_categories + 20) plus a fraction in {0, 0.5, 0.999}, 5 % NaN and
    1 % 3e9, and their first rows the edges of LightGBM's rule: -1.0, -0.5,
    -0.0, 31, 32, the last code inside and the first past the longest and the
    shortest bitset, and 2147483647 (which float32 rounds to 2^31)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f.n_features))
    X[rng.random(X.shape) < 0.08] = np.nan
    X[rng.random(X.shape) < 0.08] = 0.0
    cols = cat_columns(f)
    cat = (f.feature >= 0) & ((f.flags & NODE_CATEGORICAL) != 0)
    nws = sorted({int(f.cat_nwords[cat].max()), int(f.cat_nwords[cat].min())}) if cols else []
    edges = [-1.0, -0.5, -0.0, 31.0, 32.0, 2147483647.0]
    for nw in nws:
        edges += [32.0 * nw - 1, 32.0 * nw]
    for j, c in enumerate(cols):
        v = rng.integers(-5, n_categories + 20, size=n).astype(np.float64)
        v += rng.choice([0.0, 0.5, 0.999], size=n)
        v[rng.random(n) < 0.05] = np.nan
        v[rng.random(n) < 0.01] = 3e9
        X[:, c] = v
    X = X.astype(np.float32).astype(np.float64)
    for j, c in enumerate(cols):
        for i, e in enumerate(edges):
            X[(i + 3 * j) % n, c] = e
    return X


def path_element_kinds(f):
    """From the forest's arrays: over all root-to-leaf paths, how many
    (path, feature) pairs have a numerical and a categorical split
    ("num+cat"), at least two categorical splits all turning left ("cat-LL"),
    all turning right ("cat-RR"), or turning both ways ("cat-LR"); and the
    longest path in unique features ("max_unique")."""
    kinds = {"num+cat": 0, "cat-LL": 0, "cat-RR": 0, "cat-LR": 0, "paths": 0, "max_unique": 0}
    for t in range(f.n_trees):
        b = int(f.tree_offset[t])
        stack = [(0, ())]
        while stack:
            v, path = stack.pop()
            g = b + v
            if f.feature[g] < 0:
                kinds["paths"] += 1
                by_feature = {}
                for fe, is_cat, turn in path:
                    by_feature.setdefault(fe, []).append((is_cat, turn))
                kinds["max_unique"] = max(kinds["max_unique"], len(by_feature))
                for splits in by_feature.values():
                    turns = [turn for is_cat, turn in splits if is_cat]
                    if turns and len(turns) < len(splits):
                        kinds["num+cat"] += 1
                    if len(turns) >= 2:
                        key = "cat-LL" if all(turns) else "cat-LR" if any(turns) else "cat-RR"
                        kinds[key] += 1
                continue
            step = (int(f.feature[g]), bool(f.flags[g] & NODE_CATEGORICAL))
            stack.append((int(f.left[g]), path + (step + (True,),)))
            stack.append((int(f.right[g]), path + (step + (False,),)))
    return kinds
