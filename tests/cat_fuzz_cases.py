"""Seeded categorical forests and rows shared by tests/test_cat_oracle.py (CPU:
the references against each other, and what the cases cover) and
tests/test_gpu_cat_fuzz.py (the kernels against the references).

A case is a forest at the edges the categorical kernels branch on -- depth 1
to 8, fewer / exactly / more trees than one lane walks at once, group counts
around the kernels' widths, feature counts around the tile heights and the
widest LDS image, bitsets of 1 to 282 words -- with category sets at the
bitset edges (xgboost_format.edge_category_sets), categorical roots, and rows
that carry EDGE_VALUES in every categorical column.  Every parameter takes
each of its values equally often over the seeds (a shuffled deck), so no
value depends on luck.
"""
import json
import os
import tempfile

import numpy as np

from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import load_lightgbm_model
from kfserving_amd.formats import xgboost_format as xf
from oracle import lgb_ref, xgb_ref

XGB_SEEDS = range(32)
LGB_SEEDS = range(16)
DEPTHS = (1, 2, 3, 4, 5, 6, 7, 8)
TREES = (1, 2, 7, 8, 9, 17, 41, 72)          # per group
GROUPS = (1, 3, 4, 5, 16, 17)
FEATURES = (1, 3, 28, 64, 65, 128, 129, 200)
CATEGORIES = (1, 31, 32, 33, 64, 255, 1000, 9000)
MAX_TREES = 125                               # T * K of a case
ROW_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LGB_TREES = (1, 2, 7, 8, 9, 17, 41)
LGB_LEAVES = (2, 3, 8, 9)                     # depth <= 8: the categorical heap takes them
LGB_GROUPS = (1, 3)
LGB_FEATURES = (1, 3, 28, 65, 128)
LGB_CATEGORIES = (1, 32, 33, 255, 1000)
LGB_MISSING = ((lf.MISSING_NONE,), (lf.MISSING_ZERO,), (lf.MISSING_NAN,),
               (lf.MISSING_NONE, lf.MISSING_ZERO, lf.MISSING_NAN))
# total members of the random sets of a forest: keeps the JSON document small
MEMBER_BUDGET = 200000


def edge_values(nw):
    """The values of the issue for bitsets of at most ``nw`` words: the last
    member, the first value past the words, the tops of words 0 and 1, the
    invalid and the saturating values, and NaN."""
    return [32.0 * nw - 1, 32.0 * nw, 32.0 * nw + 0.5, 31.0, 31.999, 32.0, 63.0, 64.0, -0.0, -1e-40,
            -0.5, -1.0, np.inf, -np.inf, 16777215.0, 16777216.0, 2147483648.0, 4294967296.0, 1e30,
            np.nan]


LGB_EXTRA = [-0.999, -0.25]                   # (-1, 0): category 0 under LightGBM's rule


def _deck(values, n, key):
    """``n`` entries holding each of ``values`` equally often, in a fixed
    shuffled order of their own."""
    reps = -(-n // len(values))
    deck = np.array(list(values) * reps)[:n]
    return np.random.default_rng([key, 64]).permutation(deck)


def _tree_deck(groups, key):
    """Trees per group for each seed's group count: each of TREES equally
    often, the largest first onto a random seed whose T * K stays within
    MAX_TREES (72 trees a group go with K = 1 only, 41 with K <= 3, ...)."""
    rng = np.random.default_rng([key, 64])
    out = [0] * len(groups)
    for tg in sorted(_deck(TREES, len(groups), key), reverse=True):
        free = [i for i, k in enumerate(groups) if out[i] == 0 and tg * k <= MAX_TREES]
        out[free[int(rng.integers(0, len(free)))]] = int(tg)
    return np.array(out)


_XGB_DECKS = [_deck(v, len(XGB_SEEDS), k) for k, v in
              enumerate((DEPTHS, GROUPS, FEATURES, CATEGORIES))]
_XGB_DECKS.insert(1, _tree_deck(_XGB_DECKS[1], 9))
_LGB_DECKS = [_deck(v, len(LGB_SEEDS), 10 + k) for k, v in
              enumerate((LGB_TREES, LGB_LEAVES, LGB_GROUPS, LGB_FEATURES, LGB_CATEGORIES))]


def clean_rows(n):
    """Rows that hold no NaN: 64-row spans 1, 4..7 and the odd ones from 9 on,
    so tiles of 64, 128 and 256 rows exist both wholly NaN-free and not."""
    span = np.arange(n) // 64
    return (span == 1) | ((span >= 4) & (span < 8)) | ((span >= 8) & (span % 2 == 1))


def make_rows(rng, n, F, cat_features, nw, extra=()):
    """[n, F] float32: the value mix of tests/test_gpu_xgb_categorical.py
    (N(0, 1) with 2 % NaN; categorical columns integers plus a fraction up to
    past the longest bitset, 5 % NaN, 1 % each of 3e9, 2^24 and -0.5), then
    edge_values(nw) + extra at random rows of every categorical column, then
    the NaN of clean_rows replaced."""
    X = rng.standard_normal((n, F))
    X[rng.random(X.shape) < 0.02] = np.nan
    vals = np.array(edge_values(nw) + list(extra))
    for j in cat_features:
        X[:, j] = rng.integers(-5, 32 * nw + 16, size=n) + rng.choice([0, 0.5, 0.999], size=n)
        X[rng.random(n) < 0.05, j] = np.nan
        X[rng.random(n) < 0.01, j] = 3e9
        X[rng.random(n) < 0.01, j] = 16777216.0
        X[rng.random(n) < 0.01, j] = -0.5
        pos = rng.permutation(n)[:vals.shape[0]]
        X[pos, j] = rng.permutation(vals)[:pos.shape[0]]
    clean = clean_rows(n)
    fill = np.isnan(X) & clean[:, None]
    X[fill] = rng.integers(0, 32 * nw + 16, size=int(fill.sum()))
    for s in range(0, n if n >= 64 else 0, 64):   # every other span holds a NaN for certain
        if not clean[s] and not np.isnan(X[s:s + 64]).any():
            X[s + int(rng.integers(0, min(64, n - s))), cat_features[-1]] = np.nan
    return X.astype(np.float32)


def _all_rows(rng, F, cat_features, nw, extra=()):
    counts = ROW_COUNTS + (int(rng.integers(600, 2101)),)
    return [make_rows(rng, n, F, cat_features, nw, extra) for n in counts]


class XGBCase:
    """One XGBoost fuzz case: the raw trees, the JSON document, the loaded
    forest, the vectorised reference and the row blocks."""

    def __init__(self, seed):
        rng = np.random.default_rng([seed, 64])
        depth, tg, K, F, ncat = (int(d[seed]) for d in _XGB_DECKS)
        T = tg * K
        self.seed, self.depth, self.T, self.K, self.F, self.ncat = seed, depth, T, K, F, ncat
        self.desc = dict(seed=seed, depth=depth, T=T, K=K, F=F, ncat=ncat)
        self.objective = "binary:logistic" if K == 1 else "multi:softprob"
        num_class = 0 if K == 1 else K
        self.cat_features = sorted(int(j) for j in rng.choice(F, size=min(F, 3), replace=False))
        trees, ti = xf.synthetic_complete_trees(T, depth, F, seed=1000 + seed, num_class=num_class)
        # as many categorical nodes as the member budget allows, half at the most
        feat = np.concatenate([(t["sindex"][t["cleft"] != -1] & 0x7FFFFFFF) for t in trees])
        candidates = max(1, int(np.isin(feat, self.cat_features).sum()))
        frac = min(0.5, max(8.0, MEMBER_BUDGET / (0.4 * ncat + 1)) / candidates)
        xf.add_categorical_splits(trees, self.cat_features, ncat, seed=2000 + seed, frac=frac,
                                  edge_frac=0.25, root_trees=5)
        self.trees, self.tree_info = trees, ti
        self.sets = [c for t in trees for c in t.get("cats", {}).values()]
        self.nw = max(int(np.max(c)) // 32 + 1 for c in self.sets)
        self.doc = xf.json_model_doc(trees, ti, F, num_class, 0.5, self.objective, version=(2, 0, 0))
        self.forest = xf.parse_xgboost_bytes(json.dumps(self.doc).encode())
        self.ref = xgb_ref.from_raw_trees(trees, ti, F, num_class, 0.5, self.objective,
                                          major_version=2)
        self.rows = _all_rows(rng, F, self.cat_features, self.nw)
        self._want = None

    def want(self):
        """[(X, leaves, margins [n, K], predictions, trace)] of the reference,
        one entry a row block, computed once."""
        if self._want is None:
            self._want = []
            for X in self.rows:
                trace = []
                leaf = xgb_ref.leaf_index(self.ref, X, trace=trace)
                margin = np.asarray(xgb_ref.predict(self.ref, X, output_margin=True))
                margin = margin.reshape(X.shape[0], self.K)
                pred = np.asarray(xgb_ref.transform(self.objective, margin))
                self._want.append((X, leaf, margin, pred, trace))
        return self._want


class LGBCase:
    """One LightGBM fuzz case: leaf-wise trees of depth <= 8 with categorical
    splits, one missing type or all three."""

    def __init__(self, seed):
        rng = np.random.default_rng([seed, 65])
        tg, leaves, K, F, ncat = (int(d[seed]) for d in _LGB_DECKS)
        T = tg * K
        self.mts = LGB_MISSING[seed % 4]
        self.seed, self.T, self.K, self.F, self.ncat = seed, T, K, F, ncat
        self.desc = dict(seed=seed, T=T, leaves=leaves, K=K, F=F, ncat=ncat, mts=self.mts)
        self.cat_features = sorted(int(j) for j in rng.choice(F, size=min(F, 3), replace=False))
        trees = lf.synthetic_leafwise_trees(T, leaves, F, seed=3000 + seed, missing_types=self.mts)
        lf.add_categorical_splits(trees, self.cat_features, ncat, seed=4000 + seed, edge_frac=0.25,
                                  root_trees=5)
        self.trees = trees
        self.nw = max(int(np.diff(t["cat_boundaries"]).max()) for t in trees
                      if "cat_boundaries" in t)
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "model.txt")
            lf.write_lightgbm_text(p, trees, F, "binary sigmoid:1" if K == 1 else
                                   f"multiclass num_class:{K}", num_class=K)
            self.forest = load_lightgbm_model(p)
            self.ref = lgb_ref.read_lgb_text(p)
        self.rows = _all_rows(rng, F, self.cat_features, self.nw, LGB_EXTRA)
        self._want = None

    def want(self):
        """[(X, leaves, raw scores, predictions, trace)] of oracle/lgb_ref, one
        entry a row block (the reference reads the rows widened to float64)."""
        if self._want is None:
            self._want = []
            for X in self.rows:
                Xd = X.astype(np.float64)
                trace = []
                leaf = lgb_ref.leaf_index(self.ref, Xd, trace=trace)
                self._want.append((X, leaf, lgb_ref.predict(self.ref, Xd, raw_score=True),
                                   lgb_ref.predict(self.ref, Xd), trace))
        return self._want


_CASES = {}


def xgb_case(seed) -> XGBCase:
    if ("xgb", seed) not in _CASES:
        _CASES["xgb", seed] = XGBCase(seed)
    return _CASES["xgb", seed]


def lgb_case(seed) -> LGBCase:
    if ("lgb", seed) not in _CASES:
        _CASES["lgb", seed] = LGBCase(seed)
    return _CASES["lgb", seed]


def decided(trace):
    """(values, went_left) over every visit to a categorical node."""
    if not trace:
        return np.zeros(0, dtype=np.float64), np.zeros(0, dtype=bool)
    return (np.concatenate([np.asarray(v, dtype=np.float64) for _, _, _, v, _ in trace]),
            np.concatenate([g for _, _, _, _, g in trace]))


def holds(values, v):
    """Whether the float32 image of ``v`` is among ``values`` (NaN matches NaN,
    -0.0 only -0.0)."""
    v = np.float64(np.float32(v))
    if np.isnan(v):
        return bool(np.isnan(values).any())
    return bool(((values == v) & (np.signbit(values) == np.signbit(v))).any())
