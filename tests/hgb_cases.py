"""Fitted sklearn HistGradientBoosting models and rows for the HGB tests
(tests/test_hgb_format.py on the CPU, tests/test_gpu_hgb.py on the device) --
test helper only.  Models are fitted here with fixed seeds (about a second
for all of them), once a process, and never changed; sklearn itself is the
reference, plus :func:`sk_leaf_index`, a walk of the estimator's own node
arrays by sklearn's rule that shares nothing with the loader's encoding."""
import functools

import numpy as np

F = 6
CAT_COLS = (1, 4)                 # not leading: the estimator's column permutation shows
CATS = {1: np.array([0, 1, 2, 3, 5, 7, 11, 40, 41, 63, 64, 200, 300, 1000], dtype=np.float64),
        4: np.arange(9, dtype=np.float64)}
N_TRAIN = 2000
MAX_ITER = 10

# name -> (estimator kind, loss or None, categorical, extra constructor arguments)
MODELS = {
    "reg-num": ("reg", "squared_error", False, {}),
    "reg-cat": ("reg", "squared_error", True, {}),
    "poisson-num": ("reg", "poisson", False, {}),
    "poisson-cat": ("reg", "poisson", True, {}),
    "binary-num": ("clf2", None, False, {}),
    "binary-cat": ("clf2", None, True, {}),
    "multi-num": ("clf3", None, False, {}),
    "multi-cat": ("clf3", None, True, {}),
    # depth-limited: complete-able to depth 6, so the heap layouts take it
    "reg-cat-d6": ("reg", "squared_error", True, {"max_depth": 6}),
    "reg-num-d6": ("reg", "squared_error", False, {"max_depth": 6}),
}
NUMERICAL = [n for n, m in MODELS.items() if not m[2]]
CATEGORICAL = [n for n, m in MODELS.items() if m[2]]


def _training():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((N_TRAIN, F))
    for c in CAT_COLS:
        X[:, c] = rng.choice(CATS[c], size=N_TRAIN)
    X[rng.random((N_TRAIN, F)) < 0.1] = np.nan      # both values of missing_go_to_left occur
    z = np.nan_to_num(X)
    y = (z[:, 1] % 3 == 0) * 2.0 + z[:, 2] + (z[:, 4] > 4) - 0.5 * z[:, 0] * z[:, 3] \
        + 0.1 * rng.standard_normal(N_TRAIN)
    return X, y


@functools.lru_cache(maxsize=None)
def fitted(name):
    """The fitted estimator of MODELS[name]."""
    from sklearn.ensemble import HistGradientBoostingClassifier, HistGradientBoostingRegressor
    kind, loss, categorical, extra = MODELS[name]
    X, y = _training()
    kw = dict(max_iter=MAX_ITER, random_state=0, **extra)
    if categorical:
        kw["categorical_features"] = list(CAT_COLS)
    if kind == "reg":
        if loss == "poisson":
            y = np.random.default_rng(1).poisson(np.exp(0.4 * y))
        return HistGradientBoostingRegressor(loss=loss, **kw).fit(X, y)
    if kind == "clf2":
        return HistGradientBoostingClassifier(**kw).fit(X, np.where(y > np.median(y), "yes", "no"))
    labels = (y > np.quantile(y, 0.35)).astype(int) + (y > np.quantile(y, 0.7))
    return HistGradientBoostingClassifier(**kw).fit(X, labels * 10 + 3)     # classes 3, 13, 23


@functools.lru_cache(maxsize=None)
def forest(name):
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn
    return forest_from_sklearn(fitted(name))


def served(name):
    """A SKLearnModel holding the forest, for its request checks (no device
    is touched until a predict)."""
    from kfserving_amd.sklearnserver import SKLearnModel
    model = SKLearnModel(name, "")
    model._set_forest(forest(name))
    model.ready = True
    return model


@functools.lru_cache(maxsize=None)
def rows(n=1000, seed=5, non_integer=False):
    """[n, F] float64 rows, read-only.  Numerical columns: N(0,1) with NaN and
    +-inf.  Columns CAT_COLS (categorical to half of the models, numbers to
    the rest): known categories, unknown integers, negatives, -0.0, 2^24,
    1e300 and NaN -- and with ``non_integer`` halves added to half of them,
    which sklearn reads as unknown categories."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F))
    X[:, 1] = rng.integers(-3, 1100, size=n)
    X[: n // 2, 1] = rng.choice(CATS[1], size=n // 2)
    X[:, 4] = rng.integers(-2, 12, size=n)
    if non_integer:
        for c in CAT_COLS:
            X[:, c] += rng.choice([0.0, 0.5, 0.25], size=n)
    X[rng.random(X.shape) < 0.1] = np.nan
    special = rng.permutation(n)
    for i, (c, v) in enumerate([(1, -0.0), (1, 2.0 ** 24), (1, 1e300), (4, -0.0), (4, 2.0 ** 24),
                                (4, 1e300), (1, -7.0), (4, -1.0), (1, np.nan), (4, np.nan),
                                (2, np.inf), (2, -np.inf), (0, np.inf), (5, -np.inf),
                                (3, np.nan), (0, 1e300), (5, -1e300)]):
        X[special[i % n], c] = v
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference(name, n=1000, seed=5, non_integer=False):
    """sklearn's own (raw margins [n, K], predict, leaf index [n, T]) on rows()."""
    est = fitted(name)
    X = rows(n, seed, non_integer)
    out = (np.ascontiguousarray(est._raw_predict(X)), est.predict(X), sk_leaf_index(est, X))
    for a in out:
        a.setflags(write=False)
    return out


def _bit(words, code):
    """Bit ``code`` (float, NaN-free, in [0, 256)) of each row's 8-word bitset."""
    c = code.astype(np.int64)
    return ((words[np.arange(c.size), c // 32] >> (c % 32).astype(np.uint32)) & 1) != 0


def sk_leaf_index(est, X):
    """[rows, trees] node index of the leaf each row reaches, by sklearn's own
    rule (_predictor.pyx, _predict_one_from_raw_data) on the estimator's own
    preprocessed matrix and code-space bitsets; trees iteration-major."""
    Xt = np.asarray(est._preprocess_X(np.asarray(X, dtype=np.float64), reset=False))
    known, f_idx_map = (est._bin_mapper.make_known_categories_bitsets()
                        if est._preprocessor is not None else (None, None))
    cols = []
    for it in est._predictors:
        for p in it:
            nd = p.nodes
            node = np.zeros(Xt.shape[0], dtype=np.int64)
            while True:
                act = np.flatnonzero(nd["is_leaf"][node] == 0)
                if act.size == 0:
                    break
                g = nd[node[act]]
                x = Xt[act, g["feature_idx"]]
                nan = np.isnan(x)
                left = x <= g["num_threshold"]
                cat = g["is_categorical"] != 0
                if cat.any():
                    code = np.where(nan | ~cat, 0.0, x)
                    in_left = _bit(p.raw_left_cat_bitsets[np.where(cat, g["bitset_idx"], 0)], code)
                    in_known = _bit(known[f_idx_map[np.where(cat, g["feature_idx"], 0)]], code)
                    mgl = g["missing_go_to_left"] != 0
                    left = np.where(cat, in_left | (~in_known & mgl), left)
                left = np.where(nan, g["missing_go_to_left"] != 0, left)
                node[act] = np.where(left, g["left"], g["right"])
            cols.append(node)
    return np.stack(cols, axis=1)


def categorical_orientations(est):
    """(missing_go_to_left = 1, = 0) counts over the categorical split nodes."""
    one = zero = 0
    for it in est._predictors:
        for p in it:
            nd = p.nodes
            cat = (nd["is_leaf"] == 0) & (nd["is_categorical"] != 0)
            one += int((cat & (nd["missing_go_to_left"] != 0)).sum())
            zero += int((cat & (nd["missing_go_to_left"] == 0)).sum())
    return one, zero
