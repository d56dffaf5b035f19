"""Small batches on the tree-parallel walk (TI_OPT_SMALL_BATCH_ROWS,
treeinfer_small.h).  Margins bit for bit to the family's oracle; every kind bit
for bit to the same DeviceForest with the option at 0; leaf ids to the numpy
walk of the Forest arrays (tests/canon_eval.py).  DeviceForest.predict casts
float64 rows of an XGBoost or sklearn forest to float32, as the plugins do:
float64 rows of those reach the walk through predict_device."""
import os
import tempfile

import numpy as np
import pytest

from kfserving_amd.engine import OPT_SMALL_BATCH_ROWS, DeviceForest, TreeInferError
from kfserving_amd.forest import OUT_LEAF, OUT_MARGIN, OUT_PREDICT, T_ARGMAX, T_IDENTITY
from kfserving_amd.formats import lightgbm_format as lf, load_lightgbm_model, xgboost_format as xf
from oracle import lgb_ref, sk_ref, xgb_ref
from tests import canon_eval, sk_pipeline_cases

pytestmark = pytest.mark.gpu

TH = 70                          # the option's value
ROWS = (1, 2, 65, TH, TH + 1)    # TH + 1 takes the forest's own walk


def _xgb(n_trees, depth, F, seed, cats=()):
    trees, ti = xf.synthetic_complete_trees(n_trees, depth, F, seed=seed)
    if cats:
        xf.add_categorical_splits(trees, list(cats), 70, seed + 1, root_trees=3)
    ref = xgb_ref.from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic")
    return (xf.forest_from_raw_trees(trees, ti, F, 0, 0.0, "binary:logistic"), cats,
            lambda X, margin: xgb_ref.predict(ref, X.astype(np.float32), output_margin=margin))


def _lgb(n_trees, leaves, F, seed, cats, linear=False):
    trees = lf.synthetic_leafwise_trees(n_trees, leaves, F, seed=seed)   # every missing type
    if cats:
        lf.add_categorical_splits(trees, list(cats), 300, seed + 1)
    if linear:
        lf.add_linear_leaves(trees, F, seed + 2)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "model.txt")
        lf.write_lightgbm_text(p, trees, F, "multiclass num_class:3", num_class=3)
        f, m = load_lightgbm_model(p), lgb_ref.read_lgb_text(p)
    return f, cats, lambda X, margin: lgb_ref.predict(m, X.astype(np.float64), raw_score=margin)


def _sk():
    from sklearn.ensemble import RandomForestClassifier
    from kfserving_amd.formats.sklearn_format import forest_from_sklearn, tree_arrays_from_sklearn
    rng = np.random.default_rng(3)
    X = rng.standard_normal((3000, 10)).astype(np.float32)
    y = (X[:, 0] + X[:, 3] * X[:, 7] > 0).astype(int) + (X[:, 5] > 0.5)
    est = RandomForestClassifier(n_estimators=10, max_depth=12, random_state=0).fit(X, y)
    trees = [tree_arrays_from_sklearn(e.tree_) for e in est.estimators_]
    for t in trees:   # sk_ref reads probabilities, as the stored models hold them
        t["value"] = t["value"] / t["value"].sum(axis=2, keepdims=True)

    def ref(X, margin):
        p = sk_ref.predict_proba(trees, X.astype(np.float32), 3)
        return p if margin else np.argmax(p, axis=1).astype(np.float64)
    return forest_from_sklearn(est), (), ref


CASES = {
    "xgb-d8-65": lambda: _xgb(65, 8, 28, 5),          # float32 sums, default layout 3
    "xgb-d3-63": lambda: _xgb(63, 3, 9, 6),
    "xgb-one-leaf": lambda: _xgb(1, 0, 4, 7),
    "xgb-1025-stumps": lambda: _xgb(1025, 1, 6, 8),   # two passes of 1,024 lanes, the last of one tree
    "xgb-cat": lambda: _xgb(30, 5, 8, 9, cats=(0, 3)),
    "lgb-cat-k3": lambda: _lgb(63, 31, 12, 21, (0, 3, 7)),   # float64, zero-missing nodes, K = 3
    "sk-d12-vector": _sk,                              # vector leaves, a record layout
    "xgb-wide": lambda: _xgb(2, 3, 16400, 10),        # float32 rows of 65,600 B: read from global memory
}
_BUILT = {}


def case(name):
    if name not in _BUILT:
        f, cats, ref = CASES[name]()
        _BUILT[name] = (f, cats, ref, DeviceForest(f, [0]))
    return _BUILT[name]


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    while _BUILT:
        _BUILT.popitem()[1][3].close()


def rows(f, cats, n, seed):
    """float32 rows with NaN, +-0, +-inf, tiny values and values equal to thresholds."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, f.n_features)).astype(np.float32)
    for j in cats:
        X[:, j] = rng.integers(-2, 320, size=n) + rng.choice([0, 0.5], size=n)
    sp = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-36, -1e-36], dtype=np.float32)
    m = rng.random(X.shape) < 0.15
    X[m] = sp[rng.integers(0, len(sp), m.sum())]
    internal = np.nonzero(f.left >= 0)[0]
    if len(internal):
        g = rng.choice(internal, size=(n, 3))
        X[np.arange(n)[:, None], f.feature[g]] = f.threshold[g].astype(np.float32)
    return X


def check(name, X, n_cols=None):
    """Every kind on X[:, :n_cols], the option on and off, against the references."""
    f, _, ref, dev = case(name)
    Xin = np.ascontiguousarray(X[:, :n_cols])
    Xref = X.copy()
    Xref[:, Xin.shape[1]:] = np.nan
    dev.set_option(OPT_SMALL_BATCH_ROWS, TH)
    got = {k: dev.predict(Xin, k) for k in (OUT_MARGIN, OUT_PREDICT, OUT_LEAF)}
    dev.set_option(OPT_SMALL_BATCH_ROWS, 0)
    for k, g in got.items():
        assert np.array_equal(g, dev.predict(Xin, k), equal_nan=True), f"kind {k} against the option at 0"
    assert np.array_equal(got[OUT_MARGIN], ref(Xref, True).reshape(got[OUT_MARGIN].shape))
    want = ref(Xref, False).reshape(got[OUT_PREDICT].shape)
    if f.transform in (T_IDENTITY, T_ARGMAX):
        assert np.array_equal(got[OUT_PREDICT], want)
    else:
        # the oracle's exp is the host's libm: 1e-5 as tests/test_gpu_parity.py; bits held above
        np.testing.assert_allclose(got[OUT_PREDICT], want, rtol=1e-5)
    assert np.array_equal(got[OUT_LEAF], canon_eval.predict(f, Xref, OUT_LEAF))
    if len(X) <= TH:
        assert dev.info()["small_walk"] == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(CASES))
def test_answers(name, n, dtype):
    f, cats, _, _ = case(name)
    check(name, rows(f, cats, n, seed=n).astype(dtype))


@pytest.mark.parametrize("name", ["xgb-d8-65", "lgb-cat-k3", "xgb-wide"])
def test_fewer_columns_read_nan(name):
    f, cats, _, _ = case(name)
    check(name, rows(f, cats, 5, seed=40), n_cols=f.n_features - 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,short", [("xgb-d8-65", 0), ("xgb-wide", 3)])
def test_device_rows_of_either_type_and_a_wider_stride(name, short, dtype):
    """The rows' own type (float64 against thr64), 5 columns of padding a row, `short`
    columns fewer than the forest reads (xgb-wide: the NaN decided in the walk)."""
    torch = pytest.importorskip("torch")
    f, cats, ref, dev = case(name)
    F, cols, n = f.n_features, f.n_features - short, 9
    X = rows(f, cats, n, seed=41)
    X[:, cols:] = np.nan
    xt = torch.from_numpy(np.concatenate([X[:, :cols], np.full((n, F + 5 - cols), 7.0, np.float32)],
                                         axis=1).astype(dtype)).cuda()
    for kind, want in ((OUT_MARGIN, ref(X, True)), (OUT_LEAF, canon_eval.predict(f, X.astype(dtype), OUT_LEAF))):
        out = torch.empty(n * f.output_width(kind), dtype=torch.float32 if kind == OUT_MARGIN else torch.int32,
                          device="cuda")
        dev.set_option(OPT_SMALL_BATCH_ROWS, TH)
        dev.predict_device(xt.data_ptr(), int(dtype is np.float64), n, cols, F + 5, kind, out.data_ptr(),
                           out.numel(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        dev.set_option(OPT_SMALL_BATCH_ROWS, 0)
        assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


def test_rows_above_the_option_keep_the_own_walk():
    f, cats, ref = CASES["xgb-d3-63"]()
    dev = DeviceForest(f, [0])
    dev.set_option(OPT_SMALL_BATCH_ROWS, TH)
    X = rows(f, cats, TH + 1, seed=43)
    for n, state in ((TH + 1, 0), (TH, 1)):
        assert np.array_equal(dev.predict(X[:n], OUT_MARGIN), ref(X[:n], True))
        assert dev.info()["small_walk"] == state
    dev.close()


@pytest.mark.parametrize("name", ["pre-steps", "linear-leaves"])
def test_routed_forests_keep_their_path(name):
    if name == "pre-steps":
        f = sk_pipeline_cases.forest("minmax-rfc3")
        X = sk_pipeline_cases.batch("minmax-rfc3", 5, 3)
    else:
        f, cats, _ = _lgb(12, 15, 6, 31, (), linear=True)
        X = rows(f, cats, 5, seed=42).astype(np.float64)
    dev = DeviceForest(f, [0])
    want = [dev.predict(X, k) for k in (OUT_MARGIN, OUT_PREDICT, OUT_LEAF)]
    dev.set_option(OPT_SMALL_BATCH_ROWS, TH)
    for k, w in zip((OUT_MARGIN, OUT_PREDICT, OUT_LEAF), want):
        assert np.array_equal(dev.predict(X, k), w, equal_nan=True)
    assert dev.info()["small_walk"] == -1
    dev.close()


def test_negative_value_is_invalid():
    dev = case("xgb-d3-63")[3]
    with pytest.raises(TreeInferError) as e:
        dev.set_option(OPT_SMALL_BATCH_ROWS, -1)
    assert e.value.code == -1
