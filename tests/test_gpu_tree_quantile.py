"""TI_OUTPUT_TREE_QUANTILE on the GPU, bit for bit: fitted AdaBoost models against
sklearn through SKLearnModel, synthetic forests and RandomForest quantiles
against the rule's numpy restatement (tests/adaboost_cases), and the plumbing."""
import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import OUT_MARGIN, OUT_TREE_QUANTILE, TREE_QUANTILE_MAX_TREES
from kfserving_amd.formats.sklearn_format import forest_from_sklearn
from tests import adaboost_cases as ac

pytestmark = pytest.mark.gpu
CAP = TREE_QUANTILE_MAX_TREES


def served(est, name="m"):
    from kfserving_amd.sklearnserver import SKLearnModel
    model = SKLearnModel(name, "")
    model._set_forest(forest_from_sklearn(est))
    model.devices = [0]
    model.ready = True
    return model


@pytest.mark.parametrize("n_trees", sorted(ac.REGRESSORS))
def test_adaboost_regressor_equals_sklearn(n_trees):
    est = ac.regressor(n_trees)
    model = served(est)
    X = ac.rows(257)
    want = est.predict(X)
    for n in (1, 64, 65, 257):      # a lone row, a full and a ragged workgroup, several
        assert model.predict({"instances": X[:n].tolist()})["predictions"] == want[:n].tolist()
    assert np.array_equal(model.predict_tensor(X.astype(np.float32)), want)
    assert model.predict_tensor(X).tobytes() == want.tobytes()        # a second call: the same bits


def quantiles(f, X, q):
    dev = DeviceForest(f, devices=[0])
    try:
        dev.set_quantiles(q)
        return dev.predict(X, OUT_TREE_QUANTILE).reshape(X.shape[0], len(q))
    finally:
        dev.close()


_RNG = np.random.default_rng(3)
SYNTHETIC = {   # trees, weights, value-scale period of the copies, levels
    "ties": (40, _RNG.random(40), 1, [0.5]),                 # every tree twice: whole rows tie
    "zero-ends": (60, np.where(np.arange(60) % 20 < 14, 0.0, _RNG.random(60)), 3, [0.0, 0.5, 1.0]),
    "on-threshold": (4, np.ones(4), 1, [0.25, 0.5, 0.75]),   # 1 + 1 lands on 0.5 * 4 exactly
    "eight-keys": (300, None, 7, [0.1, 0.9]),                # the largest network held in registers
    "lds-1024": (600, _RNG.random(600), 11, [0.0, 0.3, 0.5, 1.0]),   # four rows a workgroup in LDS
    "cap": (CAP, _RNG.random(CAP), 13, [0.05, 0.5, 0.95]),
}


@pytest.mark.parametrize("case", sorted(SYNTHETIC))
def test_synthetic_forests_equal_the_rule(case):
    n_trees, weights, period, q = SYNTHETIC[case]
    f = ac.copies_forest(n_trees, weights, period)
    X = ac.rows(70 if n_trees <= 300 else 9, dtype=np.float32)
    w = np.ones(n_trees) if weights is None else weights
    want = ac.tree_quantile_rule(ac.forest_predictions(f, X), w, q)
    assert np.array_equal(quantiles(f, X, q), want)


def test_random_forest_quantiles():
    est = ac.random_forest()
    q = [0.0, 0.05, 0.5, 0.95, 1.0]
    X = ac.rows(257)
    V = ac.member_predictions(est, X)
    want = ac.tree_quantile_rule(V, np.ones(20), q)
    got = quantiles(forest_from_sklearn(est), X.astype(np.float32), q)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 0], V.min(axis=1)) and np.array_equal(got[:, 4], V.max(axis=1))
    model = served(est)
    assert model.predict({"instances": X.tolist(), "quantiles": q})["predictions"] == want.tolist()
    with pytest.raises(Exception, match="levels in"):
        model.predict({"instances": X[:2].tolist(), "quantiles": [1.5]})
    with pytest.raises(Exception, match='"quantiles" is served for'):
        served(ac.classifier(2)).predict({"instances": X[:2].tolist(), "quantiles": [0.5]})


@pytest.mark.parametrize("n_classes", [2, 3])
def test_adaboost_classifier(n_classes):
    est = ac.classifier(n_classes)
    model = served(est)
    X = ac.rows(257)
    assert model.predict({"instances": X.tolist()})["predictions"] == est.predict(X).tolist()
    if n_classes == 3:
        m = model.predict_matrix(model.request_matrix({"instances": X}), OUT_MARGIN)
        assert np.array_equal(m, est.decision_function(X))


def test_chunked_host_pipeline_is_bit_identical(monkeypatch):
    est = ac.regressor(50)
    f = forest_from_sklearn(est)
    X = np.tile(ac.rows(2000, dtype=np.float32), (6, 1))     # 4 * T = 200 B a row: 5,184-row chunks
    dev = DeviceForest(f, devices=[0])
    try:
        base = dev.info()["device_bytes"]
        one = dev.predict(X, OUT_TREE_QUANTILE)
        n_values = sum(m.tree_.node_count for m in est.estimators_)
        assert dev.info()["device_bytes"] - base == 8 * (n_values + 50) + 8 * 51   # values, weights; bases
        monkeypatch.setenv("TI_CHUNK_MB", "1")
        assert dev.predict(X, OUT_TREE_QUANTILE).tobytes() == one.tobytes()
        monkeypatch.delenv("TI_CHUNK_MB")
        assert np.array_equal(one[:2000], est.predict(X[:2000]))
        assert dev.output_shape(OUT_TREE_QUANTILE, 10) == (10, 1)
        for bad in ([], [0.5] * 9, [-0.1], [1.1], [np.nan]):
            with pytest.raises(TreeInferError) as e:
                dev.set_quantiles(bad)
            assert e.value.code == -1
        dev.set_quantiles([0.1, 0.9])
        assert dev.output_shape(OUT_TREE_QUANTILE, 10) == (20, 1)
        assert dev.predict(X[:65], OUT_TREE_QUANTILE).shape == (65, 2)
        assert np.array_equal(quantiles(f, X[:65], [0.5])[:, 0], one[:65])   # another handle: its own levels
    finally:
        dev.close()


def test_forests_the_kind_refuses():
    clf = forest_from_sklearn(ac.classifier(3))
    dup = ac.copies_forest(3, None)
    dup.leaf_id = np.zeros_like(dup.leaf_id)                  # not distinct within a tree
    big = ac.copies_forest(CAP + 1, None)                     # one tree above the cap
    X = ac.rows(4, dtype=np.float32)
    for f, why in ((clf, "leaf_width == 1 and n_groups == 1"), (dup, "not distinct"),
                   (big, "at most 4096 trees")):
        dev = DeviceForest(f, devices=[0])
        try:
            with pytest.raises(TreeInferError, match=why) as e:
                dev.predict(X, OUT_TREE_QUANTILE)
            assert e.value.code == -4
            if f is big:                                      # and its margins are still served
                in_tree_order = np.cumsum(ac.forest_predictions(f, X), axis=1)[:, -1]
                assert np.array_equal(dev.predict(X, OUT_MARGIN).ravel(), in_tree_order)
        finally:
            dev.close()
    bad = ac.copies_forest(3, [1.0, -1.0, 1.0])
    bad.validate = lambda: None                                # the library's own check
    with pytest.raises(TreeInferError, match="tree_weight") as e:
        DeviceForest(bad, devices=[0])
    assert e.value.code == -1
