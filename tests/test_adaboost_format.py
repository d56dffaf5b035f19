"""sklearn AdaBoost -> canonical forest, without a GPU: the flattened forests,
the refusals, and the tree-quantile rule's numpy restatement against sklearn."""
import numpy as np
import pytest

from kfserving_amd.forest import OUT_PREDICT, OUT_TREE_QUANTILE, TI_F32, T_ARGMAX
from kfserving_amd.formats.sklearn_format import forest_from_sklearn, save_tree_arrays
from tests import adaboost_cases as ac
from tests import canon_eval


@pytest.mark.parametrize("n_trees", sorted(ac.REGRESSORS))
def test_regressor_forest_and_rule(n_trees):
    est = ac.regressor(n_trees)
    T = len(est.estimators_)
    assert (T < n_trees) if n_trees == 300 else (T == n_trees)
    f = forest_from_sklearn(est)
    assert (f.n_trees, f.n_groups, f.leaf_width, f.input_dtype) == (T, 1, 1, TI_F32)
    assert np.array_equal(f.tree_weight, est.estimator_weights_[:T])
    assert f.meta["allow_nan"] is False and f.meta["predict_kind"] == OUT_TREE_QUANTILE
    t0 = est.estimators_[0].tree_
    leaf = t0.children_left == -1
    assert np.array_equal(f.leaf_value[:t0.node_count, 0][leaf], t0.value[leaf, 0, 0])
    sub = f.tree_subset(0, max(T // 2, 1))
    assert np.array_equal(sub.tree_weight, f.tree_weight[:max(T // 2, 1)])
    X = ac.rows(257)
    V = ac.member_predictions(est, X)
    assert np.array_equal(ac.forest_predictions(f, X), V)
    assert T != 50 or sum(len(set(r)) < len(r) for r in V.tolist()) > 20     # rows with ties
    assert np.array_equal(ac.tree_quantile_rule(V, f.tree_weight, [0.5])[:, 0], est.predict(X))


@pytest.mark.parametrize("n_classes", [2, 3])
def test_classifier_forest_labels_and_margins(n_classes):
    est = ac.classifier(n_classes)
    f = forest_from_sklearn(est)
    assert (f.n_groups, f.leaf_width, f.transform) == (n_classes, n_classes, T_ARGMAX)
    assert f.tree_weight is None and "predict_kind" not in f.meta
    assert f.average_divisor == est.estimator_weights_.sum()
    X = ac.rows(257)
    labels = est.classes_.take(canon_eval.predict(f, X.astype(np.float32), OUT_PREDICT).astype(np.int64))
    assert np.array_equal(labels, est.predict(X))


def test_refusals(tmp_path):
    from sklearn.ensemble import AdaBoostClassifier, AdaBoostRegressor
    from sklearn.linear_model import LinearRegression
    X = ac.rows(80)
    with pytest.raises(TypeError, match="LinearRegression"):
        forest_from_sklearn(AdaBoostRegressor(LinearRegression(), n_estimators=3).fit(X, X[:, 0]))
    with pytest.raises(TypeError, match="one class"):
        forest_from_sklearn(AdaBoostClassifier(n_estimators=3).fit(X, np.zeros(80)))
    est = ac.classifier(3)
    odd = AdaBoostClassifier(n_estimators=3, random_state=0).fit(X, np.arange(80) % 3)
    odd.estimators_[1] = est.estimators_[0]          # a member fitted on other classes
    with pytest.raises(TypeError, match="member 1 was fitted on classes"):
        forest_from_sklearn(odd)
    with pytest.raises(TypeError, match="AdaBoostRegressor has no tree-array"):
        save_tree_arrays(str(tmp_path / "m.npz"), ac.regressor(2))
    f = forest_from_sklearn(ac.regressor(2))
    for bad in ([1.0, -0.5], [1.0, np.nan], [1.0]):
        f.tree_weight = np.asarray(bad)
        with pytest.raises(ValueError, match="tree_weight"):
            f.validate()


def test_a_quantiles_request_skips_the_batcher():
    """KFServer --max_batchsize: a batch carries rows alone, so a request with the
    key goes to predict() by itself; the plain one still takes the batcher."""
    import asyncio
    import json
    from kfserving_amd.kfserving import KFServer
    from kfserving_amd.sklearnserver import SKLearnModel
    est, X, q = ac.random_forest(), ac.rows(5), [0.05, 0.95]
    rule = lambda Z, levels: ac.tree_quantile_rule(ac.member_predictions(est, Z), np.ones(20), levels)  # noqa: E731
    model = SKLearnModel("rf", "")
    model._set_forest(forest_from_sklearn(est))
    model.ready = True
    model.predict_matrix = lambda Z, kind=OUT_PREDICT: est.predict(Z)      # the device's stand-ins
    model.predict_quantiles = rule
    server = KFServer(max_batchsize=8, max_latency_ms=5)
    server.register_model(model)
    app = server.create_application()

    async def ask():
        got = [json.loads((await app.predict({}, json.dumps(r).encode(), "rf"))[3])["predictions"]
               for r in ({"instances": X.tolist(), "quantiles": q}, {"instances": X.tolist()})]
        for b in app._batchers.values():
            b.close()
        return got
    assert asyncio.run(ask()) == [rule(X, q).tolist(), est.predict(X).tolist()]
    assert list(app._batchers) == [("rf", "instances")]
