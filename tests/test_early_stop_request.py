"""lgbserver's "pred_early_stop*" request keys: parsing, defaults, objective gating
and what reaches the device forest, with a stub in the device's place."""
import os

import numpy as np
import pytest

from kfserving_amd.forest import OUT_EARLY_STOP, OUT_PREDICT
from kfserving_amd.formats import lightgbm_format as lf, load_lightgbm_model
from kfserving_amd.lgbserver.model import LightGBMModel

F = 4


class StubDevice:
    def __init__(self):
        self.early_stop, self.kinds = (1, float("inf"), False), []

    def set_early_stop(self, round_trees, margin, transformed=False):
        self.early_stop = (round_trees, margin, transformed)

    def predict(self, X, kind=OUT_PREDICT):
        self.kinds.append(kind)
        return np.zeros(X.shape[0])


def _model(tmp_path, objective, K=1):
    trees = lf.synthetic_leafwise_trees(6 * K, 4, F, seed=1)
    p = os.path.join(tmp_path, "model.txt")
    lf.write_lightgbm_text(p, trees, F, objective, num_class=K)
    m = LightGBMModel("m", "", 1, booster=load_lightgbm_model(p))
    m._device_forest = StubDevice()
    inputs = [{n: [0.5, 1.5] for n in m.feature_name()}]
    return m, m._device_forest, inputs


@pytest.mark.parametrize("keys,state", [
    ({"pred_early_stop": True}, (30, 10.0, True)),                                  # LightGBM's defaults
    ({"pred_early_stop": True, "pred_early_stop_freq": 2}, (6, 10.0, True)),        # R = freq x 3 trees
    ({"pred_early_stop": True, "pred_early_stop_margin": 1}, (30, 1.0, True)),
    ({"pred_early_stop": True, "pred_early_stop_freq": 1, "pred_early_stop_margin": -0.5}, (3, -0.5, True)),
])
def test_multiclass_request_reaches_the_device(tmp_path, keys, state):
    m, dev, inputs = _model(tmp_path, "multiclass num_class:3", K=3)
    assert m.predict(dict(inputs=inputs, **keys)) == {"predictions": [0.0, 0.0]}
    assert dev.early_stop == state and dev.kinds == [OUT_EARLY_STOP]
    assert set(keys) <= set(LightGBMModel.unbatched_request_keys)     # never through a batcher


@pytest.mark.parametrize("objective,keys", [
    ("regression", {"pred_early_stop": True}),               # needs an accurate prediction: ignored
    ("binary sigmoid:1", {"pred_early_stop": False, "pred_early_stop_freq": 3}),
    ("binary sigmoid:1", {"pred_early_stop_margin": 2.0}),   # the switch defaults to off
])
def test_ignored_or_off_serves_the_plain_path(tmp_path, objective, keys):
    m, dev, inputs = _model(tmp_path, objective)
    assert m.predict(dict(inputs=inputs, **keys)) == m.predict(dict(inputs=inputs))
    assert dev.kinds == [OUT_PREDICT, OUT_PREDICT] and dev.early_stop[2] is False


@pytest.mark.parametrize("keys", [
    {"pred_early_stop": 1}, {"pred_early_stop": "true"},
    {"pred_early_stop": True, "pred_early_stop_freq": 0},
    {"pred_early_stop": True, "pred_early_stop_freq": 2.0},
    {"pred_early_stop": True, "pred_early_stop_freq": True},
    {"pred_early_stop": True, "pred_early_stop_margin": "10"},
    {"pred_early_stop": True, "pred_early_stop_margin": float("nan")},
    {"pred_early_stop": True, "num_iteration": 3},
    {"pred_early_stop": True, "start_iteration": 1},
])
def test_malformed_or_combined_keys_raise(tmp_path, keys):
    m, dev, inputs = _model(tmp_path, "binary sigmoid:1")
    with pytest.raises(ValueError):
        m.early_stop(dict(inputs=inputs, **keys))
    assert dev.kinds == []
