"""LightGBMModel -- GPU drop-in for python/lgbserver/lgbserver/model.py:25-54.

Same constructor (name, model_dir, nthread, booster=None) and ``inputs``
request format: one DataFrame per element with ``columns=feature_name()``,
rows concatenated (:46-50), then one libtreeinfer call in float64 where the
reference called ``Booster.predict`` (:51).
"""
import os
from typing import Dict

import numpy as np

from ..formats.lightgbm_format import load_lightgbm_model
from ..forest import Forest
from ..kfserving.kfmodel import KFModel
from ..kfserving.storage import Storage
from ..tree_model import GPUForestMixin, lgb_matrix_from_inputs

BOOSTER_FILE = "model.bst"


class LightGBMModel(GPUForestMixin, KFModel):
    # request keys beside "inputs" that change the answer: KFServer sends such
    # a request to predict() alone, never through a batcher
    unbatched_request_keys = ("start_iteration", "num_iteration", "pred_early_stop",
                              "pred_early_stop_freq", "pred_early_stop_margin")
    # the objectives LightGBM early-stops (NeedAccuratePrediction() is false): every
    # other one ignores the option
    early_stop_objectives = ("binary", "multiclass", "multiclassova", "lambdarank", "rank_xendcg")

    def __init__(self, name: str, model_dir: str, nthread: int, booster: Forest = None,
                 background=None):
        super().__init__(name)
        self.name = name
        self.model_dir = model_dir
        self.nthread = nthread
        if background is not None:
            self.set_background(background)
        if booster is not None:
            self._set_forest(booster)
            self.ready = True

    def load(self) -> bool:
        model_path = Storage.download(self.model_dir)
        self._set_forest(load_lightgbm_model(os.path.join(model_path, BOOSTER_FILE)))
        self._load_background(model_path)
        self.ready = True
        return self.ready

    def feature_name(self):
        names = self._forest.feature_names
        return list(names) if names else [f"Column_{j}" for j in range(self._forest.n_features)]

    def request_matrix(self, request: Dict) -> np.ndarray:
        return lgb_matrix_from_inputs(request["inputs"], self.feature_name())

    def tensor_matrix(self, X: np.ndarray) -> np.ndarray:
        """A V2 tensor's columns in the booster's feature order, float64 (as
        ``Booster.predict(ndarray)`` reads them)."""
        X = np.asarray(X, dtype=np.float64)
        n = self._forest.n_features
        if X.ndim != 2 or X.shape[1] != n:
            raise ValueError("The number of features in data (%d) is not the same as it was "
                             "in training data (%d)." % (X.shape[-1], n))
        return X

    def iteration_trees(self, request: Dict):
        """The request's optional ``"start_iteration"`` / ``"num_iteration"``
        keys (LightGBM's own: num_iteration <= 0 or absent means every iteration
        from the start on) as a tree range; None when both are absent.  An
        iteration is num_tree_per_iteration trees."""
        if not isinstance(request, dict) or not any(k in request for k in ("start_iteration", "num_iteration")):
            return None
        f = self._forest
        per = int(f.meta.get("trees_per_iteration", f.n_groups))
        b, n = request.get("start_iteration", 0), request.get("num_iteration", -1)
        n = -1 if n is None else n
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in (b, n)):
            raise ValueError('"start_iteration" and "num_iteration" must be integers')
        n_iter = f.n_trees // per
        b = max(b, 0)
        e = n_iter if n <= 0 else min(b + n, n_iter)
        if not b < e:
            raise ValueError('"start_iteration" %d is beyond the model\'s %d iterations' % (b, n_iter))
        return b * per, e * per

    def early_stop(self, request: Dict):
        """The request's optional ``"pred_early_stop"`` (bool),
        ``"pred_early_stop_freq"`` (iterations between two tests, default 10)
        and ``"pred_early_stop_margin"`` (default 10.0), LightGBM's own, as
        (trees a round, margin); None when the option is absent, false, or --
        as in LightGBM -- the objective needs an accurate prediction."""
        keys = ("pred_early_stop", "pred_early_stop_freq", "pred_early_stop_margin")
        if not isinstance(request, dict) or not any(k in request for k in keys):
            return None
        on = request.get("pred_early_stop", False)
        freq = request.get("pred_early_stop_freq", 10)
        margin = request.get("pred_early_stop_margin", 10.0)
        if not isinstance(on, bool):
            raise ValueError('"pred_early_stop" must be true or false')
        if not isinstance(freq, int) or isinstance(freq, bool) or freq < 1:
            raise ValueError('"pred_early_stop_freq" must be an integer >= 1')
        if isinstance(margin, bool) or not isinstance(margin, (int, float)) or margin != margin:
            raise ValueError('"pred_early_stop_margin" must be a number')
        if on and any(k in request for k in ("start_iteration", "num_iteration")):
            raise ValueError('"pred_early_stop" with "start_iteration" / "num_iteration" is not served')
        f = self._forest
        objective = (f.objective or "").split()
        if not on or not objective or objective[0] not in self.early_stop_objectives:
            return None
        return freq * int(f.meta.get("trees_per_iteration", f.n_groups)), float(margin)

    def predict(self, request: Dict) -> Dict:
        try:
            stop = self.early_stop(request)
            trees = self.iteration_trees(request)
            X = self.request_matrix(request)
            if stop is not None:
                return {"predictions": self.predict_early_stop(X, *stop).tolist()}
            if trees is not None:
                return {"predictions": self.predict_tree_range(X, *trees).tolist()}
            result = self.predict_matrix(X)
            return {"predictions": result.tolist()}
        except Exception as e:
            raise Exception("Failed to predict %s" % e)

    # the native HTTP front end (kfhttp.h) reads batched v1 {"inputs": ...}
    # bodies of this model itself (kf_parse_inputs: columns by these names, the
    # subset lgb_matrix_from_inputs takes without pandas), rows as they are
    native_v1_transform = 0

    def native_v1_names(self):
        return self.feature_name()

    # V2 tensors: tensor_matrix reads the columns in the booster's order as
    # float64 (FP32 data widened exactly), the plain cast of the native route
    native_v2_transform = 0

    # KFServer's in-process batcher (kfserving_amd.batcher.ModelBatcher, kind
    # "inputs"): one request's rows as the float64 matrix its columns select,
    # then one predict over the concatenated rows of a batch
    def batch_inputs(self, request: Dict) -> np.ndarray:
        X = self.request_matrix(request)
        if X.shape[0] == 0:
            raise ValueError("no rows in the request")
        return X

    def predict_batched(self, X: np.ndarray) -> Dict:
        try:
            return {"predictions": self.predict_matrix(X).tolist()}
        except Exception as e:
            raise Exception("Failed to predict %s" % e)
