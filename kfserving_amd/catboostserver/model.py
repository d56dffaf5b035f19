"""CatBoostModel -- a CatBoost model served as xgbserver and lgbserver serve
theirs: ``model.json`` (CatBoost's JSON export) in the model directory, v1
``instances`` cast to float32 as CatBoost's pool stores them (NaN = missing),
the library's probability or value as the answer.  V2 tensors and ``:explain``
come from :class:`GPUForestMixin`; contributions need the document's
``leaf_weights`` (the covers) and are refused without them, as for any forest
without covers.
"""
import os
from typing import Dict

import numpy as np

from ..formats.catboost_format import load_catboost_model
from ..forest import Forest
from ..kfserving.kfmodel import KFModel
from ..kfserving.storage import Storage
from ..tree_model import GPUForestMixin

MODEL_FILE = "model.json"


class CatBoostModel(GPUForestMixin, KFModel):
    # the application route and the asyncio batcher; the native routes are not
    # taught CatBoost's input rule
    native_batching = False

    def __init__(self, name: str, model_dir: str, forest: Forest = None, background=None):
        super().__init__(name)
        self.name = name
        self.model_dir = model_dir
        if background is not None:
            self.set_background(background)
        if forest is not None:
            self._set_forest(forest)
            self.ready = True

    def load(self) -> bool:
        model_path = Storage.download(self.model_dir)
        self._set_forest(load_catboost_model(os.path.join(model_path, MODEL_FILE)))
        self._load_background(model_path)
        self.ready = True
        return self.ready

    def request_matrix(self, request: Dict) -> np.ndarray:
        return self.tensor_matrix(np.asarray(request["instances"], dtype=np.float64))

    def tensor_matrix(self, X: np.ndarray) -> np.ndarray:
        X = np.asarray(X)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        return X if X.dtype == np.float32 else X.astype(np.float32)

    def predict(self, request: Dict) -> Dict:
        try:
            result = self.predict_matrix(self.request_matrix(request))
            return {"predictions": result.tolist()}
        except Exception as e:
            raise Exception("Failed to predict %s" % e)
