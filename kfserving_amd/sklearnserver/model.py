"""SKLearnModel -- GPU drop-in for python/sklearnserver/sklearnserver/model.py:25-54.

Same constructor (name, model_dir) and ``instances`` request format.  ``load``
finds model.joblib / .pkl / .pickle like the reference (:21-41; these files
are the user's own model, loaded with joblib exactly as the reference does)
or the pickle-free ``model.npz`` tree-array export, and flattens a
RandomForest / ExtraTrees / DecisionTree / GradientBoosting /
HistGradientBoosting estimator, or a Pipeline of imputer / scaler steps in
front of one (its steps run on the device as the forest's pre-steps);
``predict`` runs the trees through
libtreeinfer where the reference called ``_model.predict``.
"""
import os
from typing import Dict

import numpy as np

from ..formats.sklearn_format import forest_from_sklearn, load_tree_arrays
from ..kfserving.kfmodel import KFModel
from ..kfserving.storage import Storage
from ..engine import prepare_input
from ..tree_model import GPUForestMixin

MODEL_BASENAME = "model"
MODEL_EXTENSIONS = [".joblib", ".pkl", ".pickle"]
ARRAYS_EXTENSION = ".npz"


class SKLearnModel(GPUForestMixin, KFModel):  # pylint:disable=c-extension-no-member
    def __init__(self, name: str, model_dir: str):
        super().__init__(name)
        self.name = name
        self.model_dir = model_dir
        self.ready = False

    def load(self) -> bool:
        model_path = Storage.download(self.model_dir)
        paths = [os.path.join(model_path, MODEL_BASENAME + ext) for ext in MODEL_EXTENSIONS]
        for path in paths:
            if os.path.exists(path):
                import joblib
                self._set_forest(forest_from_sklearn(joblib.load(path)))
                self.ready = True
                break
        if not self.ready:
            npz = os.path.join(model_path, MODEL_BASENAME + ARRAYS_EXTENSION)
            if os.path.exists(npz):
                self._set_forest(load_tree_arrays(npz))
                self.ready = True
        return self.ready

    def _array(self, request: Dict) -> np.ndarray:
        instances = request["instances"]
        try:
            return np.array(instances)
        except Exception as e:
            raise Exception(
                "Failed to initialize NumPy array from inputs: %s, %s" % (e, instances))

    def request_matrix(self, request: Dict) -> np.ndarray:
        """sklearn's validate_data checks on the ``instances`` array."""
        f = self._forest
        if f.meta.get("pipeline"):
            return self._pipeline_matrix(self._array(request))
        X = np.asarray(self._array(request), dtype=np.float64)
        if f.meta.get("hist_gradient_boosting"):
            return self._hgb_matrix(X)
        if X.ndim != 2:
            raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
        if X.shape[1] != f.n_features:
            raise ValueError("X has %d features, but %s is expecting %d features as input."
                             % (X.shape[1], f.objective, f.n_features))
        if not f.meta.get("allow_nan", True) and np.isnan(X).any():
            raise ValueError("Input X contains NaN.")   # GradientBoosting: validate_data
        # sklearn converts to float32 (DTYPE) before its finiteness check, so a
        # finite float64 beyond the float32 range is rejected like infinity
        with np.errstate(over="ignore"):
            X32 = X.astype(np.float32)
        if np.isinf(X32).any():
            raise ValueError("Input X contains infinity or a value too large for "
                             "dtype('float32').")
        return X

    def _pipeline_matrix(self, X: np.ndarray) -> np.ndarray:
        """``Pipeline.predict``'s checks, in the order its steps make them.
        The first real step validates the array: float32 stays float32,
        anything else becomes float64; it must be 2-D, free of infinity (NaN
        passes the scalers and the imputer) and of the fitted width, and the
        step's name is in the width message.  The final estimator then casts
        to float32 and checks again: NaN reaches it only when no imputer
        precedes it and is refused by GradientBoosting; a value the steps push
        beyond float32 is refused as too large.  That last check does not
        transform the batch: every pre-step is monotone in the value and
        rounding keeps that, so a column's transformed extremes come from its
        finite minimum and maximum (and the imputer's fill), and the op chain
        runs on those 3 x F values alone."""
        f = self._forest
        who, F = f.meta["validator"], f.n_features
        X = np.asarray(X)
        if X.dtype != np.float32:
            X = np.asarray(X, dtype=np.float64)
        if X.ndim < 2:      # check_array's text: the first line, then the array and the advice
            raise ValueError("Expected 2D array, got %s array instead:\narray=%s.\n"
                             "Reshape your data either using array.reshape(-1, 1) if your data "
                             "has a single feature or array.reshape(1, -1) if it contains a "
                             "single sample." % ("1D" if X.ndim else "scalar", X))
        if X.ndim > 2:
            raise ValueError("Found array with dim %d, while dim <= 2 is required by %s."
                             % (X.ndim, who))
        if np.isinf(X).any():
            raise ValueError("Input X contains infinity or a value too large for dtype('%s')."
                             % X.dtype.name)
        if X.shape[1] != F:
            raise ValueError("X has %d features, but %s is expecting %d features as input."
                             % (X.shape[1], who, F))
        nan = np.isnan(X)
        has_nan = bool(nan.any())
        if has_nan and not f.meta.get("imputes") and not f.meta.get("allow_nan", True):
            raise ValueError("Input X contains NaN.")   # the final estimator's validate_data
        if X.shape[0] == 0:
            return X
        if has_nan:
            lo = np.where(nan, np.inf, X).min(axis=0)
            hi = np.where(nan, -np.inf, X).max(axis=0)
            lo[np.isinf(lo)] = np.nan        # a column of NaN alone
            hi[np.isinf(hi)] = np.nan
        else:
            lo, hi = X.min(axis=0), X.max(axis=0)
        E = np.stack([lo, hi, np.full(F, np.nan, dtype=X.dtype)]).astype(X.dtype)
        if f.n_pre_steps:
            with np.errstate(all="ignore"):
                for s in range(f.n_pre_steps):
                    E = f.pre_step_host(E, s)
                    if np.isinf(E).any():    # the next step's own check_array
                        raise ValueError("Input X contains infinity or a value too large for "
                                         "dtype('%s')." % X.dtype.name)
        with np.errstate(over="ignore"):
            if np.isinf(E.astype(np.float32)).any():
                raise ValueError("Input X contains infinity or a value too large for "
                                 "dtype('float32').")
        return X

    def _hgb_matrix(self, X: np.ndarray) -> np.ndarray:
        """HistGradientBoosting's ``_preprocess_X(reset=False)``: X stays
        float64, NaN and (on numerical columns) infinity pass, nothing is cast
        to float32.  Without categorical features validate_data checks the
        shape; with them the estimator's ColumnTransformer does (its name is
        in the messages) and its ordinal encoder rejects infinity on a
        categorical column.  A value the encoder does not know is missing: the
        forest's bitsets say so for integers (forest_from_hist_gradient_boosting),
        and non-integer values become NaN here, in a copy."""
        f = self._forest
        who, F = f.meta["validator"], f.n_features
        cat = np.asarray(f.meta["categorical_features"], dtype=np.int64)
        if cat.size and X.ndim == 1:
            raise ValueError("X does not contain any features, but %s is expecting %d features"
                             % (who, F))
        if cat.size == 0 and X.ndim < 2:
            raise ValueError("Expected 2D array, got %s array instead"
                             % ("1D" if X.ndim else "scalar"))
        if X.ndim > 2 and (cat.size == 0 or X.shape[1] == F):
            raise ValueError("Found array with dim %d, while dim <= 2 is required by %s."
                             % (X.ndim, f.objective))
        if X.ndim < 2 or X.shape[1] != F:
            raise ValueError("X has %d features, but %s is expecting %d features as input."
                             % (X.shape[1] if X.ndim > 1 else 0, who, F))
        if cat.size:
            C = X[:, cat]
            if np.isinf(C).any():
                raise ValueError("Input contains infinity or a value too large for "
                                 "dtype('float64').")
            stray = C != np.floor(C)         # NaN too, which stays NaN
            if stray.any():
                X = X.copy()
                X[:, cat] = np.where(stray, np.nan, C)
        return X

    def predict_tensor(self, X: np.ndarray) -> np.ndarray:
        """A V2 tensor through the same checks and label mapping as predict."""
        f = self._forest
        result = self.predict_matrix(self.request_matrix({"instances": X}))
        classes = f.meta.get("classes")
        if classes is not None:
            result = np.asarray(classes).take(result.astype(np.int64), axis=0)
        return result

    @property
    def native_v1_transform(self):
        """The native HTTP route's element rule and checks (kfhttp.h): the
        float32 cast; a value that overflows it, or a NaN the estimator
        rejects, sends the request to predict's own checks.
        HistGradientBoosting forests declare none, so the application answers
        them: the categorical columns' infinity check and non-integer rule
        (_hgb_matrix) are no element rule of the native route, and its plain
        float64 rule has not been held against _hgb_matrix on an
        ``instances`` route even for models without categorical features."""
        f = self._forest
        if f is None or f.meta.get("hist_gradient_boosting") or f.meta.get("pipeline"):
            return None   # a Pipeline's checks (_pipeline_matrix) are the application's too
        return (1 << 8) | (0 if f.meta.get("allow_nan", True) else (1 << 9))

    @property
    def native_v2_transform(self):
        """V2 tensors take request_matrix's checks and float32 cast too
        (native_rows), so regressors answer them natively with the same flags;
        a classifier's labels come back as a typed tensor, which the
        application encodes."""
        f = self._forest
        if f is None or f.meta.get("classes") is not None:
            return None
        return self.native_v1_transform

    def native_v1_labels(self):
        """A classifier's labels as its predict renders them
        (classes.take(index).tolist() -> json.dumps), for the native route."""
        import json
        classes = self._forest.meta.get("classes")
        if classes is None:
            return None
        return [json.dumps(c) for c in np.asarray(classes).tolist()]

    def native_rows(self, chunk, kind: str) -> np.ndarray:
        # the same checks for V2 tensors and instances (predict_tensor)
        X = chunk if kind == "inputs" else self.request_matrix({"instances": chunk})
        return prepare_input(self._forest, X)

    def native_predictions(self, out: np.ndarray, kind: str):
        classes = self._forest.meta.get("classes")
        if classes is not None:
            out = np.asarray(classes).take(out.astype(np.int64), axis=0)
        return out if kind == "tensor" else out.tolist()

    def predict(self, request: Dict) -> Dict:
        inputs = self._array(request)
        try:
            f = self._forest
            result = self.predict_matrix(self.request_matrix({"instances": inputs}))
            classes = f.meta.get("classes")
            if classes is not None:
                result = np.asarray(classes).take(result.astype(np.int64), axis=0)
            return {"predictions": result.tolist()}
        except Exception as e:
            raise Exception("Failed to predict %s" % e)
