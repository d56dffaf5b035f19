"""Layout 12 (oblivious trees) against tests/catboost_cases, the numpy float64
restatement of CatBoost's rule over the JSON document: margins bit for bit
(both sum float64 in tree order), leaf ids, the same forest on layout 1, and
the plugin's transformed answers at RTOL.

With float64 sums a scalar leaf table is staged up to depth 10 and gathered
from depth 11; a table of three values a leaf is staged up to depth 8."""
import json

import numpy as np
import pytest

from kfserving_amd.catboostserver import CatBoostModel
from kfserving_amd.forest import OUT_LEAF, OUT_MARGIN
from kfserving_amd.formats import catboost_format as cf
from tests import catboost_cases
from tests.test_gpu_xgb_categorical import _dev

pytestmark = pytest.mark.gpu

RTOL = 1e-5
N_FEATURES = 11
MIXED = (0, 3, 7)
#        depth(s)        T   rows dim  rows' dtype
CASES = [
    (1,              1,   1,   1, np.float32),
    (6,              33,  257, 1, np.float32),
    (6,              7,   63,  3, np.float64),
    (8,              7,   257, 3, np.float32),    # the last staged depth of three float64 a leaf
    (9,              7,   63,  3, np.float64),    # ... and the first gathered one
    (8,              33,  63,  1, np.float64),
    (9,              33,  257, 1, np.float32),
    (10,             7,   257, 1, np.float64),    # the last staged depth of scalar leaves
    (11,             7,   257, 1, np.float32),    # the first gathered one
    (11,             1,   63,  1, np.float64),    # nothing staged at all
    (MIXED,          33,  257, 1, np.float32),
    (MIXED,          7,   257, 3, np.float64),
    ((0, 11, 3, 10), 7,   63,  1, np.float32),    # staged and gathered trees in one forest
]


def _rows(doc, rows, seed):
    """float32 rows with NaN, +-inf and exact borders; a batch of 63 rows has no
    NaN (its tile takes the fast step), and the last row of any batch has none
    (257 rows: a second tile of one row on the fast step)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, N_FEATURES)).astype(np.float32)
    borders = [ff["borders"] for ff in doc["features_info"]["float_features"]]
    for r in range(rows):
        j = int(rng.integers(N_FEATURES))
        X[r, j] = borders[j][int(rng.integers(len(borders[j])))]
    X[rng.random(X.shape) < 0.03] = np.inf
    X[rng.random(X.shape) < 0.03] = -np.inf
    if rows != 63:
        X[rng.random(X.shape) < 0.05] = np.nan
        X[0, :3] = np.nan
        if rows > 1:
            X[-1] = np.nan_to_num(X[-1], nan=0.5, posinf=np.inf, neginf=-np.inf)
    return X


@pytest.mark.parametrize("depth,T,rows,dim,dtype", CASES)
def test_oblivious_layout(depth, T, rows, dim, dtype):
    depths = [depth] * T if isinstance(depth, int) else [depth[i % len(depth)] for i in range(T)]
    doc = cf.json_model_doc(T, depths, N_FEATURES, dim=dim, seed=T + rows + dim)
    forest = cf.forest_from_catboost_doc(doc)
    X = _rows(doc, rows, seed=rows).astype(dtype)
    want_m, want_l = catboost_cases.raw(doc, X), catboost_cases.leaf_index(doc, X)
    dev = _dev(forest, "oblivious", dtype)
    try:
        assert dev.info()["layout"] == 12
        got_m = dev.predict(X, OUT_MARGIN).reshape(rows, dim)
        got_l = dev.predict(X, OUT_LEAF)
    finally:
        dev.close()
    assert np.array_equal(got_l, want_l)
    assert np.array_equal(got_m, want_m)
    ref = _dev(forest, "explicit", dtype)
    try:
        assert ref.info()["layout"] == 1
        assert np.array_equal(ref.predict(X, OUT_MARGIN).reshape(rows, dim), got_m)
        assert np.array_equal(ref.predict(X, OUT_LEAF), got_l)
    finally:
        ref.close()


@pytest.mark.parametrize("loss,dim", [("Logloss", 1), ("MultiClass", 3)])
def test_plugin_answers(tmp_path, loss, dim):
    doc = cf.json_model_doc(33, 6, N_FEATURES, dim=dim, loss=loss, seed=9)
    (tmp_path / "model.json").write_text(json.dumps(doc))
    model = CatBoostModel("m", str(tmp_path))
    assert model.load()
    X = _rows(doc, 257, seed=4)
    got = np.asarray(model.predict({"instances": X.astype(np.float64).tolist()})["predictions"])
    want = catboost_cases.answer(doc, X)
    np.testing.assert_allclose(got.reshape(257, dim), want, rtol=RTOL, atol=0)
    model.device_forest().close()
