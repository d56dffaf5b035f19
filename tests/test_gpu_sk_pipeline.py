"""sklearn Pipelines on the device, held to sklearn 1.7.2 itself bit for bit:
the pre-pass alone (DeviceForest.pretransform against Pipeline[:-1].transform),
padded rows, SKLearnModel.predict against Pipeline.predict for every case of
tests/sk_pipeline_cases, every output kind against the step-less forest fed
sklearn's own transformed rows (the code path before pre-steps existed), the
K = 20 classifier through group parts, repeated calls, memory, and the
argument errors.  No tolerance anywhere."""
import dataclasses
import functools

import numpy as np
import pytest

from kfserving_amd.engine import DeviceForest, TreeInferError
from kfserving_amd.forest import (OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_INTERACT, OUT_LEAF,
                                  OUT_MARGIN, OUT_PREDICT, PRE_SUB, TI_F32, TI_F64)
from kfserving_amd.formats.sklearn_format import forest_from_sklearn
from tests import sk_pipeline_cases as pc

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 257, 1000)      # below, at and past a wave; past a 256-lane workgroup
DTYPES = [np.float64, np.float32]


def _stepless(f):
    """The same trees without the steps: fed float32 rows, the engine's path
    as it was before pre-steps."""
    return dataclasses.replace(f, pre_ops=None, pre_consts=None, input_dtype=TI_F32,
                               meta=dict(f.meta))


@functools.lru_cache(maxsize=None)
def _chain(F):
    """imputer -> standard -> min-max -> robust -> max-abs (8 operations) in
    front of a depth-3 tree on F columns."""
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import MaxAbsScaler, MinMaxScaler, RobustScaler, StandardScaler
    from sklearn.tree import DecisionTreeRegressor
    X = pc.rows(300, 40 + F, True, cols=F)
    pipe = Pipeline([("imp", SimpleImputer(strategy="median")), ("std", StandardScaler()),
                     ("mm", MinMaxScaler()), ("rob", RobustScaler()), ("ma", MaxAbsScaler()),
                     ("dt", DecisionTreeRegressor(max_depth=3, random_state=0))])
    return pipe.fit(X, np.nan_to_num(X[:, 0]))


# ------------------------------------------------------------ the pre-pass alone
@pytest.mark.parametrize("dtype", DTYPES, ids=["x64", "x32"])
@pytest.mark.parametrize("F", [1, 3, 20, 33])
def test_pretransform_equals_sklearn_transform(F, dtype):
    pipe = _chain(F)
    f = forest_from_sklearn(pipe)
    assert f.n_pre_steps == 8 and f.n_features == F
    dev = DeviceForest(f, [0])
    try:
        assert dev.info()["pre_steps"] == 8
        for n in ROWS:
            X = pc.rows(n, 100 + n, True, cols=F).astype(dtype)
            want = pipe[:-1].transform(X).astype(np.float32)
            got = dev.pretransform(X)
            assert got.dtype == np.float32 and got.shape == (n, F)
            assert np.array_equal(pc.bits(got), pc.bits(want)), (F, n)
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["x64", "x32"])
def test_pretransform_subnormal_column_signed_zeros_and_nan(dtype):
    """maxabs-sub-rf divides by a scale of 1: the tiny column comes out in
    float32's subnormal range, NaN stays NaN (no imputer) and -0.0 stays -0.0."""
    name = "maxabs-sub-rf"
    dev = DeviceForest(pc.forest(name), [0])
    try:
        for n in ROWS:
            X = pc.rows(n, 7 + n, True).astype(dtype)
            want = pc.transformed(name, X).astype(np.float32)
            got = dev.pretransform(X)
            assert np.array_equal(pc.bits(got), pc.bits(want)), n
        tiny = np.abs(want[:, pc.F - 1])
        assert ((tiny > 0) & (tiny < np.finfo(np.float32).tiny)).any()
        assert np.isnan(want).any() and (pc.bits(want) == 0x80000000).any()
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=["x64", "x32"])
def test_pretransform_constants_past_the_lds_budget(dtype):
    """8 steps x 600 columns = 38,400 B of constants: read from global memory.
    3,600 rows are 2.16M elements, more than one pass of the capped grid."""
    f = pc.wide_forest()
    assert f.n_pre_steps * f.n_features * 8 > 32 * 1024
    dev = DeviceForest(f, [0])
    try:
        for n in (1, 257, 3600):
            X = pc.rows(n, 300 + n, True, cols=f.n_features).astype(dtype)
            got = dev.pretransform(X)
            assert np.array_equal(pc.bits(got), pc.bits(pc.apply_steps(f, X))), n
    finally:
        dev.close()


def test_cases_pretransform_every_case():
    for name in pc.CASES:
        dev = DeviceForest(pc.forest(name), [0])
        try:
            for dtype in DTYPES:
                X = pc.rows(257, 17, True).astype(dtype)
                want = pc.transformed(name, X).astype(np.float32)
                assert np.array_equal(pc.bits(dev.pretransform(X)), pc.bits(want)), (name, dtype)
        finally:
            dev.close()


def test_pretransform_without_steps_is_the_cast():
    plain = _stepless(pc.forest("imp-std-rf"))
    dev = DeviceForest(dataclasses.replace(plain, input_dtype=TI_F64), [0])
    try:
        assert dev.info()["pre_steps"] == 0
        for n in (1, 65, 1000):
            X = pc.rows(n, 9, True)
            X[0, 0] = 1e300                      # overflows to +inf
            X[0, 1] = -1e-50                     # underflows to -0.0
            with np.errstate(over="ignore"):
                want = X.astype(np.float32)
            assert np.array_equal(pc.bits(dev.pretransform(X)), pc.bits(want))
            x32 = X.astype(np.float32)
            assert np.array_equal(pc.bits(dev.pretransform(x32)), pc.bits(x32))
    finally:
        dev.close()


# ------------------------------------------------------------------ padded rows
@pytest.mark.parametrize("dtype", DTYPES, ids=["x64", "x32"])
def test_padded_rows_through_predict_device(dtype):
    import torch
    name = "imp-std-rf"
    f, pipe = pc.forest(name), pc.fitted(name)
    rows, stride = 321, pc.F + 5
    X = pc.batch(name, rows, 33).astype(dtype)
    padded = np.full((rows, stride), 12345.0, dtype=dtype)     # a value that would move rows
    padded[:, :pc.F] = X
    dev = DeviceForest(f, [0])
    try:
        xdt = TI_F32 if dtype == np.float32 else TI_F64
        xd, xp = torch.from_numpy(X).cuda(), torch.from_numpy(padded).cuda()
        od = torch.zeros(rows, dtype=torch.float64, device="cuda")
        op = torch.zeros(rows, dtype=torch.float64, device="cuda")
        tp = torch.zeros((rows, pc.F), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dev.predict_device(xd.data_ptr(), xdt, rows, pc.F, pc.F, OUT_PREDICT, od.data_ptr(), rows)
        dev.predict_device(xp.data_ptr(), xdt, rows, pc.F, stride, OUT_PREDICT, op.data_ptr(), rows)
        dev.pretransform_device(xp.data_ptr(), xdt, rows, pc.F, stride, tp.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(op.cpu().numpy(), od.cpu().numpy())
        assert np.array_equal(od.cpu().numpy(), pipe.predict(X))
        assert np.array_equal(pc.bits(tp.cpu().numpy()),
                              pc.bits(pc.transformed(name, X).astype(np.float32)))
    finally:
        dev.close()


# ------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", pc.CASES)
def test_sklearnserver_predict_equals_pipeline_predict(name, tmp_path):
    import joblib
    from kfserving_amd.sklearnserver import SKLearnModel
    pipe = pc.fitted(name)
    joblib.dump(pipe, str(tmp_path / "model.joblib"))
    model = SKLearnModel(name, str(tmp_path))
    assert model.load()
    assert model._forest.meta["pipeline"] is True
    X = pc.batch(name, 1000, 51)
    assert np.isnan(X).any() == pc.admits_nan(name)
    want = pipe.predict(X)
    got = model.predict({"instances": X.tolist()})["predictions"]
    assert got == want.tolist()                                     # labels and values, exact
    X32 = X.astype(np.float32)
    got32 = model.predict_tensor(X32)
    want32 = pipe.predict(X32)
    assert got32.dtype == want32.dtype and np.array_equal(got32, want32)
    if not pc.admits_nan(name):
        X[5, 2] = np.nan
        with pytest.raises(Exception, match="Input X contains NaN"):
            model.predict({"instances": X.tolist()})
    model.device_forest().close()


def test_explain_sums_to_the_pipeline_prediction(tmp_path):
    """:explain goes through GPUForestMixin unchanged: contributions of the
    forest on the transformed columns; a row sums to Pipeline.predict."""
    import joblib
    from kfserving_amd.sklearnserver import SKLearnModel
    pipe = pc.fitted("imp-std-rf")
    joblib.dump(pipe, str(tmp_path / "model.joblib"))
    model = SKLearnModel("p", str(tmp_path))
    assert model.load()
    X = pc.batch("imp-std-rf", 9, 2)
    exp = np.asarray(model.explain({"instances": X.tolist()})["explanations"])
    assert exp.shape == (9, pc.F + 1)
    # the sum of F + 1 float64 terms against the forest's own sum: 1e-9 is the
    # float64 bound the contribution tests of this suite use
    np.testing.assert_allclose(exp.sum(axis=1), pipe.predict(X), rtol=1e-9, atol=1e-9)
    model.device_forest().close()


# ------------------------------------------------------------ every output kind
@pytest.mark.parametrize("dtype", DTYPES, ids=["x64", "x32"])
def test_every_output_kind_reads_the_transformed_rows(dtype):
    name = "imp-std-rf"
    f, pipe = pc.forest(name), pc.fitted(name)
    X = pc.batch(name, 300, 77).astype(dtype)
    Xt = pc.transformed(name, X).astype(np.float32)
    dev, ref = DeviceForest(f, [0]), DeviceForest(_stepless(f), [0])
    try:
        assert np.array_equal(dev.predict(X, OUT_LEAF), pipe[-1].apply(pc.transformed(name, X)))
        assert np.array_equal(dev.predict(X, OUT_PREDICT), pipe.predict(X))
        for kind in (OUT_MARGIN, OUT_LEAF, OUT_CONTRIB, OUT_INTERACT, OUT_CONTRIB_APPROX):
            got, want = dev.predict(X, kind), ref.predict(Xt, kind)
            assert got.shape == want.shape and got.dtype == want.dtype
            assert np.array_equal(got.view(np.uint64 if got.dtype == np.float64 else np.uint32),
                                  want.view(np.uint64 if want.dtype == np.float64 else np.uint32)), kind
    finally:
        dev.close()
        ref.close()


# ------------------------------------------------------------------ group parts
@pytest.mark.parametrize("dtype", DTYPES, ids=["x64", "x32"])
def test_twenty_classes_transform_once_under_group_parts(dtype):
    name = "std-rfc20"
    f, pipe = pc.forest(name), pc.fitted(name)
    assert f.n_groups == 20 and f.leaf_width == 20          # two parts: 16 + 4 classes
    X = pc.batch(name, 700, 8).astype(dtype)
    Xt = pc.transformed(name, X)
    dev, ref = DeviceForest(f, [0]), DeviceForest(_stepless(f), [0])
    try:
        for _ in range(2):
            assert np.array_equal(dev.predict(X, OUT_MARGIN), pipe.predict_proba(X))
            lab = f.meta["classes"].take(dev.predict(X, OUT_PREDICT).astype(np.int64))
            assert np.array_equal(lab, pipe.predict(X))
            assert np.array_equal(dev.predict(X, OUT_LEAF), pipe[-1].apply(Xt))
            for kind in (OUT_CONTRIB, OUT_CONTRIB_APPROX):
                assert np.array_equal(dev.predict(X[:70], kind),
                                      ref.predict(Xt[:70].astype(np.float32), kind)), kind
        grown = dev.info()["device_bytes"] - ref.info()["device_bytes"]
        assert grown == 2 * 4 + 2 * pc.F * 8                # uploaded once, not once a part
    finally:
        dev.close()
        ref.close()


# --------------------------------------------------- repeated calls and memory
def test_repeated_calls_one_handle():
    name = "imp-std-gb"
    pipe = pc.fitted(name)
    dev = DeviceForest(pc.forest(name), [0])
    try:
        for n, seed in ((1, 1), (1000, 2), (1, 3), (257, 4), (1000, 5)):
            X = pc.batch(name, n, seed)
            assert np.array_equal(dev.predict(X, OUT_PREDICT).reshape(n), pipe.predict(X)), n
    finally:
        dev.close()


def test_device_bytes_and_memory_over_cycles():
    """device_bytes grows by exactly the op codes and the constants, and eight
    create / predict (1, 1,000, 1 rows) / close cycles leave free device memory
    within 4 x device_bytes (the bound of the suite's other scratch tests; the
    forest is above 1 MiB so that the allocator's own slack stays inside it)."""
    import torch
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.impute import SimpleImputer
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import StandardScaler
    X = pc.rows(6000, 61, True)
    pipe = Pipeline([("imp", SimpleImputer()), ("std", StandardScaler()),
                     ("rf", RandomForestRegressor(n_estimators=30, random_state=0))])
    pipe.fit(X, np.nan_to_num(X[:, 1] * X[:, 2]))
    f = forest_from_sklearn(pipe)
    batches = [pc.rows(n, 70 + i, True) for i, n in enumerate((1, 1000, 1))]
    wants = [pipe.predict(b) for b in batches]

    def cycle(forest):
        dev = DeviceForest(forest, [0])
        try:
            start = dev.info()["device_bytes"]
            for b, w in zip(batches, wants):
                assert np.array_equal(dev.predict(b, OUT_PREDICT).reshape(len(w)), w)
            assert dev.info()["device_bytes"] == start     # scratch is not forest memory
            return start
        finally:
            dev.close()
    plain = DeviceForest(_stepless(f), [0])
    base = plain.info()["device_bytes"]
    plain.close()
    nbytes = cycle(f)
    assert nbytes - base == 3 * 4 + 3 * pc.F * 8
    assert nbytes >= 1 << 20, nbytes
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(8):
        assert cycle(f) == nbytes
    torch.cuda.synchronize()
    dropped = free0 - torch.cuda.mem_get_info(0)[0]
    print(f"device_bytes {nbytes}, free memory dropped by {dropped} over 8 cycles")
    assert dropped < 4 * nbytes


# --------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_handle_serving():
    import torch
    name = "imp-std-rf"
    f, pipe = pc.forest(name), pc.fitted(name)
    X = pc.batch(name, 65, 3)
    want = pipe.predict(X)
    dev = DeviceForest(f, [0])
    try:
        def serves():
            assert np.array_equal(dev.predict(X, OUT_PREDICT), want)
        serves()
        xd = torch.from_numpy(X).cuda()
        out = torch.zeros(65, dtype=torch.float64, device="cuda")
        tp = torch.zeros((65, pc.F), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(TreeInferError) as e:        # n_cols != n_features
            dev.predict_device(xd.data_ptr(), TI_F64, 65, pc.F - 1, pc.F, OUT_PREDICT,
                               out.data_ptr(), 65)
        assert e.value.code == -1
        serves()
        with pytest.raises(TreeInferError) as e:
            dev.pretransform_device(xd.data_ptr(), TI_F64, 65, pc.F - 1, pc.F, tp.data_ptr())
        assert e.value.code == -1
        serves()
        with pytest.raises(TreeInferError) as e:        # 17 steps
            DeviceForest(dataclasses.replace(
                f, pre_ops=np.full(17, PRE_SUB, dtype=np.int32),
                pre_consts=np.zeros((17, pc.F))), [0])
        assert e.value.code == -4
        serves()
        with pytest.raises(TreeInferError) as e:        # an unknown op code
            DeviceForest(dataclasses.replace(f, pre_ops=np.array([0, 1, 9], dtype=np.int32)), [0])
        assert e.value.code == -1
        serves()
        DeviceForest(dataclasses.replace(                # 16 steps load
            f, pre_ops=np.full(16, PRE_SUB, dtype=np.int32),
            pre_consts=np.zeros((16, pc.F))), [0]).close()
        serves()
    finally:
        dev.close()
