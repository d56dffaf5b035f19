"""sklearn Pipelines flattened to a forest with pre-steps (no GPU): the steps'
numpy restatement against ``Pipeline[:-1].transform`` bit for bit, the forest
on the transformed rows against ``Pipeline.predict``, the loader's refusals,
and SKLearnModel.request_matrix against the messages of ``Pipeline.predict``
(installed sklearn 1.7.2)."""
import dataclasses

import numpy as np
import pytest

from kfserving_amd.forest import PRE_DIV, PRE_FILL_NAN, PRE_SUB, TI_F32, TI_F64
from kfserving_amd.formats.sklearn_format import forest_from_sklearn, save_tree_arrays
from tests import canon_eval as ce
from tests import sk_pipeline_cases as pc


def _labels(f, out):
    classes = f.meta.get("classes")
    return out if classes is None else np.asarray(classes).take(out.astype(np.int64))


def _served(name):
    from kfserving_amd.sklearnserver import SKLearnModel
    m = SKLearnModel(name, "")
    m._set_forest(pc.forest(name))
    return m


def _first_line(fn):
    with pytest.raises(ValueError) as e:
        fn()
    return str(e.value).splitlines()[0]


# ------------------------------------------------------------------ the steps
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["x64", "x32"])
@pytest.mark.parametrize("name", pc.CASES)
def test_steps_reproduce_transform_and_predict(name, dtype):
    f, pipe = pc.forest(name), pc.fitted(name)
    X = pc.batch(name, 500, 21).astype(dtype)
    got = pc.apply_steps(f, X)
    want = pc.transformed(name, X)
    assert want.dtype == dtype                       # the scalers keep the element type
    assert np.array_equal(pc.bits(got), pc.bits(want.astype(np.float32))), name
    assert np.array_equal(_labels(f, ce.predict(f, got)), pipe.predict(X)), name


def test_flattened_fields():
    f = pc.forest("imp-std-rf")
    assert f.meta["pipeline"] is True and f.meta["validator"] == "SimpleImputer"
    assert f.input_dtype == TI_F64 and f.n_pre_steps == 3
    assert f.pre_ops.tolist() == [PRE_FILL_NAN, PRE_SUB, PRE_DIV]
    assert f.pre_ops.dtype == np.int32 and f.pre_consts.dtype == np.float64
    assert f.pre_consts.shape == (3, pc.F) and f.pre_consts.flags.c_contiguous
    pipe = pc.fitted("imp-std-rf")
    assert np.array_equal(f.pre_consts[0], pipe["imp"].statistics_)
    assert np.array_equal(f.pre_consts[1], pipe["std"].mean_)
    assert np.array_equal(f.pre_consts[2], pipe["std"].scale_)
    assert pc.forest("std-nomean-dt").pre_ops.tolist() == [PRE_DIV]
    assert pc.forest("passthrough-std-rf").meta["validator"] == "StandardScaler"
    assert pc.forest("std-rfc20").n_groups == 20
    # the steps survive validate / contiguous / replace
    g = dataclasses.replace(f).contiguous()
    g.validate()
    assert np.array_equal(g.pre_ops, f.pre_ops) and np.array_equal(g.pre_consts, f.pre_consts)
    with pytest.raises(ValueError, match="pre_consts"):
        dataclasses.replace(f, pre_consts=f.pre_consts[:2]).validate()
    with pytest.raises(ValueError, match="pre_ops and pre_consts"):
        dataclasses.replace(f, pre_consts=None).validate()


def test_only_passthrough_steps_is_the_bare_estimator():
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.pipeline import Pipeline
    X = pc.rows(200, 3)
    pipe = Pipeline([("skip", "passthrough"),
                     ("rf", RandomForestRegressor(n_estimators=3, max_depth=3, random_state=0))])
    pipe.fit(X, X[:, 1])
    f = forest_from_sklearn(pipe)
    assert f.n_pre_steps == 0 and f.input_dtype == TI_F32 and f.meta["pipeline"] is True
    assert np.array_equal(ce.predict(f, X.astype(np.float32)), pipe.predict(X))


def test_tree_shard_slice_keeps_the_steps():
    f = pc.forest("imp-std-rf")
    s = f.tree_subset(3, 7, keep_base=False)
    assert s.n_trees == 4 and s.input_dtype == TI_F64
    assert np.array_equal(s.pre_ops, f.pre_ops) and np.array_equal(s.pre_consts, f.pre_consts)
    s.contiguous().validate()
    X = pc.batch("imp-std-rf", 50, 4)
    assert np.array_equal(pc.apply_steps(s, X), pc.apply_steps(f, X), equal_nan=True)


# ------------------------------------------------------------------- refusals
def _fit(steps, n_classes=0):
    from sklearn.pipeline import Pipeline
    X = pc.rows(120, 9)
    y = (X[:, 1] > -3).astype(int) if n_classes else X[:, 1]
    return Pipeline(steps).fit(X, y)


def _tree():
    from sklearn.tree import DecisionTreeRegressor
    return DecisionTreeRegressor(max_depth=2, random_state=0)


def test_refusals_name_the_step():
    from sklearn.compose import ColumnTransformer
    from sklearn.decomposition import PCA
    from sklearn.ensemble import HistGradientBoostingRegressor
    from sklearn.impute import SimpleImputer
    from sklearn.linear_model import LinearRegression
    from sklearn.pipeline import Pipeline
    from sklearn.preprocessing import MinMaxScaler, StandardScaler
    bad = [
        ([("pca", PCA(n_components=3)), ("dt", _tree())], r"'pca' \(PCA\)"),
        ([("ct", ColumnTransformer([("s", StandardScaler(), [0, 1])], remainder="passthrough")),
          ("dt", _tree())], r"'ct' \(ColumnTransformer\)"),
        ([("mm", MinMaxScaler(clip=True)), ("dt", _tree())], r"'mm' \(MinMaxScaler\).*clip"),
        ([("inner", Pipeline([("s", StandardScaler())])), ("dt", _tree())], r"'inner' \(Pipeline\)"),
        ([("std", StandardScaler()), ("hgb", HistGradientBoostingRegressor(max_iter=2))],
         r"'hgb' \(HistGradientBoostingRegressor\)"),
        ([("std", StandardScaler()), ("lr", LinearRegression())], r"'lr' \(LinearRegression\)"),
        ([("ind", SimpleImputer(add_indicator=True)), ("dt", _tree())],
         r"'ind' \(SimpleImputer\).*add_indicator"),
        ([("imp", SimpleImputer(missing_values=-1.0)), ("dt", _tree())],
         r"'imp' \(SimpleImputer\).*missing_values"),
    ]
    for steps, pattern in bad:
        with pytest.raises(TypeError, match=pattern):
            forest_from_sklearn(_fit(steps))
    # an imputer that dropped an all-missing column
    X = pc.rows(120, 9)
    X[:, 2] = np.nan
    with pytest.warns(UserWarning):
        dropped = Pipeline([("imp", SimpleImputer()), ("dt", _tree())]).fit(X, X[:, 1])
    with pytest.raises(TypeError, match=r"'imp' \(SimpleImputer\)"):
        forest_from_sklearn(dropped)
    # more than 16 operations in total: nine StandardScalers are 18
    many = [("s%d" % i, StandardScaler()) for i in range(9)] + [("dt", _tree())]
    with pytest.raises(TypeError, match="18 per-column operations"):
        forest_from_sklearn(_fit(many))
    # eight are 16, and load
    assert forest_from_sklearn(_fit(many[1:])).n_pre_steps == 16
    # the bare refusal stays what it was
    with pytest.raises(TypeError, match="^sklearn estimator LinearRegression is not a supported"):
        forest_from_sklearn(LinearRegression().fit(X[:, :2], X[:, 1]))


def test_npz_export_refuses_a_pipeline(tmp_path):
    with pytest.raises(TypeError):
        save_tree_arrays(str(tmp_path / "model.npz"), pc.fitted("imp-std-rf"))


# ----------------------------------------------------------- request checks
def test_request_matrix_raises_what_pipeline_predict_raises():
    good = pc.rows(3, 2)
    for name in ("imp-std-rf", "std-gb", "minmax-rfc3", "passthrough-std-rf"):
        m, pipe = _served(name), pc.fitted(name)
        step = pc.forest(name).meta["validator"]
        bad = {
            "width": good[:, :3],
            "1-D": good[0],
            "inf": np.where(np.arange(pc.F) == 2, np.inf, good),
            "overflow": np.where(np.arange(pc.F) == 1, 1e300, good),
        }
        for what, X in bad.items():
            want = _first_line(lambda: pipe.predict(X))
            got = _first_line(lambda: m.request_matrix({"instances": X.tolist()}))
            assert got == want, (name, what, got, want)
        assert "X has 3 features, but %s is expecting 6 features as input." % step == \
            _first_line(lambda: m.request_matrix({"instances": good[:, :3].tolist()}))
        assert _first_line(lambda: m.request_matrix({"instances": [1.0, 2.0]})).startswith(
            "Expected 2D array, got 1D array instead")
        assert _first_line(lambda: m.request_matrix({"instances": bad["inf"].tolist()})) == \
            "Input X contains infinity or a value too large for dtype('float64')."
        assert _first_line(lambda: m.request_matrix({"instances": bad["overflow"].tolist()})) == \
            "Input X contains infinity or a value too large for dtype('float32')."


def test_nan_is_refused_only_without_an_imputer():
    X = pc.rows(5, 3)
    X[2, 4] = np.nan
    want = _first_line(lambda: pc.fitted("std-gb").predict(X))
    assert want == "Input X contains NaN."
    assert _first_line(lambda: _served("std-gb").request_matrix({"instances": X.tolist()})) == want
    for name in ("imp-std-gb", "imp-std-rf", "std-rfc20"):
        pc.fitted(name).predict(X)                                   # sklearn takes it
        out = _served(name).request_matrix({"instances": X.tolist()})
        assert out.dtype == np.float64 and np.array_equal(out, X, equal_nan=True)


def test_float32_edge_after_scaling():
    """std-nomean-dt divides column 1 by its scale: the largest float32 times
    that scale, taken one float64 down, lands inside the float32 range after
    the step; twice it lands outside.  Both as sklearn answers."""
    name = "std-nomean-dt"
    m, pipe = _served(name), pc.fitted(name)
    scale = float(pipe["std"].scale_[1])
    fmax = float(np.finfo(np.float32).max)
    inside = np.nextafter(fmax * scale, 0.0)
    X = pc.rows(2, 5)
    X[0, 1] = inside
    X[1, 1] = -inside
    assert np.isfinite(pipe[:-1].transform(X).astype(np.float32)).all()
    pipe.predict(X)
    assert np.array_equal(m.request_matrix({"instances": X.tolist()}), X)
    X[0, 1] = 2 * inside
    want = _first_line(lambda: pipe.predict(X))
    assert want == "Input X contains infinity or a value too large for dtype('float32')."
    assert _first_line(lambda: m.request_matrix({"instances": X.tolist()})) == want


def test_request_matrix_element_types():
    m = _served("imp-std-rf")
    ints = [[1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1]]
    assert m.request_matrix({"instances": ints}).dtype == np.float64       # as the scalers make them
    x32 = pc.rows(4, 8).astype(np.float32)
    out = m.request_matrix({"instances": x32})
    assert out.dtype == np.float32 and np.array_equal(out, x32)
    assert m.native_v1_transform is None and m.native_v2_transform is None
    # a float32 tensor that overflows inside a step is refused in its own type
    x32[1, 4] = np.float32(3e38)
    small = dataclasses.replace(pc.forest("std-nomean-dt"),
                                pre_consts=np.full((1, pc.F), 1e-3), meta=dict(pc.forest("std-nomean-dt").meta))
    from kfserving_amd.sklearnserver import SKLearnModel
    ms = SKLearnModel("small", "")
    ms._set_forest(small)
    assert _first_line(lambda: ms.request_matrix({"instances": x32})) == \
        "Input X contains infinity or a value too large for dtype('float32')."


def test_bare_estimators_are_untouched():
    from sklearn.ensemble import RandomForestRegressor
    X = pc.rows(100, 1)
    f = forest_from_sklearn(RandomForestRegressor(n_estimators=2, max_depth=2, random_state=0)
                            .fit(X, X[:, 0]))
    assert f.pre_ops is None and f.pre_consts is None and f.n_pre_steps == 0
    assert f.input_dtype == TI_F32 and "pipeline" not in f.meta
