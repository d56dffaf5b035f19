"""Device memory of a forest comes back when the forest is closed: the
layout-3 leak test of tests/test_gpu_bheap.py
(test_fix_image_uploaded_once_and_freed) over every layout's set of device
arrays, the linear-leaf tables, the parts of a chunked forest and the TreeSHAP
group.

Per case: one create / predict (700 rows) / close on device 0, then eight more
cycles; free device memory (torch.cuda.mem_get_info) may drop by less than
4 x the forest's device_bytes.  Eight leaked replicas would be 8 x; the slack
is the allocator's own.  The forests are a few MiB each so that the bound is
far above the allocator's granularity.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from kfserving_amd.engine import DeviceForest
from kfserving_amd.forest import OUT_CONTRIB, OUT_MARGIN
from kfserving_amd.formats import lightgbm_format as lf
from kfserving_amd.formats import xgboost_format as xf
from tests.test_gpu_lgb_linear import _text_of

pytestmark = pytest.mark.gpu

ROWS = 700
CYCLES = 8


@functools.lru_cache(maxsize=None)
def _forest(name):
    if name == "shallow":        # 500 x depth 8: the heap family
        trees, ti = xf.synthetic_complete_trees(500, 8, 28, seed=5)
        return xf.forest_from_raw_trees(trees, ti, 28, 0, 0.5, "binary:logistic")
    if name == "groups17":       # 17 output groups: parts of 16 and 1
        trees, ti = xf.synthetic_complete_trees(17 * 30, 8, 28, seed=6, num_class=17)
        return xf.forest_from_raw_trees(trees, ti, 28, 17, 0.5, "multi:softprob")
    if name == "categorical":    # XGBoost-rule categorical splits, depth 6
        trees, ti = xf.synthetic_complete_trees(1500, 6, 12, seed=7)
        xf.add_categorical_splits(trees, [0, 3, 7], 70, seed=8)
        doc = xf.json_model_doc(trees, ti, 12, 0, 0.5, "binary:logistic", version=(2, 0, 0))
        return xf.parse_xgboost_bytes(json.dumps(doc).encode())
    if name == "small_trees":    # 1,500 leaf-wise trees of 63 leaves: stages of whole trees
        trees = lf.synthetic_leafwise_trees(1500, 63, 28, seed=9)
        return lf.parse_lightgbm_text(_text_of(trees, 28, "binary sigmoid:1"))
    if name == "deep":           # 60 x depth 12 (kHxMinDepth): no tree fits a stage
        trees, ti = xf.synthetic_complete_trees(60, 12, 28, seed=10)
        return xf.forest_from_raw_trees(trees, ti, 28, 0, 0.5, "binary:logistic")
    if name == "linear":         # linear leaves, up to 40 terms a leaf
        trees = lf.synthetic_leafwise_trees(200, 63, 40, seed=11)
        lf.add_linear_leaves(trees, 40, seed=12, max_terms=40, const_tree_every=4)
        return lf.parse_lightgbm_text(_text_of(trees, 40, "binary sigmoid:1"))
    if name == "shap":           # 100 x depth 6, 10 features: paths of <= 6 features
        trees, ti = xf.synthetic_complete_trees(100, 6, 10, seed=13)
        return xf.forest_from_raw_trees(trees, ti, 10, 0, 0.5, "binary:logistic")
    raise KeyError(name)


def _cycle(forest, force, kind, X):
    """create / predict / info / close under TI_FORCE_LAYOUT=force."""
    old = os.environ.get("TI_FORCE_LAYOUT")
    if force:
        os.environ["TI_FORCE_LAYOUT"] = force
    else:
        os.environ.pop("TI_FORCE_LAYOUT", None)
    try:
        dev = DeviceForest(forest, [0])
    finally:
        if old is None:
            os.environ.pop("TI_FORCE_LAYOUT", None)
        else:
            os.environ["TI_FORCE_LAYOUT"] = old
    try:
        dev.predict(X, kind)
        return dev.info()
    finally:
        dev.close()


def _check_cycles(forest, force, kind, expect):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((ROWS, forest.n_features)).astype(np.float32)
    X[rng.random(X.shape) < 0.02] = np.nan
    info = _cycle(forest, force, kind, X)
    for key, want in expect.items():
        assert info[key] == want, (key, info)
    nbytes = info["device_bytes"]
    assert nbytes >= 1 << 20, info
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(CYCLES):
        _cycle(forest, force, kind, X)
    torch.cuda.synchronize()
    dropped = free0 - torch.cuda.mem_get_info(0)[0]
    print(f"{force or 'default'}: device_bytes {nbytes}, free memory dropped by {dropped} "
          f"over {CYCLES} cycles")
    assert dropped < 4 * nbytes, (dropped, info)


# name of the layout -> (forest, TI_FORCE_LAYOUT or None where the default
# chooses it, ti_forest_info.layout)
LAYOUTS = {
    "heap": ("shallow", "heap", 0),
    "bheap": ("shallow", None, 3),
    "explicit": ("small_trees", "explicit", 1),
    "rexplicit": ("small_trees", "rexplicit", 6),
    "lexplicit": ("small_trees", "lexplicit", 7),
    "hexplicit": ("deep", None, 8),
    "texplicit": ("small_trees", None, 9),
    "cheap": ("categorical", None, 10),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layout_arrays_freed(layout):
    name, force, number = LAYOUTS[layout]
    _check_cycles(_forest(name), force, OUT_MARGIN, {"layout": number})


def test_linear_leaf_tables_freed():
    _check_cycles(_forest("linear"), None, OUT_MARGIN, {"linear": 1})


def test_chunked_forest_parts_freed():
    _check_cycles(_forest("groups17"), None, OUT_MARGIN, {"n_groups": 17, "layout": 3})


def test_treeshap_group_freed():
    # contributions allocate the path tables and the coefficient table
    _check_cycles(_forest("shap"), None, OUT_CONTRIB, {"shap_table": 1})
