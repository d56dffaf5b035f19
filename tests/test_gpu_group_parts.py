"""Forests of more than 16 output groups ("group parts", launch_chunked in
treeinfer.hip) held to their references on repeated calls of one handle, as a
serving worker makes them: a different batch and batch size every call, every
call checked.  Margins, predictions, leaf ids and TreeSHAP contributions of a
part reach the output through a scratch the parts of a call share; before
this module every group-part test called each kind once on a fresh handle.

Cases, batches and references: tests/group_parts_cases.py (the call sequence
is 70, 6, 70, 1, 257, 8, 64, 65 rows, each a different batch);
tests/test_group_parts_cases.py asserts, without a GPU, that a misplaced row
or column block cannot pass for right in them.

Bounds are the project's own (group_parts_cases.bound): margins and leaf ids
bit-exact, labels exact, probabilities rtol 1e-5, contributions and
approximate contributions 1e-6 (float32 forests) or 1e-9 (float64) of the
row's scale, interactions 1e-6 or 1e-14."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kfserving_amd.engine import OPT_SHAP_TABLE_ROWS, DeviceForest
from kfserving_amd.forest import (OUT_CONTRIB, OUT_CONTRIB_APPROX, OUT_INTERACT, OUT_LEAF,
                                  OUT_MARGIN, OUT_PREDICT, TI_F32)
from tests import group_parts_cases as gp
from tests import shap_interact_cases as ic

pytestmark = pytest.mark.gpu

NAMES = {OUT_MARGIN: "margin", OUT_PREDICT: "predict", OUT_LEAF: "leaf", OUT_CONTRIB: "contrib",
         OUT_CONTRIB_APPROX: "approx", OUT_INTERACT: "interact"}
# (kind, TI_OPT_SHAP_TABLE_ROWS or None to leave it)
MODES = {"margin": (OUT_MARGIN, None), "predict": (OUT_PREDICT, None), "leaf": (OUT_LEAF, None),
         "contrib-arith": (OUT_CONTRIB, 0), "contrib-table": (OUT_CONTRIB, 1 << 30)}
XTYPES = pytest.mark.parametrize("xdtype", [np.float32, np.float64], ids=["x32", "x64"])


def _hold(name, kind, got, n, seed, what):
    """`got` against the cached reference of batch (n, seed); the message names
    the call (in `what`), the row range and the parts that are wrong."""
    f = gp.case(name).forest
    w = gp.want(name, kind, n, seed)
    assert got.dtype == f.output_dtype(kind), what
    bad = gp.wrong_elements(f, kind, got, w)
    assert not bad.any(), f"{name} {NAMES[kind]}, {what}, {n} rows: {gp.describe_wrong(f, kind, bad)}"


def _calls(dev, name, kind, calls, xdtype, what=""):
    """One predict a (rows, seed) of `calls` on the handle; the first wrong
    call fails the test."""
    for i, (n, seed) in enumerate(calls):
        got = ic.predict(dev, gp.batch(name, n, seed).astype(xdtype), kind)
        _hold(name, kind, got, n, seed, f"{what}call {i} of {len(calls)}")


@XTYPES
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", gp.CASES)
def test_repeated_calls_one_kind(name, mode, xdtype):
    """Eight calls of one kind on one handle, every one against its reference.
    k33-generic: the 16-group parts' rows are wider than kShapLdsW, so there is
    no coefficient table to build and contrib_kernel serves them."""
    kind, table_rows = MODES[mode]
    dev = DeviceForest(gp.case(name).forest, [0])
    try:
        if table_rows is not None:
            dev.set_option(OPT_SHAP_TABLE_ROWS, table_rows)
        _calls(dev, name, kind, gp.sequence(name), xdtype)
        if name == "k33-generic" and kind == OUT_CONTRIB:
            info = dev.info()
            assert info["shap_table"] != 1 and info["shap_table_bytes"] == 0, info
    finally:
        dev.close()


@pytest.mark.parametrize("batches", ["different", "same"])
@pytest.mark.parametrize("table", ["arith-70-rows", "table-6-rows"])
def test_design_reproducer(table, batches):
    """DESIGN.md's record of the defect, as written: the 17-group forest, 70
    rows x 6 calls with the coefficient table off, 6 rows x 6 calls with it."""
    seq = gp.K17_70 if table == "arith-70-rows" else gp.K17_6
    if batches == "same":
        seq = (seq[0],) * 6
    dev = DeviceForest(gp.case("k17-design").forest, [0])
    try:
        dev.set_option(OPT_SHAP_TABLE_ROWS, 0 if table == "arith-70-rows" else 1 << 30)
        _calls(dev, "k17-design", OUT_CONTRIB, seq, np.float32)
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["k20-sliced", "k17-design"])
def test_kinds_interleaved(name):
    """The kinds in turn on one handle, twice round, over changing batches:
    each kind takes the replica's scratch buffers after another kind gave them back."""
    cycle = [OUT_MARGIN, OUT_CONTRIB, OUT_LEAF, OUT_PREDICT, OUT_CONTRIB_APPROX, OUT_CONTRIB]
    if name == "k17-design":
        cycle.insert(3, OUT_INTERACT)
    seq = gp.sequence(name)
    if name == "k17-design":      # interactions: the small batches (a row is 17 x 36 values)
        seq = tuple(s for s in seq if s[0] <= 70)
    dev = DeviceForest(gp.case(name).forest, [0])
    try:
        for i, kind in enumerate(cycle * 2):
            n, seed = seq[i % len(seq)]
            xdtype = np.float32 if i % 3 else np.float64
            got = ic.predict(dev, gp.batch(name, n, seed).astype(xdtype), kind)
            _hold(name, kind, got, n, seed, f"call {i} of {2 * len(cycle)}")
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["k20-sliced", "k20-softmax"])
def test_transforms_over_assembled_margins(name):
    """Softmax and argmax copy the parts' margins into a second scratch that
    transform_rows_kernel reads; identity margins are copied straight into the
    output.  The two orders of copy against consumer alternate on one handle."""
    seq = gp.sequence(name)
    dev = DeviceForest(gp.case(name).forest, [0])
    try:
        for i, (n, seed) in enumerate(seq + seq[:4]):
            kind = OUT_MARGIN if i % 3 == 2 else OUT_PREDICT
            got = ic.predict(dev, gp.batch(name, n, seed).astype(np.float32), kind)
            _hold(name, kind, got, n, seed, f"call {i}")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", [OUT_MARGIN, OUT_CONTRIB], ids=["margin", "contrib"])
def test_callers_stream_without_host_synchronisation(kind):
    """predict_device on a stream of the caller's: six calls over changing
    batches enqueued back to back, each into its own output, one
    synchronisation at the end."""
    import torch
    name = "k20-sliced"
    f = gp.case(name).forest
    seq = gp.sequence(name)[:6]
    xs = [torch.from_numpy(gp.batch(name, n, seed).astype(np.float32)).cuda() for n, seed in seq]
    outs = [torch.full((n, f.output_width(kind)), float("nan"), dtype=torch.float32, device="cuda")
            for n, _ in seq]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    dev = DeviceForest(f, [0])
    try:
        for x, o in zip(xs, outs):
            dev.predict_device(x.data_ptr(), TI_F32, x.shape[0], x.shape[1], x.shape[1], kind,
                               o.data_ptr(), o.numel(), stream=stream.cuda_stream)
        stream.synchronize()
        for i, ((n, seed), o) in enumerate(zip(seq, outs)):
            _hold(name, kind, o.cpu().numpy(), n, seed, f"enqueued call {i} of 6")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", [OUT_MARGIN, OUT_CONTRIB], ids=["margin", "contrib"])
def test_two_slots(kind):
    """Two slots on one device: a call's rows are cut in two shards, each on
    its slot's stream with its own scratch, at the same time.  (The batches:
    test_group_parts_cases.py::test_k17_two_slot_batches.)"""
    dev = DeviceForest(gp.case("k17-design").forest, [0, 0])
    try:
        _calls(dev, "k17-design", kind, gp.K17_257, np.float32)
    finally:
        dev.close()


@pytest.mark.parametrize("kind", [OUT_MARGIN, OUT_CONTRIB], ids=["margin", "contrib"])
def test_host_pipeline_two_lanes(kind, monkeypatch):
    """TI_CHUNK_MB=1 and float32 rows at a pitch of 512 elements: a chunk is
    1 MiB / 2,048 B = 512 rows, so 1,300 rows are three chunks on the host
    pipeline's two lanes, which run launch_chunked from two streams in one
    call.  Bit-identical to one predict_device launch over the same rows, and
    32 of the rows (both sides of each chunk edge, the first and the last 8)
    are held to the reference."""
    import torch
    name, rows, stride = "k20-sliced", 1300, 512
    f = gp.case(name).forest
    assert f.input_dtype == TI_F32
    chunk = (1 << 20) // (stride * 4)
    assert chunk == 512 and -(-rows // chunk) == 3          # three chunks: lanes 0, 1, 0
    X = np.concatenate([gp.batch(name, 257, 2050 + i) for i in range(6)])[:rows].astype(np.float32)
    sample = np.r_[0:8, 508:516, 1020:1028, rows - 8:rows]
    w = gp.reference(name, kind, X[sample])
    dev = DeviceForest(f, [0])
    try:
        width = f.output_width(kind)
        xt = torch.from_numpy(X).cuda()
        ot = torch.full((rows, width), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dev.predict_device(xt.data_ptr(), TI_F32, rows, X.shape[1], X.shape[1], kind, ot.data_ptr(),
                           ot.numel(), stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        one = ot.cpu().numpy()
        monkeypatch.setenv("TI_CHUNK_MB", "1")
        for call in range(2):
            got = ic.predict(dev, X, kind, stride=stride)
            assert np.array_equal(got, one), f"call {call}: the chunks differ from one launch"
            bad = gp.wrong_elements(f, kind, got[sample], w)
            assert not bad.any(), f"call {call}: {gp.describe_wrong(f, kind, bad)} (of the sampled rows)"
    finally:
        dev.close()


@pytest.mark.parametrize("table", ["arith", "table"])
def test_forced_path_slices(table, monkeypatch):
    """TI_SHAP_SLICES=2 (a developer knob): the first part's 768 paths in two
    slices, so each call also takes and frees the slices' partials beside the
    scratch the parts share."""
    monkeypatch.setenv("TI_SHAP_SLICES", "2")
    dev = DeviceForest(gp.case("k20-sliced").forest, [0])
    try:
        dev.set_option(OPT_SHAP_TABLE_ROWS, 0 if table == "arith" else 1 << 30)
        _calls(dev, "k20-sliced", OUT_CONTRIB, gp.sequence("k20-sliced"), np.float32, "two slices, ")
    finally:
        dev.close()


@pytest.mark.parametrize("kind", [OUT_MARGIN, OUT_PREDICT, OUT_LEAF, OUT_CONTRIB, OUT_CONTRIB_APPROX],
                         ids=["margin", "predict", "leaf", "contrib", "approx"])
@pytest.mark.parametrize("name", ["k20-sliced", "lgb-k18-f64"])
def test_repeat_equals_fresh(name, kind):
    """The fourth call of a used handle returns, bit for bit, what the first
    call of a fresh handle returns on the same batch."""
    f = gp.case(name).forest
    seq = gp.sequence(name)
    n, seed = seq[2]
    B = gp.batch(name, n, seed).astype(np.float32)
    used, fresh = DeviceForest(f, [0]), DeviceForest(f, [0])
    try:
        for pn, pseed in (seq[0], seq[4], seq[1]):
            ic.predict(used, gp.batch(name, pn, pseed).astype(np.float32), kind)
        got = ic.predict(used, B, kind)
        first = ic.predict(fresh, B, kind)
        assert np.array_equal(got, first, equal_nan=True), \
            f"{np.count_nonzero(got != first)} of {got.size} values differ from a fresh handle's"
        _hold(name, kind, first, n, seed, "fresh handle")
    finally:
        used.close()
        fresh.close()


def test_plugin_explain_and_predict_repeated():
    """XGBoostModel on the K = 20 booster: three :explain and three :predict
    requests with different instances, each against its reference at the
    bounds of test_gpu_shap.py::test_plugin_explain."""
    from kfserving_amd.xgbserver import XGBoostModel
    from oracle import shap_ref, xgb_ref
    c = gp.case("k20-sliced")
    f = c.forest
    model = XGBoostModel("m", "", 1, booster=f)
    for i, (n, seed) in enumerate(gp.sequence("k20-sliced")[1:6:2]):      # 6, 1 and 8 rows
        rows = np.nan_to_num(gp.batch("k20-sliced", n, seed), nan=0.5).tolist()
        X = model.request_matrix({"instances": rows})
        got = np.asarray(model.explain({"instances": rows})["explanations"])
        want = shap_ref.contributions(f, X.astype(np.float64)).reshape(n, f.n_groups, f.n_features + 1)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=f"explain request {i}")
        pred = np.asarray(model.predict({"instances": rows})["predictions"])
        np.testing.assert_allclose(pred, xgb_ref.predict(c.model, X), rtol=1e-5,
                                   err_msg=f"predict request {i}")


def test_process_without_torch():
    """This module's process has torch loaded (tests/conftest.py), so the
    library runs on the HIP runtime PyTorch bundles; a serving worker has the
    system's, and wrong values of these forests have shown under the system's
    runtime alone ("Call scratch").  So the repeated calls run
    once more in a fresh process that imports no torch
    (tests/group_parts_child.py lists the scenarios).  The child takes about
    17 s, most of it the Python references of three cases'
    contributions, which it cannot share with this process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.group_parts_child"], cwd=root,
                       capture_output=True, text=True, timeout=240)
    print(r.stdout)
    wrong = [line for line in r.stdout.splitlines() if "WRONG" in line]
    assert r.returncode == 0 and not wrong, "\n".join(wrong) or r.stderr[-2000:]
    assert "HIP runtime:" in r.stdout          # the child ran to its end, torch not imported
