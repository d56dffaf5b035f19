"""bench.py's plain run (no --full) on CPU with the stand-in engines of
tests/bench_stub.py: it times the headline alone whatever the other legs'
options say, --steps sets the timed steps, ms_per_step is in the line, and
--dump-outputs writes the last timed step's predictions, the same on every
run of the same arguments."""
import os

import numpy as np
import pytest

import bench
from tests import bench_stub, canon_eval

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
                 "warmup", "n_gpus"}
FULL_KEYS = {"roofline", "single_stream", "cpu_baseline", "batched_latency", "tree_shard",
             "nan_variant", "host_pipeline", "c5_http", "c3", "c4"}


@pytest.fixture(autouse=True)
def _one_rank(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)


def _run(argv, factory):
    engines = []

    def make(forest):
        engines.append(factory(forest, 0))
        return engines[-1]

    return bench.run(bench.parse_args(argv), device="cpu", backend="gloo", make_engine=make), engines


def test_plain_run_is_the_headline_alone():
    # the other legs' options are given, and ignored without --full
    line, engines = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--rows", "512",
                          "--configs", "c3", "--rows3", "1000", "--latency-qps", "200",
                          "--cpu-seconds", "0.1", "--host-rows", "1000"], bench_stub.make)
    assert len(engines) == 1                              # no other forest was built
    assert engines[0].calls == [(512, 28)] * 9            # warmup 2 + 7 timed steps, no more
    assert HEADLINE_KEYS <= set(line) and not FULL_KEYS & set(line)
    assert line["full"] is False and line["steps"] == 7 and line["warmup"] == 2
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] >= 1.0                     # the stand-in's 1 ms a step
    want = 512 * 7 / (line["ms_per_step"] * 7e-3)
    assert abs(line["value"] - want) < 1e-6 * want


def test_full_is_off_by_default_and_keeps_the_other_legs():
    assert bench.parse_args([]).full is False and bench.parse_args([]).dump_outputs == ""
    line, engines = _run(["--full", "--steps", "2", "--warmup", "1", "--rows", "256",
                          "--configs", "", "--no-cpu-baseline", "--latency-qps", "0"],
                         bench_stub.make)
    assert line["full"] is True and len(engines) == 2     # the headline's and the tree shard's
    assert {"roofline", "single_stream", "tree_shard"} <= set(line)
    assert line["single_stream"]["value"] == line["value"]


def test_dump_outputs_last_step_same_on_every_run(tmp_path):
    rows = 257
    argv = ["--steps", "2", "--warmup", "1", "--rows", str(rows), "--x-buffers", "1"]
    outs = []
    for d in ("a", "b"):
        line, _ = _run(argv + ["--dump-outputs", str(tmp_path / d)], bench_stub.make_canon)
        assert os.listdir(tmp_path / d) == ["predict.npy"] and line["steps"] == 2
        outs.append(np.load(tmp_path / d / "predict.npy"))
    assert outs[0].dtype == np.float32 and outs[0].shape == (rows,)
    assert np.array_equal(outs[0], outs[1])
    # the batch of rank 0 (bench.shard_rows's seed) through the canonical evaluator
    _, _, forest = bench.build_model()
    X = np.random.default_rng(1000).standard_normal((rows, bench.N_FEAT), dtype=np.float32)
    want = np.asarray(canon_eval.predict(forest, X.astype(np.float64)), np.float32).reshape(-1)
    assert np.array_equal(outs[0], want)


def test_dump_outputs_samples_past_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    a = np.arange(5000, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"predict": a, "small": a[:7].astype(np.float16)})
    got = np.load(tmp_path / "a" / "predict.npy")
    assert got.dtype == np.float64 and got.nbytes == 2048          # half the limit each
    assert np.all(np.diff(got) > 0) and np.isin(got, a).all()      # rows of a, in row order
    assert np.array_equal(got, np.load(tmp_path / "b" / "predict.npy"))
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and np.array_equal(small, a[:7])
    bench.dump_outputs(str(tmp_path / "r"), {"predict": a}, rank=1, world=2)
    assert np.load(tmp_path / "r" / "predict_rank1.npy").nbytes == 2048
