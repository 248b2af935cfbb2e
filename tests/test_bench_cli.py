"""bench.py's command line and its --dump-outputs writer (CPU), and one small plain run with a dump (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default_and_steps_are_validated():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--dry-run", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def _npy_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_of_the_headline_size_is_whole_and_within_budget(tmp_path):
    n = 7762696                                 # UNet(1, 8, init_features=32) parameters
    rng = np.random.default_rng(1)
    arrays = {"loss": np.array([2.1, 2.1, 0.0], np.float32), "params": rng.standard_normal(n, dtype=np.float32),
              "grads": rng.standard_normal(n, dtype=np.float32), "buffers": np.ones(5888, np.float32)}
    bench.write_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["buffers.npy", "grads.npy", "loss.npy", "params.npy"]
    for k, v in arrays.items():
        np.testing.assert_array_equal(np.load(tmp_path / f"{k}.npy"), v)
    assert _npy_bytes(tmp_path) <= bench.DUMP_BUDGET_BYTES


def test_an_oversized_dump_is_the_same_seeded_sample_every_time(tmp_path):
    arrays = {"big": np.arange(10_000_000, dtype=np.float64), "small": np.ones(3, np.float32)}
    bench.write_outputs(str(tmp_path / "a"), arrays)
    bench.write_outputs(str(tmp_path / "b"), arrays)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.size < arrays["big"].size and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0)               # sorted distinct elements of the original
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])
    assert _npy_bytes(tmp_path / "a") <= bench.DUMP_BUDGET_BYTES


def _small_plain_run(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", "2", "--height", "64", "--width", "128", "--dump-outputs", str(out_dir)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_line_and_dumps_the_last_step(tmp_path):
    out = _small_plain_run(tmp_path / "a", 3)
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "bf16"
    assert out["full"] is False and out["roofline"] is None and out["cpu_baseline"] is None
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.shape == (3,) and np.isclose(loss[0], out["loss"])
    p, g = np.load(tmp_path / "a" / "params.npy"), np.load(tmp_path / "a" / "grads.npy")
    assert p.dtype == np.float32 and p.shape == g.shape and np.isfinite(p).all() and np.isfinite(g).all()
    assert np.abs(g).max() > 0
    # the last timed step starts from the seeded state: another run, with another step count, reads the same inputs and
    # differs only by the rounding of the weight gradients' fp32 atomic sums
    _small_plain_run(tmp_path / "b", 2)
    for name, tol in (("loss", 1e-6), ("params", 1e-6), ("buffers", 1e-6), ("grads", 1e-5)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.shape == b.shape
        assert np.abs(a.astype(np.float64) - b).max() <= tol * np.abs(a).max(), name
