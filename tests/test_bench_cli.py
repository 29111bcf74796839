"""bench.py's command line: a plain run prints the headline and nothing that needs runs of its own, --full adds parity,
cpu_baseline, roofline and pipelined, --dump-outputs DIR writes the frame of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_KEYS = {"parity", "cpu_baseline", "roofline", "pipelined"}


def _env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=_env(),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_writes_the_whole_frame_below_the_limit(tmp_path):
    frame = np.random.default_rng(0).random((37, 24, 3))
    bench.dump_outputs(str(tmp_path / "out"), frame)
    assert sorted(os.listdir(tmp_path / "out")) == ["frame.npy"]
    got = np.load(tmp_path / "out" / "frame.npy")
    assert got.dtype == np.float64 and np.array_equal(got, frame)


def test_dump_of_a_large_frame_is_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 24 * 3 * 8 + 8 * 37)   # room for ten rows and the index
    frame = np.random.default_rng(0).random((37, 24, 3))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame)
    assert sorted(os.listdir(tmp_path / "a")) == ["frame_row_index.npy", "frame_rows.npy"]
    idx, rows = np.load(tmp_path / "a" / "frame_row_index.npy"), np.load(tmp_path / "a" / "frame_rows.npy")
    assert idx.dtype == np.float64 and rows.dtype == np.float64 and rows.shape == (10, 24, 3)
    assert np.all(np.diff(idx) > 0) and np.array_equal(rows, frame[idx.astype(int)])
    assert np.array_equal(idx, np.load(tmp_path / "b" / "frame_row_index.npy"))   # the same rows every time


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be at least 1" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_frame(tmp_path, oracle):
    out = _bench("--steps", "2", "--warmup", "1", "--spp", "4", "--dump-outputs", str(tmp_path / "out"))
    assert HEADLINE_KEYS <= set(out) and not (FULL_KEYS & set(out))
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["unit"] == "Msamples/s"
    frame = np.load(tmp_path / "out" / "frame.npy")
    assert frame.dtype == np.float64 and frame.shape == (800, 1200, 3)
    scene_id, world_kind = bench.WORKLOADS["c2"][:2]
    want = oracle.render(scene_id, world_kind, 1200, 800, 4, rows=(400, 408), threads=8)[400:408]
    within = float(np.mean(np.all(np.abs(frame[400:408] - want) <= bench.TOL, axis=-1)))
    assert within >= 0.999, "the dumped frame is not the strict build's frame of the timed scene"


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_side_measurements():
    out = _bench("--full", "--steps", "1", "--warmup", "1", "--spp", "4", "--oracle-budget", "2")
    assert HEADLINE_KEYS <= set(out) and FULL_KEYS <= set(out)
    assert out["parity"]["within_1e-5"] >= 0.999 and out["roofline"]["bound"] == "valu_fp64"
