"""CPU: bench.py's command line - `--dump-outputs DIR` (what the last timed step computed, as .npy, within a
64 MB budget), `--steps` validation, and a plain run leaving every extra measurement to `--full`."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_writes_the_whole_output_within_budget(tmp_path):
    out = torch.randn((4, 8, 5), generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(out, str(tmp_path / "d"))
    got = np.load(tmp_path / "d" / "melspectrogram.npy")
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, out.numpy())
    assert sorted(os.listdir(tmp_path / "d")) == ["melspectrogram.npy"]


def test_dump_outputs_samples_whole_clips_with_a_fixed_seed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 10 * 8 * 5 * 4)      # room for 10 of the 64 clips
    out = torch.randn((64, 8, 5), generator=torch.Generator().manual_seed(1))
    for d in ("a", "b"):
        bench.dump_outputs(out, str(tmp_path / d))
    got = np.load(tmp_path / "a" / "melspectrogram.npy")
    idx = np.load(tmp_path / "a" / "melspectrogram_clips.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64
    assert got.shape == (10, 8, 5) and got.nbytes <= bench.DUMP_BYTES_MAX
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 64
    np.testing.assert_array_equal(got, out.numpy()[idx.astype(np.int64)])
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "melspectrogram.npy"), got)      # same clips every run
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "melspectrogram_clips.npy"), idx)


def test_headline_output_is_dumped_whole():
    B, L, sr, n_fft, hop, n_mels = bench.WORKLOADS["headline"]
    assert B * n_mels * (1 + L // hop) * 4 <= bench.DUMP_BYTES_MAX


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--stub-step", "--dump-outputs", "x"]])
def test_bench_rejects_bad_arguments(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


def test_plain_run_leaves_the_gather_to_full():
    """Two gloo ranks with the no-op step, cfg5 workload: without --full the line has no `gather`, and the
    steps asked for are the steps timed."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--stub-step", "--workload", "cfg5"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert "gather" not in rec and "cpu_baseline" not in rec and "configs" not in rec
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
