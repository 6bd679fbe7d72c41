"""bench.py's ``--dump-outputs`` and the plain / ``--full`` split: the dump writer on the CPU, and
one tiny plain run of the bench on the GPU (what it prints, what it leaves out, what it dumps)."""

from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402


def test_dump_outputs_dtypes_and_names(tmp_path):
    arrays = {"pose_T_rel": np.arange(32, dtype=np.float64).reshape(2, 1, 4, 4),
              "pose_stats": np.array([[0, 7, -3]], dtype=np.int32),
              "tsdf": np.linspace(0, 1, 5, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "d" / "e"), arrays)
    got = {p.stem: np.load(p) for p in (tmp_path / "d" / "e").glob("*.npy")}
    assert sorted(got) == sorted(arrays)
    assert got["pose_T_rel"].dtype == np.float64 and got["pose_stats"].dtype == np.float64
    assert got["tsdf"].dtype == np.float32
    for k, a in arrays.items():
        assert got[k].shape == a.shape
        np.testing.assert_array_equal(got[k], a)


def test_dump_outputs_caps_with_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = np.random.default_rng(5).normal(size=(64, 64))      # 32 KiB: over its 2 KiB share
    small = np.arange(10, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    np.testing.assert_array_equal(a, b)                        # the same sample every run
    assert a.nbytes <= 2048 and a.size == 256
    assert np.isin(a, big).all()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    total = sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy"))
    assert total <= 4096 + 2 * 128                             # + the .npy headers
    # under the limit together nothing is cut, even an array over its share
    bench.dump_outputs(str(tmp_path / "c"), {"big": big[:5], "small": small})   # 2,560 + 40 bytes
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "big.npy"), big[:5])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "16", "--unique", "8", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u8+f64"
    np.testing.assert_allclose(line["value"], 16 / (line["ms_per_step"] * 1e-3), rtol=1e-9)
    # the legs behind --full did not run
    for k in ("boundary", "cpu_baseline"):
        assert k not in line
    for k in ("latency_b1_ms", "pose_with_outliers", "per_kernel_us_isolated"):
        assert line[k] is None
    assert "isolated" not in line["roofline"]
    got = {p.stem: np.load(p) for p in out_dir.glob("*.npy")}
    assert sorted(got) == ["pose_T_abs", "pose_T_rel", "pose_cov", "pose_stats"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["pose_T_rel"].shape == (16, 1, 4, 4) and got["pose_cov"].shape == (16, 1, 6, 6)
    assert got["pose_stats"].shape == (16, 1, 8)
    assert np.isfinite(got["pose_T_rel"]).all() and np.isfinite(got["pose_T_abs"]).all()
    np.testing.assert_array_equal(got["pose_T_rel"][:, 0, 3], np.tile([0.0, 0.0, 0.0, 1.0], (16, 1)))
    assert float(np.mean(got["pose_stats"][:, 0, 0] == 0)) == line["tracking_ok_fraction_last_batch"]
    # the camera moves between consecutive frames, so a tracked frame's relative pose is not identity
    ok = got["pose_stats"][:, 0, 0] == 0
    assert ok.any()
    assert np.abs(got["pose_T_rel"][ok, 0] - np.eye(4)).max(axis=(1, 2)).min() > 1e-6
