"""The whole-map mesh's host arithmetic (thor-slam_amd/csrc/tslam_tsdf_store_mesh.h: the window's brick
range, the outside test, the per-voxel source of a 9 x 9 x 9 corner tile, the list's order) under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/c/store_mesh_check.cpp is an executable of its
own (`make build-asan/store_mesh_check`; nothing is preloaded), any report aborts it.  CPU only."""

from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "thor-slam_amd" / "csrc"
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1",
       "PATH": "/usr/bin:/bin"}


def _has_asan() -> bool:
    if shutil.which("g++") is None:
        return False
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", "/dev/null"],
                           input="int main(){return 0;}", capture_output=True, text=True)
    return probe.returncode == 0


@pytest.mark.skipif(not _has_asan(), reason="g++ with libasan / libubsan not available")
def test_sanitized_store_mesh_arithmetic():
    subprocess.run(["make", "-s", "-C", str(CSRC), "build-asan/store_mesh_check"], check=True)
    out = subprocess.run([str(CSRC / "build-asan" / "store_mesh_check")], capture_output=True, text=True, env=ENV)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-3000:]
    assert out.stdout.startswith("store mesh: ") and int(out.stdout.split()[2]) > 100000
