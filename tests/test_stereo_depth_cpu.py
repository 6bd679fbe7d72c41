"""Dense stereo depth without a GPU: the configuration rules, the C ABI of the built library, the
quality of the NumPy reference (tests/ref_stereo_depth.py) against the renderer's ground-truth depth
— the device is held bit-exact to that reference (tests/test_gpu_stereo_depth.py), so this bounds
the device too — and the spec's rules pinned on hand-made cost volumes."""

from __future__ import annotations

import functools
import re
import subprocess

import numpy as np
import pytest

import ref_stereo_depth as REF
from thor_slam_amd import _lib
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticStereoSource

NEW_SYMBOLS = ("tslam_stereo_depth_init", "tslam_stereo_depth", "tslam_stereo_depth_images",
               "tslam_stereo_depth_buffers", "tslam_stereo_depth_read", "tslam_tsdf_integrate_rect")


# -- configuration -------------------------------------------------------------------------------
def test_config_stereo_depth_enables_dense_map():
    HipSlamConfig(dense_map=True, stereo_depth=True).validate()
    HipSlamConfig(stereo_depth=True).validate()


def test_config_dense_map_alone_still_needs_depth():
    with pytest.raises(ValueError):
        HipSlamConfig(dense_map=True).validate()


@pytest.mark.parametrize("kw", [dict(stereo_depth=True, rgbd=True), dict(stereo_depth=True, devices=(0, 0)),
                                dict(stereo_depth_interval=0), dict(stereo_depth_uniqueness=100),
                                dict(stereo_depth_uniqueness=-1), dict(stereo_depth_lr_tol=-1)])
def test_config_rejects(kw):
    with pytest.raises(ValueError):
        HipSlamConfig(**kw).validate()


def test_config_defaults_off():
    cfg = HipSlamConfig()
    assert (cfg.stereo_depth, cfg.stereo_depth_uniqueness, cfg.stereo_depth_lr_tol, cfg.stereo_depth_interval) == (False, 10, 1, 1)


# -- C ABI ---------------------------------------------------------------------------------------
def test_library_exports_stereo_depth_abi():
    lib = _lib.load_library()
    assert lib.tslam_abi_version() == 21
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (tslam_[a-z_]+)", out))
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert hasattr(lib, name)


def test_null_handle_fails_cleanly():
    lib = _lib.load_library()
    assert lib.tslam_stereo_depth_init(None, None, 1) == -1
    assert lib.tslam_stereo_depth(None, 0, 0, 1, None) == -1
    assert lib.tslam_stereo_depth_read(None, 0, None, None) == -1


# -- reference quality against the renderer's ground truth ----------------------------------------
@functools.lru_cache(maxsize=4)
def _measure(baseline: float, n_disp: int, frame: int):
    src = SyntheticStereoSource(width=320, height=240, baseline=baseline)
    L, R = src.render_image(frame, 0), src.render_image(frame, 1)
    intr = src.get_intrinsics()[0]
    _, z = src.scene.render(src.camera_pose(frame, 0), intr, None, return_depth=True)
    fxb = intr.matrix[0, 0] * src.baseline
    depth, disp32 = REF.stereo_depth(L, R, n_disp, fxb)
    gt = fxb / z
    v = depth > 0
    err = np.abs(disp32[v] / 32.0 - gt[v])
    rel = np.abs(depth[v] / 1000.0 - z[v]) / z[v]
    return float(v.mean()), float((err > 1.0).mean()), float(np.median(rel))


@pytest.mark.parametrize("frame", [0, 7])
def test_reference_quality_default_baseline(frame):
    valid, outliers, rel = _measure(0.075, 32, frame)
    print(f"frame {frame}: valid {valid:.4f}  >1px {outliers:.5f}  median rel depth {rel:.4f}")
    assert valid >= 0.95
    assert outliers <= 0.005
    assert rel <= 0.03


def test_reference_quality_wide_baseline():
    valid, outliers, rel = _measure(0.3, 64, 0)
    print(f"baseline 0.3: valid {valid:.4f}  >1px {outliers:.5f}  median rel depth {rel:.4f}")
    assert valid >= 0.88
    assert outliers <= 0.005


# -- rule pins on hand-made arrays ----------------------------------------------------------------
def _flat_volume(D, H, W, fill=600):
    return np.full((D, H, W), fill, np.int64)


def test_ties_pick_the_smaller_disparity():
    A = _flat_volume(8, 4, 20)
    A[3] = 100
    A[6] = 100          # same minimum: the left winner is 3; m2 (d = 6, not a neighbour) ties -> not unique
    w = REF.winners(A, uniqueness=10, lr_tol=1)
    assert (w["d1"] == 3).all() and (w["m1"] == 100).all() and (w["m2"] == 100).all()
    assert not w["valid"].any() and not w["disp32"].any()
    w0 = REF.winners(A, uniqueness=0, lr_tol=1)   # u = 0 accepts the tie
    assert (w0["dR"][:, :14] == 3).all()          # right winner: smallest d as well
    assert w0["valid"][:, 3:].all() and not w0["valid"][:, :3].any()   # x - d1 >= 0


def test_subpixel_offset_is_a_true_floor_in_range():
    rng = np.random.default_rng(5)
    lo, hi = 16, -16
    for _ in range(200):
        A = _flat_volume(8, 1, 12, 1200)
        d1 = int(rng.integers(1, 7))
        m1 = int(rng.integers(0, 300))
        c0 = m1 + int(rng.integers(1, 400))      # strictly above: d1 is the smallest minimiser
        c2 = m1 + int(rng.integers(0, 400))
        A[d1], A[d1 - 1], A[d1 + 1] = m1, c0, c2
        w = REF.winners(A, uniqueness=0, lr_tol=8)
        off = int(w["off"][0, 11])
        den = c0 - 2 * m1 + c2
        assert off == int(np.floor((32 * (c0 - c2) + den) / (2 * den)))
        assert -16 <= off <= 16
        lo, hi = min(lo, off), max(hi, off)
    assert lo < 0 < hi
    A = _flat_volume(8, 1, 12, 1200)
    A[4], A[3], A[5] = 10, 11, 500               # numerator negative: floor, not truncation
    assert int(REF.winners(A, 0, 8)["off"][0, 11]) == -16
    A[3], A[5] = 500, 10                          # c2 == m1: the upper end
    assert int(REF.winners(A, 0, 8)["off"][0, 11]) == 16


def test_border_disparities_take_no_offset():
    A = _flat_volume(8, 1, 12, 1200)
    A[7] = 5
    w = REF.winners(A, 0, 8)
    assert int(w["off"][0, 11]) == 0 and int(w["disp32"][0, 11]) == 32 * 7


def test_disp32_zero_exactly_where_depth_zero_unless_out_of_range():
    rng = np.random.default_rng(1)
    L = rng.integers(0, 256, (40, 72), dtype=np.uint8)
    R = np.roll(L, -5, axis=1)
    for fxb in (20.0, 2000.0):      # 2000: mm = 64e6 / disp32 > 65535 below disp32 = 977
        depth, disp32 = REF.stereo_depth(L, R, 16, fxb)
        assert (disp32 > 0).sum() > 500
        mm = np.floor(fxb * 32000.0 / np.maximum(disp32, 1).astype(np.float64) + 0.5)
        np.testing.assert_array_equal(depth == 0, (disp32 == 0) | (mm > 65535))
        np.testing.assert_array_equal(depth[depth > 0], mm[depth > 0].astype(np.uint16))
    assert ((disp32 > 0) & (depth == 0)).any()   # the out-of-range case occurred


def test_cost_left_of_the_image_and_box_border():
    rng = np.random.default_rng(2)
    L = rng.integers(0, 256, (16, 24), dtype=np.uint8)
    R = rng.integers(0, 256, (16, 24), dtype=np.uint8)
    A = REF.volume(L, R, 30)        # D > W
    assert A.max() <= 1200
    assert (A[24:] == 1200).all()                 # no column has x >= d
    assert (A[10, :, :8] == 1200).all()           # window columns 0..9 all have x < d


def test_flat_images_are_invalid_everywhere():
    L = np.full((20, 40), 128, np.uint8)
    depth, disp32 = REF.stereo_depth(L, L, 16, 30.0)
    assert not depth.any() and not disp32.any()   # every cost 0: d1 = 0
