"""The median and speckle filters of the dense stereo matcher without a GPU: the configuration
rules, the C ABI of the built library, rules 9 and 10 of thor_slam_amd/stereo_depth.py pinned by
hand on the NumPy reference (tests/ref_stereo_filter.py), and what the filters buy against the
renderer's ground truth on the weakly textured, noisy scene — the device is held bit-exact to that
reference (tests/test_gpu_stereo_filter.py)."""

from __future__ import annotations

import functools
import re
import subprocess

import numpy as np
import pytest

import ref_stereo_depth as BOX
import ref_stereo_filter as FLT
import ref_stereo_sgm as SGM
from thor_slam_amd import _lib
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.stereo_depth import check_filter_params
from thor_slam_amd.synthetic import SyntheticStereoSource


# -- configuration -------------------------------------------------------------------------------
def test_config_defaults_off():
    cfg = HipSlamConfig()
    assert (cfg.stereo_depth_median, cfg.stereo_depth_speckle_size, cfg.stereo_depth_speckle_range) == (0, 0, 32)
    cfg.validate()
    HipSlamConfig(stereo_depth=True, stereo_depth_median=5, stereo_depth_speckle_size=50).validate()
    HipSlamConfig(stereo_depth=True, stereo_depth_median=7).validate()
    HipSlamConfig(stereo_depth=True, stereo_depth_speckle_size=65535, stereo_depth_speckle_range=8191).validate()
    HipSlamConfig(stereo_depth=True, stereo_depth_sgm=True, stereo_depth_median=3, stereo_depth_speckle_range=0).validate()


@pytest.mark.parametrize("kw", [dict(stereo_depth_median=5), dict(stereo_depth_speckle_size=50),
                                dict(stereo_depth=True, stereo_depth_median=4), dict(stereo_depth=True, stereo_depth_median=9),
                                dict(stereo_depth=True, stereo_depth_median=-3),
                                dict(stereo_depth=True, stereo_depth_speckle_size=-1),
                                dict(stereo_depth=True, stereo_depth_speckle_size=65536),
                                dict(stereo_depth=True, stereo_depth_speckle_size=50, stereo_depth_speckle_range=8192),
                                dict(stereo_depth_speckle_range=-1), dict(stereo_depth_median=1)])
def test_config_rejects(kw):
    with pytest.raises(ValueError):
        HipSlamConfig(**kw).validate()


def test_check_filter_params():
    check_filter_params(5, 50)
    check_filter_params(0, 0, 0)
    check_filter_params(7, 65535, 8191)
    for bad in [(1, 0), (4, 0), (9, 0), (-3, 0), (3, -1), (3, 65536), (3, 5, -1), (3, 5, 8192)]:
        with pytest.raises(ValueError):
            check_filter_params(*bad)


# -- C ABI ---------------------------------------------------------------------------------------
def test_library_exports_filter():
    lib = _lib.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (tslam_[a-z_]+)", out))
    assert {"tslam_stereo_depth_filter", "tslam_stereo_depth_filter_apply"} <= exported
    assert lib.tslam_stereo_depth_filter(None, None) == -1
    assert lib.tslam_stereo_depth_filter_apply(None, None, 64, 64, 1.0, 1, None) == -1
    assert hasattr(_lib.Handle, "stereo_depth_filter") and hasattr(_lib.Handle, "stereo_depth_filter_apply")


# -- rule 9 by hand ------------------------------------------------------------------------------
def _centre(rows, m=3):
    a = np.array(rows, np.uint16)
    return int(FLT.median(a, m)[a.shape[0] // 2, a.shape[1] // 2])


def test_median_even_count_takes_the_lower_middle():
    # non-zero values 10 20 30 40 (n = 4): index floor(3 / 2) = 1
    assert _centre([[0, 40, 0], [10, 20, 0], [0, 30, 0]]) == 20
    # n = 2: index 0, the smaller one, although the centre holds the larger
    assert _centre([[0, 0, 0], [0, 90, 0], [0, 0, 50]]) == 50


def test_median_zeros_do_not_take_part():
    # with the five zeros as values the median of nine would be 0; of the four valid ones it is 200
    assert _centre([[0, 0, 0], [100, 300, 0], [200, 0, 400]]) == 200
    # a lone valid pixel keeps its value (n = 1)
    assert _centre([[0, 0, 0], [0, 77, 0], [0, 0, 0]]) == 77
    # odd n = 5: 1 2 3 8 9 -> 3
    assert _centre([[9, 0, 1], [0, 8, 0], [2, 0, 3]]) == 3


def test_median_invalid_centre_stays_invalid():
    assert _centre([[5, 5, 5], [5, 0, 5], [5, 5, 5]]) == 0
    a = np.zeros((6, 7), np.uint16)
    a[2, 3] = 64
    out = FLT.median(a, 5)
    assert out[2, 3] == 64 and np.count_nonzero(out) == 1


def test_median_corner_counts_clamped_duplicates():
    # the 3x3 window of pixel (0, 0) reads rows (0, 0, 1) and columns (0, 0, 1): the corner value
    # four times, its right and lower neighbours twice each, the diagonal once
    a = np.array([[50, 10, 7], [20, 30, 7], [7, 7, 7]], np.uint16)
    # 10 10 20 20 30 50 50 50 50 (n = 9) -> index 4 = 30; each position once (10 20 30 50) would give 20
    assert int(FLT.median(a, 3)[0, 0]) == 30
    # a zero neighbour's duplicates drop out together: 20 20 30 50 50 50 50 (n = 7) -> index 3 = 50
    a[0, 1] = 0
    assert int(FLT.median(a, 3)[0, 0]) == 50
    # m = 5 at the corner of a 2 x 2 image: (0,0) 9 times, (0,1) and (1,0) 6 times, (1,1) 4 times
    b = np.array([[40, 10], [20, 30]], np.uint16)
    # 10 x6, 20 x6, 30 x4, 40 x9 (n = 25) -> index 12 = 30
    assert int(FLT.median(b, 5)[0, 0]) == 30


def test_median_reads_the_unfiltered_input():
    # one row (the clamped rows triple every value, which moves no median): windows 10 10 60,
    # 10 60 20, 60 20 70, 20 70 30, 70 30 30.  In place, left to right, the third window would
    # read the second's result and give 20 20 70 -> 20
    a = np.array([[10, 60, 20, 70, 30]], np.uint16)
    np.testing.assert_array_equal(FLT.median(a, 3), [[10, 20, 60, 30, 30]])


# -- rule 10 by hand -----------------------------------------------------------------------------
def test_speckle_range_links_at_r_not_at_r_plus_one():
    r = 32
    a = np.array([[100, 100 + r, 0, 100, 100 + r + 1]], np.uint16)
    label, sizes = FLT.components(a, r)
    assert sizes == [2, 1, 1]
    assert label[0, 0] == label[0, 1] and label[0, 3] != label[0, 4] and label[0, 2] == -1
    np.testing.assert_array_equal(FLT.speckle(a, 1, r), [[100, 100 + r, 0, 0, 0]])


def test_speckle_ramp_is_one_component():
    r = 32
    a = (100 + r * np.arange(20, dtype=np.uint16))[None]       # the ends differ by 19 r
    assert FLT.components(a, r)[1] == [20]
    np.testing.assert_array_equal(FLT.speckle(a, 19, r), a)
    assert not FLT.speckle(a, 20, r).any()
    assert FLT.components(a, r - 1)[1] == [1] * 20


def test_speckle_diagonal_does_not_link():
    a = np.array([[64, 0, 0], [0, 64, 0], [0, 0, 64]], np.uint16)
    assert FLT.components(a, 8191)[1] == [1, 1, 1]
    assert not FLT.speckle(a, 1, 8191).any()
    # a zero pixel never links, whatever the range
    b = np.array([[5, 0, 5]], np.uint16)
    assert FLT.components(b, 8191)[1] == [1, 1]


def test_speckle_size_s_goes_and_s_plus_one_stays():
    s = 6
    a = np.zeros((8, 12), np.uint16)
    a[1:3, 1:4] = 640          # 2 x 3 = s pixels
    a[4:7, 6:8] = 640          # 3 x 2 = s pixels, upright
    a[1:2, 6:13] = 320         # 1 x 6 ... up to the border: columns 6..11 = 6 = s pixels
    a[5:6, 0:4] = 320
    a[6:7, 0:3] = 320          # an L of 4 + 3 = s + 1 pixels
    out = FLT.speckle(a, s, 32)
    want = np.zeros_like(a)
    want[5:6, 0:4] = 320
    want[6:7, 0:3] = 320
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(FLT.speckle(a, 0, 32), a)     # size 0 is off
    np.testing.assert_array_equal(FLT.speckle(a, s - 1, 32), a)


def test_filter_order_is_median_then_speckle():
    # the median pulls the outlier to its neighbours' value, so the speckle filter sees one
    # component of 9, which size 8 keeps; speckle first would have seen a ring of 8 and an island
    # of 1 and removed both
    a = np.full((3, 3), 320, np.uint16)
    a[1, 1] = 2000
    np.testing.assert_array_equal(FLT.filter_disp32(a, 3, 8, 32), np.full((3, 3), 320))
    assert not FLT.filter_disp32(a, 3, 9, 32).any()
    assert not FLT.median(FLT.speckle(a, 8, 32), 3).any()
    depth, disp = FLT.filtered(a, 100.0, 3, 0)
    np.testing.assert_array_equal(disp, np.full((3, 3), 320))
    np.testing.assert_array_equal(depth, BOX.depth_from_disp32(disp, 100.0))


# -- what the filters buy against the renderer's ground truth ----------------------------------------
def _degrade(img, seed):
    noise = np.random.default_rng(seed).integers(-3, 4, img.shape)
    return np.clip(128 + (img.astype(np.int64) - 128) // 8 + noise, 0, 255).astype(np.uint8)


def _measure(matcher, baseline, n_disp, frame, degraded=False):
    """test_stereo_sgm_cpu._measure's construction: (valid share, share of valid pixels more than
    1 px off, number of such pixels)."""
    src = SyntheticStereoSource(width=320, height=240, baseline=baseline)
    L, R = src.render_image(frame, 0), src.render_image(frame, 1)
    if degraded:
        L, R = _degrade(L, 1), _degrade(R, 2)
    intr = src.get_intrinsics()[0]
    _, z = src.scene.render(src.camera_pose(frame, 0), intr, None, return_depth=True)
    fxb = intr.matrix[0, 0] * src.baseline
    depth, disp32 = matcher(L, R, n_disp, fxb)
    gt = fxb / z
    v = depth > 0
    err = np.abs(disp32[v] / 32.0 - gt[v])
    return float(v.mean()), float((err > 1.0).mean()), int((err > 1.0).sum())


def _sgm(L, R, n_disp, fxb):
    return SGM.stereo_depth_sgm(L, R, n_disp, fxb, p1=100, p2=1200)


MATCHERS = {"box": BOX.stereo_depth, "sgm": _sgm}


@functools.lru_cache(maxsize=None)
def _degraded(name):
    matcher = MATCHERS[name]

    def with_filters(L, R, n_disp, fxb):
        return FLT.filtered(matcher(L, R, n_disp, fxb)[1], fxb, 5, 50, 32)

    return _measure(matcher, 0.3, 64, 0, degraded=True), _measure(with_filters, 0.3, 64, 0, degraded=True)


@pytest.mark.parametrize("name", ["box", "sgm"])
def test_filters_cut_outliers_on_the_degraded_scene(name):
    """Median 5, then speckle (50, 32): at most a quarter of the unfiltered outlier share, for at
    most 0.01 of the frame."""
    raw, flt = _degraded(name)
    print(f"degraded {name}: unfiltered valid {raw[0]:.4f}  >1px {raw[1]:.5f} ({raw[2]} px)")
    print(f"degraded {name}: filtered   valid {flt[0]:.4f}  >1px {flt[1]:.5f} ({flt[2]} px)")
    assert raw[2] > 100                       # there is something to remove
    assert flt[1] <= raw[1] / 4
    assert raw[0] - flt[0] <= 0.01
