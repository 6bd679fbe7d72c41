"""Dense frame-to-model alignment on the CPU: the rule (thor_slam_amd/dense_align.py) against its
independent restatement (tests/ref_tsdf_align.py) on the corner scene of tests/tsdf_align_cases.py,
what it recovers, and every status.

Measured on the corner scene (67 x 45 camera, 1,667 .. 2,035 inliers of 3,015 pixels), true pose
against the three initial poses 14.2 .. 15.1 mm and 0.98 .. 1.00 degrees off: after alignment
0.08 / 0.17 / 1.86 mm and 0.004 / 0.009 / 0.077 degrees, rms residual 11.3 / 13.9 / 18.5 mm before and
0.73 / 0.82 / 1.29 mm after, four iterations each; the worst frame's translation error shrinks 7.6
times and its rotation error 13 times, so the test asks for 4 times.  Smallest pivot ratio of the
corner scene 0.031, largest of the fronto-parallel plane 0 (its first pivot, sum n_x^2, is exactly
zero): ``min_pivot = 1e-6`` is four decades below the one and above the other."""

from __future__ import annotations

import numpy as np

import ref_tsdf_align as REF
import tsdf_align_cases as C
from thor_slam_amd import dense_align as DA

USED = [0, 1, 2, 4]


def _spec(vol, depth, poses, **kw):
    return DA.align(vol[0], vol[1], C.ORIGIN, C.S, C.CAM, depth, poses, max_dist=C.MAX_D, **{**C.PRM, **kw})


def test_defaults_agree():
    assert DA.DEFAULTS == REF.PRM
    assert C.PRM["max_distance"] == 2 * C.S


def test_rule_and_reference_agree():
    ref = C.corner_reference()
    got = _spec(C.corner(), np.stack([C.corner_depth()] * 5), C.FIVE)
    np.testing.assert_array_equal(got["stats"], ref["stats"])
    np.testing.assert_array_equal(got["normal_eq"], ref["normal_eq"])
    np.testing.assert_array_equal(got["residuals"], ref["residuals"])
    np.testing.assert_array_equal(got["world_T_cam"][USED], ref["world_T_cam"][USED])
    assert [[h[0] for h in f] for f in got["history"]] == ref["counts"]
    # the trees: the bottom-up pairs of the rule against the top-down halves of the restatement
    rng = np.random.default_rng(5)
    terms = rng.standard_normal((45, 67, 29)) * 10.0 ** rng.integers(-8, 8, size=(45, 67, 1))
    np.testing.assert_array_equal(DA.reduce_view(terms), REF.view_sums(terms.reshape(-1, 29), 67, 45))
    assert not np.array_equal(DA.reduce_view(terms), terms.reshape(-1, 29).sum(axis=0))   # the order matters


def test_perturbation_recovered():
    ref = C.corner_reference()
    assert (C.corner_depth() > 0).mean() >= 0.5
    for f in (0, 1, 4):
        assert ref["stats"][f, 0] == REF.OK and ref["stats"][f, 3] >= 1000
        t0, r0 = C.pose_error(C.FIVE[f])
        t1, r1 = C.pose_error(ref["world_T_cam"][f])
        print(f"frame {f}: {1e3 * t0:.2f} mm {np.rad2deg(r0):.3f} deg -> {1e3 * t1:.3f} mm {np.rad2deg(r1):.4f} deg; rms "
              f"{1e3 * ref['residuals'][f, 0]:.2f} -> {1e3 * ref['residuals'][f, 1]:.3f} mm; {ref['stats'][f, 1]} iterations")
        assert 0.012 < t0 < 0.018 and 0.8 < np.rad2deg(r0) < 1.2          # about 1.5 cm and 1 degree
        assert t1 < t0 / 4.0 and r1 < r0 / 4.0
        assert ref["residuals"][f, 1] < ref["residuals"][f, 0] / 4.0
    # the true pose stays where it is, to the depth image's millimetre
    t1, r1 = C.pose_error(ref["world_T_cam"][2])
    assert ref["stats"][2, 0] == REF.OK and t1 < 1e-3 and r1 < 1e-3


def test_degenerate_plane_and_the_pivot_margin():
    vol = C.plane()
    depth = C.render(vol, np.eye(4))["depth_mm"]
    assert (depth > 0).mean() >= 0.25
    T0 = C.moved(np.eye(4), (0.005, 0.0, 0.01), (0.0, 0.0, 0.0))
    largest = 0.0
    for mod in (DA, REF):
        out = mod.align_frame(vol[0], vol[1], C.ORIGIN, C.S, C.CAM, depth, T0, max_dist=C.MAX_D, **C.PRM)
        assert out["status"] == REF.DEGENERATE and out["iterations"] == 1
        np.testing.assert_array_equal(out["world_T_cam"], T0)
    # every pivot the plane reaches, with the test switched off
    out = REF.align_frame(vol[0], vol[1], C.ORIGIN, C.S, C.CAM, depth, T0, max_dist=C.MAX_D, **{**C.PRM, "min_pivot": 1e-300})
    largest = max(out["pivots"])
    smallest = min(min(p) for p in C.corner_reference()["pivots"] if p)
    print("pivot ratios: corner smallest", smallest, "plane largest", largest)
    assert smallest >= 1e3 * C.PRM["min_pivot"] and largest <= 1e-3 * C.PRM["min_pivot"]


def test_no_model_rejected_unused():
    depth = C.corner_depth()
    e = C.empty()
    for mod in (DA, REF):
        out = mod.align_frame(e[0], e[1], C.ORIGIN, C.S, C.CAM, depth, C.PERTURBED[0], max_dist=C.MAX_D, **C.PRM)
        assert out["status"] == REF.NO_MODEL and out["iterations"] == 1 and tuple(out["inliers"]) == (0, 0)
        np.testing.assert_array_equal(out["world_T_cam"], C.PERTURBED[0])
        t, w = C.corner()
        out = mod.align_frame(t, w, C.ORIGIN, C.S, C.CAM, depth, C.PERTURBED[0], max_dist=C.MAX_D, **{**C.PRM, "max_translation": 0.005})
        assert out["status"] == REF.REJECTED and out["iterations"] >= 2
        np.testing.assert_array_equal(out["world_T_cam"], C.PERTURBED[0])
        out = mod.align_frame(t, w, C.ORIGIN, C.S, C.CAM, depth, C.PERTURBED[0], max_dist=C.MAX_D, **{**C.PRM, "max_rotation": 0.005})
        assert out["status"] == REF.REJECTED
        out = mod.align_frame(t, w, C.ORIGIN, C.S, C.CAM, depth, C.NAN, max_dist=C.MAX_D, **C.PRM)
        assert out["status"] == REF.UNUSED and out["iterations"] == 0
    ref = C.corner_reference()
    assert ref["stats"][3].tolist() == [REF.UNUSED, 0, 0, 0]


def test_no_pixel_on_the_gate():
    """The guard of the device comparison: the inlier counts of every iteration do not change when
    max_distance moves by a part in 1e9, so no pixel's gate test hangs on the last bits."""
    ref = C.corner_reference()
    t, w = C.corner()
    depth = np.stack([C.corner_depth()] * 5)
    for scale in (1.0 - 1e-9, 1.0 + 1e-9):
        out = REF.align(t, w, C.ORIGIN, C.S, C.CAM, depth, C.FIVE, max_dist=C.MAX_D,
                        **{**C.PRM, "max_distance": C.PRM["max_distance"] * scale})
        assert out["counts"] == ref["counts"]


def test_iteration_limit_and_parameters():
    t, w = C.corner()
    out = REF.align_frame(t, w, C.ORIGIN, C.S, C.CAM, C.corner_depth(), C.PERTURBED[1], max_dist=C.MAX_D, **{**C.PRM, "iterations": 2})
    assert out["status"] == REF.OK and out["iterations"] == 2
    import pytest

    for bad in (dict(iterations=0), dict(iterations=65), dict(min_inliers=5), dict(max_distance=0.0), dict(step_scale=1.5),
                dict(max_rotation=4.0), dict(min_pivot=1.0), dict(eps_rotation=-1.0), dict(max_translation=float("inf"))):
        with pytest.raises(ValueError):
            DA.check_align_params(**{**DA.DEFAULTS, **bad})


def test_config_refuses_dense_cameras_and_devices():
    import pytest

    from thor_slam_amd.params import HipSlamConfig

    cfg = HipSlamConfig(rgbd=True, dense_map=True, dense_align=True)
    cfg.validate()
    assert cfg.dense_align_params()["max_distance"] == 2 * cfg.voxel_size and cfg.dense_align_params()["iterations"] == 10
    assert not HipSlamConfig().dense_align
    for kw, err in ((dict(dense_cameras="all"), "dense_cameras"), (dict(devices=(0, 1)), "devices")):
        with pytest.raises(ValueError, match=err):
            HipSlamConfig(rgbd=True, dense_map=True, dense_align=True, **kw).validate()
    with pytest.raises(ValueError, match="dense_map"):
        HipSlamConfig(rgbd=True, dense_align=True).validate()
    with pytest.raises(ValueError, match="iterations"):
        HipSlamConfig(rgbd=True, dense_map=True, dense_align=True, dense_align_iterations=65).validate()
