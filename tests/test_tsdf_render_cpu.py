"""The ray-casting rule of thor_slam_amd/dense_render.py on the CPU: the spec against its
independent restatement (tests/ref_tsdf_render.py), against exact geometry and against the
integrator it reads the volume of; parameter and configuration validation.  No GPU."""

from __future__ import annotations

import numpy as np
import pytest

import ref_tsdf_render as REF
import tsdf_render_cases as C
from oracle import numpy_tsdf as NT
from thor_slam_amd import dense_render as DR
from thor_slam_amd.params import HipSlamConfig

KEYS = ("depth_m", "depth_mm", "normal", "color", "samples")


def _same(a, b, msg=""):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (k, msg)
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{k} {msg}")


@pytest.mark.parametrize("color", [False, True])
def test_spec_equals_restatement_bit_for_bit(color):
    ref = C.reference(C.DIMS, color)
    frac = C.check_not_empty(ref)
    print("hit fractions", frac.round(3), "mean samples", ref["samples"].reshape(4, -1).mean(axis=1).round(1),
          "max samples", ref["samples"].max())
    tsdf, weight = C.volume()
    kw = dict(C.PRM)
    if color:
        kw["color"], kw["color_weight"] = C.color_layer()
    got = DR.render(tsdf, weight, C.ORIGIN, C.S, C.CAM, np.stack(C.VIEWS), **kw)
    _same(got, ref)
    # the centre pixel's ray is exactly (0, 0, 1): the gd == 0 slabs are exercised
    assert (33.0 - C.CAM[4]) / C.CAM[2] == 0.0 and (22.0 - C.CAM[5]) / C.CAM[3] == 0.0
    if color:
        hit = ref["depth_m"] > 0
        assert ref["color"][hit].any() and (~ref["color"][hit].any(axis=-1)).any()     # col_w > 0 and col_w = 0
    # a back face is never a hit: from inside the sphere every ray ends on the plane behind it
    d = ref["depth_m"][3]
    assert (d > 0).all() and d.min() > 0.22
    # every ray takes at most the diagonal plus one samples
    assert ref["samples"].max() <= np.ceil(np.linalg.norm(C.DIMS)) + 1
    np.testing.assert_array_equal(DR.ray_length_table(*C.CAM), np.sqrt(
        (((np.arange(67) - 33.0) / 60.0) ** 2)[None, :] + (((np.arange(45) - 22.0) / 150.0) ** 2)[:, None] + 1.0))


def test_plane_renders_at_the_exact_ray_plane_depth():
    """Bound 1e-6 m: the f32 storage error of the TSDF (1.2e-8 m at 0.2 m) amplified at most 2x by an
    incidence of 60 degrees or less, with a slack of about forty.  The field of a plane is linear
    where no corner is clamped, and the last step before a crossing is too short to start in a
    clamped cell, so the trilinear value and the secant are exact up to storage."""
    tsdf, weight = C.volume(sphere=False, hole=False)
    W, H, fx, fy, cx, cy = C.CAM
    worst, hits = 0.0, 0
    for T in (C.OUTSIDE, C.IN_SPHERE):
        out = DR.render_view(tsdf, weight, C.ORIGIN, C.S, C.CAM, T, **C.PRM)
        ys, xs = np.mgrid[0:H, 0:W]
        d = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))], axis=-1) @ T[:3, :3].T
        cosi = -(d @ C.PLANE_N) / np.linalg.norm(d, axis=-1)
        exact = ((C.PLANE_P - T[:3, 3]) @ C.PLANE_N) / (d @ C.PLANE_N)
        hit = out["depth_m"] > 0
        assert hit.mean() >= 0.25 and np.degrees(np.arccos(cosi[hit])).max() <= 60.0
        np.testing.assert_array_equal(out["depth_m"], out["t"].astype(np.float32))
        e64 = np.abs(out["t"][hit] - exact[hit])         # t*: the hit depth before the f32 cast
        worst, hits = max(worst, float(e64.max())), hits + int(hit.sum())
        n = out["normal"][hit]
        inner = n.any(axis=-1)                           # zero where a +-1/2 voxel sample leaves the grid
        assert inner.mean() > 0.5 and np.abs(n[inner] - C.PLANE_N.astype(np.float32)).max() < 1e-5
    print("plane: worst |t* - exact|", worst, "over", hits, "hits")
    assert worst <= 1e-6


def test_round_trip_of_one_integrated_depth_frame():
    """Fronto-parallel walls at whole millimetres, integrated by the oracle from one depth frame and
    rendered at that frame's pose: the field is linear along z, so the median |depth - input| over
    the hits (which leaves the depth-discontinuity pixels out) is at most 1e-6 m."""
    W, H, fx, fy, cx, cy = C.CAM
    depth = np.full((H, W), 2300, np.uint16)
    depth[:, W // 2:] = 2651
    depth[30:, :20] = 1900
    tsdf = np.zeros(C.DIMS[::-1], np.float32)
    weight = np.zeros_like(tsdf)
    T = C.pose((0.02, -0.01, 0.0))
    NT.integrate(tsdf, weight, depth, DR.rigid_inverse(T), (fx, fy, cx, cy), C.ORIGIN, C.S, C.TRUNC, 10.0, 100.0)
    out = REF.render_view(tsdf, weight, C.ORIGIN, C.S, C.CAM, T, **C.PRM)
    hit = out["depth_m"] > 0
    err = np.abs(out["depth_m"][hit].astype(np.float64) - depth[hit] * 0.001)
    print("round trip: hits", hit.mean().round(3), "median", np.median(err), "90 %", np.quantile(err, 0.9))
    assert hit.mean() >= 0.25
    assert np.median(err) <= 1e-6
    # the output has the format the integrator reads
    assert np.median(np.abs(out["depth_mm"][hit].astype(np.int64) - depth[hit])) == 0


def test_zero_images():
    tsdf, weight = C.volume()
    zero = lambda o: all(not o[k].any() for k in ("depth_m", "depth_mm", "normal", "color"))
    for mod in (DR, REF):
        assert zero(mod.render_view(tsdf, weight, C.ORIGIN, C.S, C.CAM, C.AWAY, **C.PRM))
        assert zero(mod.render_view(tsdf, weight, C.ORIGIN, C.S, C.CAM, C.NAN, **C.PRM))
        near = dict(C.PRM, max_depth=0.9)                # the volume's near face is at z = 1.0
        out = mod.render_view(tsdf, weight, C.ORIGIN, C.S, C.CAM, C.OUTSIDE, **near)
        assert zero(out) and not out["samples"].any()
        assert not zero(mod.render_view(tsdf, weight, C.ORIGIN, C.S, C.CAM, C.OUTSIDE, **C.PRM))


def test_depth_mm_is_zero_beyond_its_range():
    # a wall 70 m away in a volume of 2 m voxels: depth_m holds it, depth_mm cannot
    s, dims, origin = 2.0, (41, 13, 12), (-41.0, -13.0, 56.0)
    z = origin[2] + s * (np.arange(dims[2]) + 0.5)
    tsdf = np.broadcast_to(np.clip(70.0 - z, -8.0, 8.0)[:, None, None], dims[::-1]).astype(np.float32)
    weight = np.ones_like(tsdf)
    prm = dict(C.PRM, max_depth=100.0)
    for mod in (DR, REF):
        out = mod.render_view(tsdf, weight, origin, s, C.CAM, np.eye(4), **prm)
        hit = out["depth_m"] > 0
        assert hit.mean() >= 0.25 and np.abs(out["depth_m"][hit] - 70.0).max() < 1e-4
        assert not out["depth_mm"].any()
    near = np.broadcast_to(np.clip(64.0 - z, -8.0, 8.0)[:, None, None], dims[::-1]).astype(np.float32)
    out = DR.render_view(near, weight, origin, s, C.CAM, np.eye(4), **prm)
    assert (out["depth_mm"][out["depth_m"] > 0] == 64000).all() and (out["depth_m"] > 0).any()


BAD = [dict(width=0), dict(height=0), dict(width=16385), dict(fx=0.0), dict(fy=-1.0), dict(cx=float("nan")),
       dict(min_weight=-1.0), dict(min_depth=-0.1), dict(max_depth=0.0), dict(min_depth=3.0, max_depth=3.0),
       dict(max_depth=float("inf")), dict(step_scale=0.0), dict(step_scale=1.5), dict(outputs=0), dict(outputs=16),
       dict(max_views=0), dict(max_views=257), dict(width=3.5)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(b) for b in BAD])
def test_parameter_validation(bad):
    good = dict(width=67, height=45, fx=60.0, fy=150.0, cx=33.0, cy=22.0, min_weight=1e-4, min_depth=0.0, max_depth=10.0,
                step_scale=0.5, outputs=15, max_views=4)
    DR.check_render_params(**good)
    with pytest.raises(ValueError):
        DR.check_render_params(**{**good, **bad})


def test_volume_needs_two_voxels_per_axis():
    with pytest.raises(ValueError, match="dims"):
        DR.render_view(np.zeros((4, 1, 4), np.float32), np.zeros((4, 1, 4), np.float32), (0, 0, 0), 0.1, C.CAM, np.eye(4))


def test_config_validation():
    cfg = HipSlamConfig(rgbd=True, dense_map=True)
    cfg.validate()
    assert cfg.dense_view_step_scale == 0.5 and cfg.dense_view_max_distance_m is None
    HipSlamConfig(rgbd=True, dense_map=True, dense_view_step_scale=1.0, dense_view_max_distance_m=4.0).validate()
    for kw in (dict(dense_view_step_scale=0.0), dict(dense_view_step_scale=1.01), dict(dense_view_step_scale=None),
               dict(dense_view_max_distance_m=0.0), dict(dense_view_max_distance_m=float("inf")),
               dict(dense_view_max_distance_m="far")):
        with pytest.raises(ValueError, match="dense_view"):
            HipSlamConfig(rgbd=True, dense_map=True, **kw).validate()


def test_view_in_volume_and_scaled_intrinsics():
    A, B = C.pose((0.3, -0.2, 1.0), 33.0), C.pose((1.0, 0.5, -2.0), -70.0)
    np.testing.assert_allclose(DR.view_in_volume(A, B), np.linalg.inv(A) @ B, atol=1e-14)
    assert DR.scaled_intrinsics((640, 480), (500.0, 500.0, 319.5, 239.5), (640, 480)) == (500.0, 500.0, 319.5, 239.5)
    assert DR.scaled_intrinsics((640, 480), (500.0, 500.0, 319.5, 239.5), (320, 240)) == (250.0, 250.0, 159.5, 119.5)


def test_params_struct_layout_and_null_arguments(tmp_path):
    """The ctypes mirror of tslam_tsdf_render_params against the C compiler's layout, and the four
    calls refusing null arguments without touching a device."""
    import ctypes
    import subprocess
    from pathlib import Path

    from thor_slam_amd import _lib

    header = Path(__file__).resolve().parents[1] / "include" / "tslam.h"
    fields = [f for f, _ in _lib.TsdfRenderParams._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n  printf("%%zu", sizeof(tslam_tsdf_render_params));\n%s  return 0;\n}\n'
                   % (header, "".join('  printf(" %%zu", offsetof(tslam_tsdf_render_params, %s));\n' % f for f in fields)))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    P = _lib.TsdfRenderParams
    assert got == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in fields]
    assert (DR.OUT_DEPTH_M, DR.OUT_DEPTH_MM, DR.OUT_NORMAL, DR.OUT_COLOR) == (1, 2, 4, 8)
    lib = _lib.load_library()
    assert lib.tslam_tsdf_render_init(None, None, 1) == -1 and lib.tslam_last_error()
    assert lib.tslam_tsdf_render(None, 0, None, 1, 0, None) == -1
    assert lib.tslam_tsdf_render_buffers(None, None, None, None, None, None) == -1
    assert lib.tslam_tsdf_render_read(None, 0, None, None, None, None) == -1
    assert lib.tslam_abi_version() == 21
