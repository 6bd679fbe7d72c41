"""The free-space depth mask without a GPU: the spec (thor_slam_amd/dense_dynamic.py) against the
tests' own restatement (tests/ref_tsdf_dynamic.py), bit for bit on mask, depth and stats, on the
scenes of tests/tsdf_dynamic_cases.py; the parameter refusals; the struct's layout against the C
header.

Every scene passes the guard first: scaling ``thr`` or ``min_free_weight`` by 1 +- 1e-9 changes no
candidate, so no pixel sits on a gate and none is left out of a comparison."""

from __future__ import annotations

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tsdf_dynamic_cases as C
from thor_slam_amd import dense_dynamic as SPEC

HEADER = Path(__file__).resolve().parents[1] / "include" / "tslam.h"


def both(depth, T=C.T_STAR, cam=C.CAM, vol=None, origin=C.ORIGIN, table=None, **prm):
    """The reference's frame, after the guard and the spec's bit equality."""
    t, w = C.volume() if vol is None else vol
    assert C.REF.guarded(t, w, origin, C.S, C.TRUNC, cam, depth, T, max_dist=C.MAX_D, table=table, **{**C.PRM, **prm})
    ref = C.REF.dynamic_frame(t, w, origin, C.S, C.TRUNC, cam, depth, T, max_dist=C.MAX_D, table=table, **{**C.PRM, **prm})
    got = SPEC.dynamic_frame(t, w, origin, C.S, C.TRUNC, cam, depth, T, max_dist=C.MAX_D, undistort=table, **{**C.PRM, **prm})
    for k in ("mask", "depth", "stats"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(got["candidates"], ref["candidates"].astype(bool))
    return ref


def test_defaults_agree():
    assert SPEC.DEFAULTS == C.REF.PRM and (SPEC.OK, SPEC.UNUSED) == (C.REF.OK, C.REF.UNUSED)


@pytest.mark.parametrize("cam", [C.CAM, C.CAM2])
def test_static_scene_has_an_empty_mask(cam):
    depth = C.static_depth(cam)
    for T in (C.T_STAR,) + tuple(C.PERTURBED):
        r = both(depth, T, cam)
        assert r["stats"][0] == SPEC.OK and r["stats"][2] == 0 and not r["mask"].any()
        np.testing.assert_array_equal(r["depth"], depth)
    if cam == C.CAM:
        assert r["stats"][1] == 2747


@pytest.mark.parametrize("cam", [C.CAM, C.CAM2])
def test_sphere_is_masked_and_nothing_far_from_it(cam):
    frame, obj = C.with_sphere(C.static_depth(cam), cam, *C.SPHERE)
    r = both(frame, cam=cam)
    cand, mask = r["candidates"].astype(bool), r["mask"].astype(bool)
    if cam == C.CAM:
        assert obj.sum() == 68
    assert obj.sum() >= 60 and np.array_equal(cand, obj)                 # every object pixel, and none off it
    assert mask[obj].all() and not (mask & ~C.chebyshev_grow(obj, C.PRM["dilate_radius"])).any()
    assert not r["depth"][mask].any() and np.array_equal(r["depth"][~mask], frame[~mask])
    assert r["stats"].tolist() == [0, int((frame > 0).sum()), int(obj.sum()), int(((frame > 0) & mask).sum())]


def test_object_over_the_word_boundary_and_the_last_column():
    W = C.CAM[0]
    frame, obj = C.with_box(C.static_depth(), C.CAM, C.EDGE_BOX)
    # the placement: in front of the map everywhere, in voxels the map has seen free
    r = both(frame)
    cand = r["candidates"].astype(bool)
    assert np.array_equal(cand, obj)
    cols = np.where(cand.any(axis=0))[0]
    assert {63, 64, W - 1} <= set(cols.tolist())
    assert r["mask"][:, W - 1].any() and r["mask"][:, 63].any() and r["mask"][:, 64].any()


def test_object_in_the_weight_2_slab_is_not_a_candidate():
    frame, obj = C.with_sphere(C.static_depth(), C.CAM, *C.SLAB_SPHERE)
    assert obj.sum() >= 15
    r = both(frame)
    assert r["stats"][2] == 0 and not r["mask"].any()
    seen = both(frame, vol=C.uniform_volume())                           # the weight is what gates it
    assert np.array_equal(seen["candidates"].astype(bool), obj)


@pytest.mark.parametrize("ro", [1, 4])
def test_opening_removes_a_blob_of_side_2r_and_keeps_2r_plus_1(ro):
    y0, x0 = 28, 40                                                     # free space around the sphere's place
    for side, survives in ((2 * ro, False), (2 * ro + 1, True)):
        frame = C.static_depth().copy()
        frame[y0:y0 + side, x0:x0 + side] = 1500
        r = both(frame, open_radius=ro)
        blob = np.zeros(frame.shape, bool)
        blob[y0:y0 + side, x0:x0 + side] = True
        assert np.array_equal(r["candidates"].astype(bool), blob)
        if survives:
            assert np.array_equal(r["mask"].astype(bool), C.chebyshev_grow(blob, C.PRM["dilate_radius"]))
        else:
            assert not r["mask"].any()
            np.testing.assert_array_equal(r["depth"], frame)


@pytest.mark.parametrize("radii", C.RADII)
def test_radii(radii):
    ro, rd = radii
    for frame, obj in (C.with_sphere(C.static_depth(), C.CAM, *C.SPHERE), C.with_box(C.static_depth(), C.CAM, C.EDGE_BOX)):
        r = both(frame, open_radius=ro, dilate_radius=rd)
        if (ro, rd) == (0, 0):
            np.testing.assert_array_equal(r["mask"], r["candidates"])
        assert not (r["mask"].astype(bool) & ~C.chebyshev_grow(obj, rd)).any()


def test_empty_volume_nan_pose_and_points_outside():
    frame, obj = C.with_sphere(C.static_depth(), C.CAM, *C.SPHERE)
    r = both(frame, vol=C.A.empty())
    assert r["stats"].tolist() == [0, int((frame > 0).sum()), 0, 0]
    r = both(frame, T=C.NAN)
    assert r["stats"].tolist() == [SPEC.UNUSED, 0, 0, 0] and not r["mask"].any()
    np.testing.assert_array_equal(r["depth"], frame)
    # a valid pixel whose point lies in front of the volume (z < its origin's) is not a candidate
    near = C.static_depth().copy()
    near[30:36, 40:46] = 600
    r = both(near)
    assert r["stats"][1] == 2747 + int((C.static_depth()[30:36, 40:46] == 0).sum()) and r["stats"][2] == 0
    # nor is anything seen from a pose far outside
    away = C.A.moved(C.T_STAR, (30.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    assert both(frame, T=away)["stats"][2] == 0


def test_table_path_shifts_and_clamps():
    W, H = C.CAM[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    table = np.stack([(xs + 3) * 32 + 5, (ys - 2) * 32 - 7], axis=-1).astype(np.int32)   # 3 right, 2 up, clamped at the edges
    raw = np.zeros((H, W), np.uint16)                                    # the raw image that resamples to the sphere frame
    frame, obj = C.with_sphere(C.static_depth(), C.CAM, *C.SPHERE)
    raw[:, 3:] = np.roll(frame, 3, axis=1)[:, 3:]
    raw[:H - 2] = raw[2:].copy()
    r = both(raw, table=table)
    looked = C.REF.resample(raw, C.CAM, table)
    assert looked[10, 5] == raw[8, 8] and looked[0, W - 1] == raw[0, W - 1] and looked[H - 1, W - 1] == raw[H - 3, W - 1]
    assert r["stats"][2] >= 40 and r["mask"].any()
    np.testing.assert_array_equal(r["depth"][r["mask"] == 0], looked[r["mask"] == 0])


def test_shifted_window():
    shift = (3, -1, 2)
    t, w = C.volume()

    def moved(v):   # what tslam_tsdf_shift leaves: vol'(i, j, k) = vol(i + dx, j + dy, k + dz), zeros entering
        out = np.zeros_like(v)
        nz, ny, nx = v.shape
        src = v[max(shift[2], 0):nz + min(shift[2], 0), max(shift[1], 0):ny + min(shift[1], 0), max(shift[0], 0):nx + min(shift[0], 0)]
        out[max(-shift[2], 0):max(-shift[2], 0) + src.shape[0], max(-shift[1], 0):max(-shift[1], 0) + src.shape[1],
            max(-shift[0], 0):max(-shift[0], 0) + src.shape[2]] = src
        return out

    vol = (moved(t), moved(w))
    origin = tuple(C.ORIGIN[a] + C.S * float(shift[a]) for a in range(3))
    frame, obj = C.with_sphere(C.static_depth(), C.CAM, *C.SPHERE)
    r = both(frame, vol=vol, origin=origin)
    assert np.array_equal(r["candidates"].astype(bool), obj)             # the same map, the same answer
    stale = both(frame, vol=vol)                                         # the effective origin matters
    assert not np.array_equal(stale["candidates"], r["candidates"])


def test_check_dynamic_params_refusals():
    SPEC.check_dynamic_params(**SPEC.DEFAULTS)
    SPEC.check_dynamic_params(1e-3, 1.0, 0, 0, max_frames=256)
    SPEC.check_dynamic_params(5, 0.5, 4, 8)
    for bad in (dict(min_free_weight=0.0), dict(min_free_weight=-1.0), dict(min_free_weight=float("nan")),
                dict(min_free_weight=float("inf")), dict(free_fraction=0.0), dict(free_fraction=1.0 + 1e-9),
                dict(free_fraction=float("nan")), dict(open_radius=-1), dict(open_radius=5), dict(open_radius=1.0),
                dict(dilate_radius=-1), dict(dilate_radius=9), dict(dilate_radius=True), dict(max_frames=0),
                dict(max_frames=257), dict(min_free_weight="5")):
        with pytest.raises(ValueError):
            SPEC.check_dynamic_params(**{**SPEC.DEFAULTS, **bad})


def test_config_options_and_refusals():
    from thor_slam_amd.params import HipSlamConfig

    base = dict(rgbd=True, dense_map=True, dense_color=False, dense_dynamic=True)
    HipSlamConfig(**base).validate()
    HipSlamConfig(**base, dense_follow=True).validate()
    HipSlamConfig(dense_map=True, stereo_depth=True, dense_dynamic=True).validate()   # dense_color is ignored on a stereo rig
    assert HipSlamConfig().dense_dynamic is False
    assert HipSlamConfig(dense_dynamic_min_weight=3.0, dense_dynamic_free_fraction=0.5, dense_dynamic_open_px=2,
                         dense_dynamic_dilate_px=4).dense_dynamic_params() == dict(min_free_weight=3.0, free_fraction=0.5,
                                                                                   open_radius=2, dilate_radius=4)
    for kw, err in ((dict(dense_map=False), "dense_dynamic needs dense_map"), (dict(devices=(0, 1)), "dense_dynamic.*devices"),
                    (dict(dense_cameras="all"), "dense_dynamic.*dense_cameras"), (dict(dense_align=True), "dense_dynamic.*dense_align"),
                    (dict(dense_loop=True, enable_loop_closure=True), "dense_dynamic.*dense_loop"),
                    (dict(dense_color=True), "dense_dynamic.*dense_color"), (dict(dense_dynamic_open_px=5), "open_radius"),
                    (dict(dense_dynamic_dilate_px=9), "dilate_radius"), (dict(dense_dynamic_min_weight=0.0), "min_free_weight"),
                    (dict(dense_dynamic_free_fraction=1.5), "free_fraction")):
        with pytest.raises(ValueError, match=err):
            HipSlamConfig(**{**base, **kw}).validate()
    with pytest.raises(ValueError, match="dense_dynamic.*stereo_color"):
        HipSlamConfig(dense_map=True, stereo_depth=True, stereo_color=True, dense_dynamic=True).validate()


def test_params_struct_layout_matches_c(tmp_path):
    from thor_slam_amd._lib import TsdfDynamicParams as P

    src = tmp_path / "probe.c"
    src.write_text(f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tslam_tsdf_dynamic_params), offsetof(tslam_tsdf_dynamic_params, min_free_weight),
         offsetof(tslam_tsdf_dynamic_params, free_fraction), offsetof(tslam_tsdf_dynamic_params, open_radius),
         offsetof(tslam_tsdf_dynamic_params, dilate_radius), offsetof(tslam_tsdf_dynamic_params, reserved));
  return 0;
}}""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == [ctypes.sizeof(P), P.min_free_weight.offset, P.free_fraction.offset, P.open_radius.offset,
                   P.dilate_radius.offset, P.reserved.offset] == [40, 0, 8, 16, 20, 24]
