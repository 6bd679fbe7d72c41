"""The free-space depth mask on the device: ``tslam_tsdf_dynamic_init`` / ``tslam_tsdf_dynamic`` /
``tslam_tsdf_dynamic_buffers`` / ``tslam_tsdf_dynamic_read`` (``k_tsdf_dynamic.hip``) and
``HipSlamConfig(dense_dynamic=True)`` against tests/ref_tsdf_dynamic.py.

``mask``, ``depth`` and ``stats`` are equal to the reference's bit for bit: the same IEEE f64
operations in the same order, integer counts, and a scene is used only after the guard has shown that
none of its pixels sits on a gate (tests/tsdf_dynamic_cases.py).  The analytic scenes run on rectified
handles of the two cameras of the CPU tests (67 x 77 and 131 x 69: one and two full 64-bit words plus
3 bits per row, partial tiles on both edges)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import ref_tsdf_dynamic as REF
import tsdf_dynamic_cases as C
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _analytic_handle(cam=C.CAM):
    """A rectified handle whose pair-0 camera is ``cam`` (no images are ever submitted)."""
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import StereoRectification

    W, H, fx, fy, cx, cy = cam
    rect = StereoRectification(W, H, fx, fy, cx, cy, 0.1, np.eye(3), np.eye(3), None, None, True)
    return Handle([rect], HipSlamConfig(n_features=256, n_levels=1), max_batch=1)


def _upload(depth_mm):
    import torch

    return torch.from_numpy(np.ascontiguousarray(depth_mm).view(np.int16).copy()).cuda()


def _from_device(ptr, shape, typestr):
    """A device buffer of the library as a host array (through torch, on the current stream)."""
    import torch

    class _Buf:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    return torch.as_tensor(_Buf(), device="cuda").cpu().numpy()


def _volume(h, vol=None):
    h.tsdf_init(C.ORIGIN, C.DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
    h.tsdf_write(*(C.volume() if vol is None else vol))


def _same(got, ref, what=""):
    for k in ("mask", "depth", "stats"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{what} {k}")


@functools.lru_cache(maxsize=None)
def _scenes(cam):
    """(frames [3][H][W], poses [3][4][4]) of one call: the sphere, the static frame on a NaN pose,
    the box over the word boundaries and the last column from a perturbed pose; guarded."""
    static = C.static_depth(cam)
    sphere, obj = C.with_sphere(static, cam, *C.SPHERE)
    box, _ = C.with_box(static, cam, C.EDGE_BOX)
    frames = np.stack([sphere, static, box])
    poses = np.stack([C.T_STAR, C.NAN, C.PERTURBED[0]])
    for f in (0, 2):
        assert C.guarded(frames[f], poses[f], cam)
    assert C.guarded(static, C.T_STAR, cam)
    frames.setflags(write=False)
    return frames, poses, obj


# -- bit equality on the analytic scenes ---------------------------------------------------------------
@pytest.mark.parametrize("radii", C.RADII)
@pytest.mark.parametrize("cam", [C.CAM, C.CAM2], ids=["67x77", "131x69"])
def test_bit_equality(cam, radii):
    W, H = cam[:2]
    ro, rd = radii
    frames, poses, obj = _scenes(cam)
    t, w = C.volume()
    ref = REF.dynamic(t, w, C.ORIGIN, C.S, C.TRUNC, cam, frames, poses, max_dist=C.MAX_D, **{**C.PRM, "open_radius": ro,
                                                                                              "dilate_radius": rd})
    h = _analytic_handle(cam)
    try:
        _volume(h)
        dev = _upload(frames)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=3, **{**C.PRM, "open_radius": ro, "dilate_radius": rd})
        h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 3, world_T_cam=poses, stream=_stream())
        ptrs, nbytes = h.tsdf_dynamic_buffers()
        assert nbytes == {"depth": 2 * W * H, "mask": W * H} and all(ptrs.values())
        # before the read synchronises: through the device pointers, on the call's stream
        buf = {"depth": _from_device(ptrs["depth"], (3, H, W), "<u2"), "mask": _from_device(ptrs["mask"], (3, H, W), "|u1"),
               "stats": _from_device(ptrs["stats"], (3, 4), "<i4")}
        for f in range(3):
            got = h.tsdf_dynamic_read(f)
            print(cam[:2], radii, "frame", f, "stats", got["stats"].tolist(), "reference", ref["stats"][f].tolist())
            _same(got, {k: ref[k][f] for k in ("mask", "depth", "stats")}, f"frame {f}")
            _same({k: buf[k][f] for k in buf}, got, f"buffers, frame {f}")
        assert ref["stats"][0, 2] == obj.sum()                                        # the sphere is found,
        assert ref["mask"][0][obj].all() or ro > 1                                    # and covered unless the opening is wider than it
        assert ref["stats"][1].tolist() == [REF.UNUSED, 0, 0, 0] and ref["stats"][2, 2] > 0
        cols = np.where(ref["candidates"][2].any(axis=0))[0]
        assert W - 1 in cols and any(c % 64 == 63 and c + 1 in cols for c in cols)    # a word boundary and the last column
        # the static frame alone, in slot 0: the other slots keep what they held
        h.tsdf_dynamic(dev.data_ptr() + 2 * W * H, 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=_stream())
        got = h.tsdf_dynamic_read(0)
        assert got["stats"].tolist() == [0, int((frames[1] > 0).sum()), 0, 0] and not got["mask"].any()
        np.testing.assert_array_equal(got["depth"], frames[1])
        _same(h.tsdf_dynamic_read(2), {k: ref[k][2] for k in ("mask", "depth", "stats")}, "slot 2 afterwards")
    finally:
        h.close()


def test_shifted_window():
    W, H = C.CAM[:2]
    frames, poses, obj = _scenes(C.CAM)
    h = _analytic_handle()
    try:
        _volume(h)
        h.tsdf_shift((3, -1, 2), stream=_stream())
        shift, origin = h.tsdf_window()
        assert shift.tolist() == [3, -1, 2]
        t2, w2 = h.tsdf_read()
        assert C.guarded(frames[0], vol=(t2, w2), origin=tuple(origin))
        ref = C.reference(frames[0], vol=(t2, w2), origin=tuple(origin))
        stale = C.reference(frames[0], vol=(t2, w2))
        assert ref["stats"][2] == obj.sum() and not np.array_equal(stale["candidates"], ref["candidates"])   # the effective origin matters
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)
        h.tsdf_dynamic(_upload(frames[0]).data_ptr(), 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=_stream())
        _same(h.tsdf_dynamic_read(0), ref, "shifted window")
    finally:
        h.close()


# -- integration: the static scene goes in as before, the object stays out ------------------------------
def _project(T, cam):
    """k_tsdf_integrate's pixel of every voxel centre for world_T_cam T: (iy, ix, seen) [nz][ny][nx]."""
    W, H, fx, fy, cx, cy = cam
    q = np.eye(4)                      # cam_T_world with k_tsdf_poses' expression order
    for r in range(3):
        for k in range(3):
            q[r, k] = T[k, r]
        q[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    p = C.A.centres()
    X, Y, Z = p[..., 0], p[..., 1], p[..., 2]
    pz = ((q[2, 0] * X + q[2, 1] * Y) + q[2, 2] * Z) + q[2, 3]
    px = ((q[0, 0] * X + q[0, 1] * Y) + q[0, 2] * Z) + q[0, 3]
    py = ((q[1, 0] * X + q[1, 1] * Y) + q[1, 2] * Z) + q[1, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        fu, fv = np.floor((fx * px / pz + cx) + 0.5), np.floor((fy * py / pz + cy) + 0.5)
        seen = (pz > 0.0) & (fu >= 0.0) & (fu < W) & (fv >= 0.0) & (fv < H)
    return np.where(seen, fv, 0).astype(np.intp), np.where(seen, fu, 0).astype(np.intp), seen


def test_static_scene_integrates_as_before_and_the_object_stays_out():
    W, H = C.CAM[:2]
    frames, poses, obj = _scenes(C.CAM)
    sphere, static = frames[0], frames[1]
    t0, w0 = C.volume()
    h = _analytic_handle()
    try:
        _volume(h)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)
        s = _stream()
        pose = C.T_STAR[None]

        def integrated(depth, filtered):
            h.tsdf_write(t0, w0)
            dev = _upload(depth)
            ptr = dev.data_ptr()
            if filtered:
                h.tsdf_dynamic(ptr, 2 * W * H, 1, world_T_cam=pose, stream=s)
                ptr = h.tsdf_dynamic_buffers()[0]["depth"]
            h.tsdf_integrate_rect(ptr, 2 * W * H, 1, world_T_cam=pose, stream=s)
            return h.tsdf_read()

        # the static frame: filtered or not, the same volume bit for bit
        raw_t, raw_w = integrated(static, False)
        fil_t, fil_w = integrated(static, True)
        assert (raw_w != w0).sum() > 5000
        np.testing.assert_array_equal(fil_w, raw_w)
        np.testing.assert_array_equal(fil_t.view(np.uint32), raw_t.view(np.uint32))
        # the sphere frame: where a voxel's pixel is masked nothing changed, elsewhere the static frame's volume
        got_t, got_w = integrated(sphere, True)
        mask = h.tsdf_dynamic_read(0)["mask"].astype(bool)
        assert mask[obj].all()
        iy, ix, seen = _project(C.T_STAR, C.CAM)
        under = seen & mask[iy, ix]
        np.testing.assert_array_equal(got_w, np.where(under, w0, raw_w))
        np.testing.assert_array_equal(got_t.view(np.uint32), np.where(under, t0, raw_t).view(np.uint32))
        centre = (C.T_STAR @ np.array([*C.SPHERE[0], 1.0]))[:3]
        ball = np.linalg.norm(C.A.centres() - centre, axis=-1) <= C.SPHERE[1]
        assert ball.sum() >= 20 and np.array_equal(got_w[ball], w0[ball]) and np.array_equal(got_t[ball], t0[ball])
        bad_t, bad_w = integrated(sphere, False)                                   # without the mask the object is written in
        assert (bad_t[ball] != t0[ball]).sum() >= 20
    finally:
        h.close()


# -- the undistortion-table path, device and host poses -------------------------------------------------
RW, RH = 320, 240
HW = RW * RH
ROOM_ORIGIN, ROOM_DIMS = (-2.0, -1.5, 0.5), (80, 60, 80)       # from half a metre ahead to the room's back wall
BOX = (slice(100, 140), slice(120, 180), 1500)                 # rows, columns and depth (mm) of an object in mid-air


@functools.lru_cache(maxsize=2)
def _records(n: int, distorted: bool = True):
    """(the RGB-D camera's rectification, n records u8 [n][1][5 HW]); frames 3.. with the object."""
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    from helpers import DISTORTION

    src = SyntheticRGBDSource(width=RW, height=RH, distortion=DISTORTION if distorted else None)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rec = np.ascontiguousarray(src.render_rgbd_sequence(n)[:, None, :])
    for f in range(3, n):
        d = rec[f, 0, 3 * HW:].view(np.uint16).reshape(RH, RW)
        d[BOX[0], BOX[1]] = BOX[2]
    rec.setflags(write=False)
    return rgbd_undistort(cams[ci]), rec


def test_rgbd_table_path_device_and_host_poses():
    import torch

    from thor_slam_amd._lib import Handle

    n = 4
    rect, rec = _records(n)
    assert not rect.is_identity
    cam = (RW, RH, rect.fx, rect.fy, rect.cx, rect.cy)
    cfg = HipSlamConfig(rgbd=True, n_features=1000, n_levels=3)
    prm = {**C.PRM, "min_free_weight": 1.5}          # between the weights 1 and 2: no voxel sits on the gate
    h = Handle([rect], cfg, max_batch=n)
    fresh = Handle([rect], cfg, max_batch=2)
    try:
        dev = torch.from_numpy(rec.copy()).cuda()
        s = _stream()
        h.submit(dev.data_ptr(), n, s)
        res = h.read_poses(n)
        T, st = res["T_abs"][:, 0], res["stats"][:, 0, 0]
        used = [bool(s_ == 0 or (s_ == 2 and f == 0)) for f, s_ in enumerate(st)]
        assert sum(used) >= 3 and used[3]
        depth_ptr, stride = dev.data_ptr() + 3 * HW, 5 * HW
        h.tsdf_init(ROOM_ORIGIN, ROOM_DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        h.tsdf_integrate(depth_ptr, stride, 3, first_frame=0, stream=s)          # the three frames without the object
        tsdf, weight = h.tsdf_read()
        depth = np.stack([rec[f, 0, 3 * HW:].view(np.uint16).reshape(RH, RW) for f in range(n)])
        tracked = np.stack([T[f] if used[f] else C.NAN for f in range(n)])
        kw = dict(max_dist=C.MAX_D, table=rect.map_left, **prm)
        ref = REF.dynamic(tsdf, weight, ROOM_ORIGIN, C.S, C.TRUNC, cam, depth, tracked, **kw)
        for f in range(n):
            if used[f]:
                assert REF.guarded(tsdf, weight, ROOM_ORIGIN, C.S, C.TRUNC, cam, depth[f], tracked[f], **kw), f
        print("table path: reference stats", ref["stats"].tolist())
        assert ref["stats"][3, 2] >= 1000 and ref["mask"][3][110:130, 130:170].all()       # the object is found
        h.tsdf_dynamic_init(pair=0, rect=False, max_frames=n, **prm)
        # from NULL: the batch's device poses
        h.tsdf_dynamic(depth_ptr, stride, n, first_frame=0, stream=s)
        for f in range(n):
            _same(h.tsdf_dynamic_read(f), {k: ref[k][f] for k in ("mask", "depth", "stats")}, f"device poses, frame {f}")
        with pytest.raises(RuntimeError, match="last batch"):
            h.tsdf_dynamic(depth_ptr, stride, 2, first_frame=3, stream=s)
        # from the same poses on the host
        h.tsdf_dynamic(depth_ptr, stride, n, world_T_cam=tracked, stream=s)
        for f in range(n):
            _same(h.tsdf_dynamic_read(f), {k: ref[k][f] for k in ("mask", "depth", "stats")}, f"host poses, frame {f}")
        # integration equivalence through the table: the filtered static frames by integrate_rect equal
        # the raw ones by integrate, from the same starting volume (the default gate of 5 is above
        # every weight here, so the masks are empty)
        h.tsdf_dynamic_init(pair=0, rect=False, max_frames=n, **C.PRM)
        h.tsdf_dynamic(depth_ptr, stride, 3, first_frame=0, stream=s)
        assert all(h.tsdf_dynamic_read(f)["stats"][2] == 0 for f in range(3))
        h.tsdf_integrate_rect(h.tsdf_dynamic_buffers()[0]["depth"], 2 * HW, 3, first_frame=0, stream=s)
        a_t, a_w = h.tsdf_read()
        h.tsdf_write(tsdf, weight)
        h.tsdf_integrate(depth_ptr, stride, 3, first_frame=0, stream=s)
        b_t, b_w = h.tsdf_read()
        assert (b_w != weight).sum() > 10000
        np.testing.assert_array_equal(a_w, b_w)
        np.testing.assert_array_equal(a_t.view(np.uint32), b_t.view(np.uint32))
        # an untracked frame: a handle that has seen two blank frames tracks nothing in the second
        blank = torch.zeros((2, 1, 5 * HW), dtype=torch.uint8, device="cuda")
        fresh.submit(blank.data_ptr(), 2, s)
        assert fresh.read_poses(2)["stats"][1, 0, 0] != 0
        fresh.tsdf_init(ROOM_ORIGIN, ROOM_DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        fresh.tsdf_write(tsdf, weight)
        fresh.tsdf_dynamic_init(pair=0, rect=False, max_frames=1, **prm)
        fresh.tsdf_dynamic(depth_ptr + 3 * stride, stride, 1, first_frame=1, stream=s)
        got = fresh.tsdf_dynamic_read(0)
        assert got["stats"].tolist() == [REF.UNUSED, 0, 0, 0] and not got["mask"].any()
        np.testing.assert_array_equal(got["depth"], REF.resample(depth[3], cam, rect.map_left))
    finally:
        h.close()
        fresh.close()


# -- refusals and the life cycle ------------------------------------------------------------------------
def test_refusals():
    import ctypes

    import torch

    from thor_slam_amd._lib import TsdfDynamicParams

    W, H = C.CAM[:2]
    frames, poses, obj = _scenes(C.CAM)
    h = _analytic_handle()
    try:
        dev = _upload(np.stack([frames[0]] * 3))
        one = np.eye(4)[None]
        with pytest.raises(RuntimeError, match="tslam error -4.*tsdf_init"):
            h.tsdf_dynamic_init(max_frames=1, **C.PRM)
        _volume(h)
        for call in (lambda: h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 1, world_T_cam=one), lambda: h.tsdf_dynamic_read(0),
                     lambda: h.tsdf_dynamic_buffers()):
            with pytest.raises(RuntimeError, match="tslam error -4.*dynamic_init"):
                call()
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=2, **C.PRM)
        h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=_stream())
        before = h.tsdf_dynamic_read(0)
        assert before["stats"][2] == obj.sum()
        for bad in (dict(min_free_weight=0.0), dict(min_free_weight=-1.0), dict(min_free_weight=float("nan")),
                    dict(min_free_weight=float("inf")), dict(free_fraction=0.0), dict(free_fraction=1.0000001),
                    dict(free_fraction=float("nan")), dict(open_radius=-1), dict(open_radius=5), dict(dilate_radius=-1),
                    dict(dilate_radius=9)):
            with pytest.raises(RuntimeError, match="tslam error -1"):
                h.tsdf_dynamic_init(pair=0, rect=True, max_frames=2, **{**C.PRM, **bad})
        for n in (0, 257):
            with pytest.raises(RuntimeError, match="tslam error -1.*max_frames"):
                h.tsdf_dynamic_init(pair=0, rect=True, max_frames=n, **C.PRM)
        with pytest.raises(RuntimeError, match="tslam error -1"):
            h.tsdf_dynamic_init(pair=1, max_frames=1, **C.PRM)
        prm = TsdfDynamicParams(5.0, 0.75, 1, 2, (ctypes.c_int32 * 4)(0, 0, 1, 0))
        assert h.lib.tslam_tsdf_dynamic_init(h.h, 0, 1, ctypes.addressof(prm), 1) == -1
        assert b"reserved" in h.lib.tslam_last_error()
        with pytest.raises(RuntimeError, match="tslam error -1.*n_frames"):
            h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 3, world_T_cam=np.stack([np.eye(4)] * 3))
        with pytest.raises(RuntimeError, match="tslam error -1.*depth"):
            h.tsdf_dynamic(0, 2 * W * H, 1, world_T_cam=one)
        with pytest.raises(RuntimeError, match="tslam error -1.*stride"):
            h.tsdf_dynamic(dev.data_ptr(), W * H, 2, world_T_cam=np.stack([np.eye(4)] * 2))
        with pytest.raises(RuntimeError, match="tslam error -1.*last batch"):
            h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 1, first_frame=0)      # device poses without a batch
        with pytest.raises(RuntimeError, match="tslam error -1.*frame"):
            h.tsdf_dynamic_read(2)
        img = torch.zeros((1, 2, W * H), dtype=torch.uint8, device="cuda")
        h.begin_batch(img.data_ptr(), 1)                                      # inside a batch (nothing is launched)
        for call in (lambda: h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 1, world_T_cam=one),
                     lambda: h.tsdf_dynamic_init(pair=0, rect=True, max_frames=2, **C.PRM)):
            with pytest.raises(RuntimeError, match="tslam error -4.*inside a batch"):
                call()
        h.end_batch()
        # every refusal left the state as it was, and working
        _same(h.tsdf_dynamic_read(0), before, "after the refusals")
        h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 2, world_T_cam=np.stack([C.T_STAR, C.T_STAR]), stream=_stream())
        _same(h.tsdf_dynamic_read(1), before, "slot 1")
        # NULL arguments are skipped
        assert h.lib.tslam_tsdf_dynamic_buffers(h.h, None, None, None, None) == 0
        assert h.lib.tslam_tsdf_dynamic_read(h.h, 0, None, None, None) == 0
    finally:
        h.close()


def test_life_cycle():
    W, H = C.CAM[:2]
    frames, poses, obj = _scenes(C.CAM)
    h = _analytic_handle()
    try:
        _volume(h)
        dev = _upload(frames[0])

        def run():
            h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=_stream())
            return h.tsdf_dynamic_read(0)

        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)
        first = run()
        assert first["stats"][2] == obj.sum()
        # tslam_reset keeps the state and clears the images (and the volume)
        h.reset()
        cleared = h.tsdf_dynamic_read(0)
        assert not cleared["mask"].any() and not cleared["depth"].any() and not cleared["stats"].any()
        assert run()["stats"].tolist() == [0, first["stats"][1], 0, 0]                    # an empty map: nothing is free
        h.tsdf_write(*C.volume())
        _same(run(), first, "after reset")
        # init twice replaces the state
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=2, **{**C.PRM, "open_radius": 0, "dilate_radius": 0})
        again = run()
        np.testing.assert_array_equal(again["mask"].astype(bool), obj)
        assert not h.tsdf_dynamic_read(1)["depth"].any()                                  # a second, fresh slot
        # NULL params frees it; tslam_tsdf_init frees it too
        h.tsdf_dynamic_init(enable=False)
        with pytest.raises(RuntimeError, match="tslam error -4.*dynamic_init"):
            h.tsdf_dynamic_buffers()
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)
        _volume(h)
        with pytest.raises(RuntimeError, match="tslam error -4.*dynamic_init"):
            run()
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)
        _same(run(), first, "a new state on the new volume")
    finally:
        h.close()


# -- engine end to end ------------------------------------------------------------------------------------
ENGINE = dict(batch_size=3, n_features=1000, n_levels=3, tsdf_origin=ROOM_ORIGIN, tsdf_dims=ROOM_DIMS, voxel_size=C.S,
              dense_map=True, dense_dynamic=True, dense_dynamic_min_weight=1.5, enable_loop_closure=False)


def test_engine_rgbd():
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    n = 6
    _, rec = _records(n, distorted=False)
    src = SyntheticRGBDSource(width=RW, height=RH)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    cfg = HipSlamConfig(rgbd=True, dense_color=False, **ENGINE)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    stamps = [0.1 * f for f in range(n)]
    try:
        assert eng.get_dynamic_mask() is None
        for b in range(2):
            eng.process_batch(torch.from_numpy(rec[3 * b:3 * b + 3].copy()).cuda(), timestamps=stamps[3 * b:3 * b + 3])
        dm = eng.get_dense_map()
        newest = eng.get_dynamic_mask()
        rect = eng.rectifications[0]
    finally:
        eng.shutdown()
    assert sorted(newest) == ["depth", "mask", "stats", "timestamp"] and newest["timestamp"] == stamps[-1]
    print("engine, RGB-D: newest frame", newest["stats"].tolist())
    assert newest["stats"][0] == 0 and newest["stats"][2] >= 1000 and newest["mask"][110:130, 130:170].all()
    assert not newest["depth"][newest["mask"] != 0].any()
    # the same call sequence on a bare handle
    h = Handle([rect], cfg, max_batch=3)
    try:
        s = _stream()
        h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                    cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
        h.tsdf_dynamic_init(pair=0, rect=False, max_frames=3, **cfg.dense_dynamic_params())
        for b in range(2):
            dev = torch.from_numpy(rec[3 * b:3 * b + 3].copy()).cuda()
            h.submit(dev.data_ptr(), 3, s)
            h.tsdf_dynamic(dev.data_ptr() + 3 * HW, 5 * HW, 3, first_frame=3 * b, stream=s)
            h.tsdf_integrate_rect(h.tsdf_dynamic_buffers()[0]["depth"], 2 * HW, 3, first_frame=3 * b, stream=s)
        want = h.tsdf_dynamic_read(2)
        t, w = h.tsdf_read()
    finally:
        h.close()
    _same(newest, want, "newest frame")
    assert (w > 0).sum() > 10000
    np.testing.assert_array_equal(dm["weight"], w)
    np.testing.assert_array_equal(dm["tsdf"].view(np.uint32), t.view(np.uint32))


def test_engine_stereo_depth():
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticStereoSource

    n = 6
    src = SyntheticStereoSource(width=RW, height=RH)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    seq = np.ascontiguousarray(src.render_stereo_sequence(n))
    cfg = HipSlamConfig(stereo_depth=True, max_disparity=48, **ENGINE)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    stamps = [0.1 * f for f in range(n)]
    try:
        for b in range(2):
            eng.process_batch(torch.from_numpy(seq[3 * b:3 * b + 3].copy()).cuda(), timestamps=stamps[3 * b:3 * b + 3])
        dm = eng.get_dense_map()
        newest = eng.get_dynamic_mask()
        depth, stamp = eng.get_depth_image()
    finally:
        eng.shutdown()
    assert newest["timestamp"] == stamps[-1] == stamp and newest["stats"][0] == 0
    print("engine, stereo: newest frame", newest["stats"].tolist())
    np.testing.assert_array_equal(newest["depth"], np.where(newest["mask"] != 0, 0, depth))   # rectified: no resampling
    cams = extract_cameras(rig.calibration, 2)
    (li, ri), = stereo_pairs(cams)
    h = Handle([stereo_rectify(cams[li], cams[ri])], cfg, max_batch=3)
    try:
        s = _stream()
        h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                    cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=3, **cfg.dense_dynamic_params())
        h.stereo_depth_init(max_frames=3, uniqueness=cfg.stereo_depth_uniqueness, lr_tol=cfg.stereo_depth_lr_tol)
        depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
        for b in range(2):
            dev = torch.from_numpy(seq[3 * b:3 * b + 3].copy()).cuda()
            h.submit(dev.data_ptr(), 3, s)
            h.stereo_depth(3 * b, 3, pair=0, stream=s)
            h.tsdf_dynamic(depth_ptr, frame_bytes, 3, first_frame=3 * b, stream=s)
            h.tsdf_integrate_rect(h.tsdf_dynamic_buffers()[0]["depth"], 2 * HW, 3, first_frame=3 * b, stream=s)
        want = h.tsdf_dynamic_read(2)
        t, w = h.tsdf_read()
    finally:
        h.close()
    _same(newest, want, "newest frame")
    assert (w > 0).sum() > 10000
    np.testing.assert_array_equal(dm["weight"], w)
    np.testing.assert_array_equal(dm["tsdf"].view(np.uint32), t.view(np.uint32))


def test_engine_refuses_what_is_not_built():
    base = dict(rgbd=True, dense_map=True, dense_color=False, dense_dynamic=True)
    HipSlamConfig(**base, dense_follow=True).validate()
    for kw, err in ((dict(dense_map=False), "dense_map"), (dict(dense_cameras="all"), "dense_cameras"),
                    (dict(devices=(0, 1)), "devices"), (dict(dense_align=True), "dense_align"),
                    (dict(dense_loop=True, enable_loop_closure=True), "dense_loop"), (dict(dense_color=True), "dense_color")):
        with pytest.raises(ValueError, match=f"dense_dynamic.*{err}"):
            HipSlamConfig(**{**base, **kw}).validate()
    with pytest.raises(ValueError, match="dense_dynamic.*stereo_color"):
        HipSlamConfig(dense_map=True, stereo_depth=True, stereo_color=True, dense_dynamic=True).validate()
