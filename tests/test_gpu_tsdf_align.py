"""Dense frame-to-model alignment on the device: ``tslam_tsdf_align_init`` / ``tslam_tsdf_align`` /
``tslam_tsdf_align_read`` / ``tslam_tsdf_align_buffers`` / ``tslam_tsdf_integrate_aligned``
(``k_tsdf_align.hip``) and ``HipSlamConfig(dense_align=True)`` against tests/ref_tsdf_align.py.

The sums of one iteration are bit-equal to the reference's when both read the same model images:
the same IEEE f64 operations in the same order, and the rule fixes the order of every sum.  Poses
after the iterations are compared within 1e-9 per entry, the project's pose parity bound: the
update's sine, cosine and square root are not pinned against the host's.

The device aligns with the handle's own camera, and a handle takes no image below 64 pixels a side,
so the analytic scenes use ``tsdf_align_cases.DEVICE_CAM`` (67 x 77: the CPU tests' 67 x 45 camera
with 32 more rows, partial tiles on both edges) on a rectified handle of that size."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import ref_tsdf_align as REF
import tsdf_align_cases as C
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-9
RENDER = dict(min_weight=C.PRM["min_weight"], min_depth=0.0, max_depth=C.PRM["max_depth"], step_scale=C.PRM["step_scale"])


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _analytic_handle():
    """A rectified handle whose pair-0 camera is DEVICE_CAM (no images are ever submitted)."""
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import StereoRectification

    W, H, fx, fy, cx, cy = C.DEVICE_CAM
    rect = StereoRectification(W, H, fx, fy, cx, cy, 0.1, np.eye(3), np.eye(3), None, None, True)
    return Handle([rect], HipSlamConfig(n_features=256, n_levels=1), max_batch=1)


def _device_views(h, poses):
    """The handle's own ray caster at the align parameters: one dict of images per pose."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    h.tsdf_render_init(*C.DEVICE_CAM, max_views=len(poses), outputs=7, **RENDER)
    h.tsdf_render(poses, stream=_stream())
    return [h.tsdf_render_read(v) for v in range(len(poses))]


def _upload(depth_mm):
    import torch

    return torch.from_numpy(np.ascontiguousarray(depth_mm).view(np.int16).copy()).cuda()


def _from_device(ptr, shape, typestr):
    """A device buffer of the library as a host array (through torch, on the current stream)."""
    import torch

    class _Buf:
        __cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2}

    return torch.as_tensor(_Buf(), device="cuda").cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _scene(h, vol, view_pose):
    """The volume into the handle; (the frame depth the map renders from view_pose, on the device
    and on the host)."""
    h.tsdf_init(C.ORIGIN, C.DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
    h.tsdf_write(*vol)
    depth = _device_views(h, view_pose[None])[0]["depth_mm"]
    return _upload(depth), depth


# -- (a) the analytic corner scene -------------------------------------------------------------------
def test_corner_scene_sums_and_poses():
    W, H = C.DEVICE_CAM[:2]
    t, w = C.corner()
    h = _analytic_handle()
    try:
        dev, depth = _scene(h, (t, w), C.T_STAR)
        assert (depth > 0).mean() >= 0.5
        frames = dev.repeat(5, 1, 1)
        models = _device_views(h, C.FIVE)
        host = np.stack([depth] * 5)
        kw = dict(max_dist=C.MAX_D, models=models)
        # one iteration: counts and the 28 sums, bit for bit
        ref1 = REF.align(t, w, C.ORIGIN, C.S, C.DEVICE_CAM, host, C.FIVE, **kw, **{**C.PRM, "iterations": 1})
        h.tsdf_align_init(pair=0, rect=True, max_frames=5, **{**C.PRM, "iterations": 1})
        h.tsdf_align(frames.data_ptr(), 2 * W * H, 5, world_T_cam=C.FIVE, stream=_stream())
        got1 = h.tsdf_align_read()
        print("inliers", got1["stats"][:, 2].tolist(), "reference", ref1["stats"][:, 2].tolist())
        assert min(ref1["stats"][f, 2] for f in (0, 1, 2, 4)) >= 1000
        np.testing.assert_array_equal(got1["stats"], ref1["stats"])
        np.testing.assert_array_equal(_bits(got1["normal_eq"]), _bits(ref1["normal_eq"]))
        np.testing.assert_array_equal(_bits(got1["residuals"]), _bits(ref1["residuals"]))
        assert got1["normal_eq"][0].any() and not got1["normal_eq"][3].any()
        # the default iterations: poses, statuses, iteration counts
        ref = REF.align(t, w, C.ORIGIN, C.S, C.DEVICE_CAM, host, C.FIVE, **kw, **C.PRM)
        for scale in (1.0 - 1e-9, 1.0 + 1e-9):   # the guard: no pixel of these frames sits on the gate
            o = REF.align(t, w, C.ORIGIN, C.S, C.DEVICE_CAM, host, C.FIVE, **kw,
                          **{**C.PRM, "max_distance": C.PRM["max_distance"] * scale})
            assert o["counts"] == ref["counts"]
        h.tsdf_align_init(pair=0, rect=True, max_frames=5, **C.PRM)
        h.tsdf_align(frames.data_ptr(), 2 * W * H, 5, world_T_cam=C.FIVE, stream=_stream())
        ptrs = h.tsdf_align_buffers()
        assert ptrs["world_T_cam"] and ptrs["stats"]
        buf_T = _from_device(ptrs["world_T_cam"], (5, 4, 4), "<f8")      # before the read synchronises: stays on the device
        buf_s = _from_device(ptrs["stats"], (5, 4), "<i4")
        got = h.tsdf_align_read()
        np.testing.assert_array_equal(_bits(buf_T), _bits(got["world_T_cam"]))
        np.testing.assert_array_equal(buf_s, got["stats"])
        used = [0, 1, 2, 4]
        err = np.abs(got["world_T_cam"][used] - ref["world_T_cam"][used]).max()
        print("poses: worst |device - reference|", err, "stats", got["stats"].tolist())
        assert err <= POSE_TOL
        np.testing.assert_array_equal(got["stats"][:, :2], ref["stats"][:, :2])
        assert got["stats"][3].tolist() == [REF.UNUSED, 0, 0, 0] and np.isnan(got["world_T_cam"][3, 0, 0])
        assert all(got["stats"][f, 0] == REF.OK for f in used)
        for f in (0, 1, 4):   # and the alignment does what it is for
            t0, r0 = C.pose_error(C.FIVE[f])
            t1, r1 = C.pose_error(got["world_T_cam"][f])
            assert t1 < t0 / 4.0 and r1 < r0 / 4.0, (f, t0, t1, r0, r1)
        # a shorter call leaves the other frames' results alone; tslam_reset keeps the state
        h.reset()
        h.tsdf_write(t, w)
        h.tsdf_align(frames.data_ptr(), 2 * W * H, 1, world_T_cam=C.FIVE[1:2], stream=_stream())
        again = h.tsdf_align_read()
        np.testing.assert_array_equal(_bits(again["world_T_cam"][0]), _bits(got["world_T_cam"][1]))
        assert again["stats"].shape == (1, 4)
    finally:
        h.close()


# -- (c) the other outcomes, refusals, the rolling window ---------------------------------------------
def test_degenerate_no_model_rejected_return_t0():
    W, H = C.DEVICE_CAM[:2]
    h = _analytic_handle()
    try:
        # a single fronto-parallel plane
        vol = C.plane()
        dev, depth = _scene(h, vol, np.eye(4))
        T0 = C.moved(np.eye(4), (0.005, 0.0, 0.01), (0.0, 0.0, 0.0))
        want = REF.align_frame(vol[0], vol[1], C.ORIGIN, C.S, C.DEVICE_CAM, depth, T0, max_dist=C.MAX_D, **C.PRM)
        assert want["status"] == REF.DEGENERATE
        h.tsdf_align_init(pair=0, rect=True, max_frames=2, **C.PRM)
        h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, world_T_cam=T0[None], stream=_stream())
        got = h.tsdf_align_read()
        assert got["stats"][0].tolist() == [REF.DEGENERATE, 1, want["inliers"][0], want["inliers"][1]]
        np.testing.assert_array_equal(_bits(got["world_T_cam"][0]), _bits(T0))
        # an empty volume: the first batch of a session
        h.tsdf_write(*C.empty())
        h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, world_T_cam=T0[None], stream=_stream())
        got = h.tsdf_align_read()
        assert got["stats"][0].tolist() == [REF.NO_MODEL, 1, 0, 0]
        np.testing.assert_array_equal(_bits(got["world_T_cam"][0]), _bits(T0))
        # a correction above max_translation
        t, w = C.corner()
        dev, depth = _scene(h, (t, w), C.T_STAR)      # tsdf_init frees the align state
        with pytest.raises(RuntimeError, match="align_init"):
            h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, world_T_cam=C.PERTURBED[0][None], stream=_stream())
        h.tsdf_align_init(pair=0, rect=True, max_frames=2, **{**C.PRM, "max_translation": 0.005})
        h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, world_T_cam=C.PERTURBED[0][None], stream=_stream())
        got = h.tsdf_align_read()
        assert got["stats"][0, 0] == REF.REJECTED and got["stats"][0, 1] >= 2
        np.testing.assert_array_equal(_bits(got["world_T_cam"][0]), _bits(C.PERTURBED[0]))
    finally:
        h.close()


def test_refusals():
    import torch

    W, H = C.DEVICE_CAM[:2]
    h = _analytic_handle()
    try:
        dev = torch.zeros((2, H, W), dtype=torch.int16, device="cuda")
        with pytest.raises(RuntimeError, match="tslam error -4.*tsdf_init"):
            h.tsdf_align_init(max_frames=1, **C.PRM)
        h.tsdf_init(C.ORIGIN, C.DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        for call in (lambda: h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, world_T_cam=np.eye(4)[None]),
                     lambda: h.tsdf_align_read(1), lambda: h.tsdf_align_buffers(),
                     lambda: h.tsdf_integrate_aligned(dev.data_ptr(), 2 * W * H, 1)):
            with pytest.raises(RuntimeError, match="tslam error -4.*align_init"):
                call()
        for bad in (dict(iterations=0), dict(iterations=65), dict(min_inliers=5), dict(max_distance=0.0), dict(step_scale=0.0),
                    dict(max_rotation=4.0), dict(min_pivot=1.0), dict(eps_translation=-1.0), dict(max_depth=float("inf")),
                    dict(max_translation=float("nan"))):
            with pytest.raises(RuntimeError, match="tslam error -1"):
                h.tsdf_align_init(max_frames=1, **{**C.PRM, **bad})
        for frames in (0, 257):
            with pytest.raises(RuntimeError, match="tslam error -1"):
                h.tsdf_align_init(max_frames=frames, **C.PRM)
        with pytest.raises(RuntimeError, match="tslam error -1"):
            h.tsdf_align_init(pair=1, max_frames=1, **C.PRM)
        with pytest.raises(RuntimeError, match="tslam error -4"):      # still none after the refusals
            h.tsdf_align_buffers()
        h.tsdf_align_init(pair=0, rect=True, max_frames=2, **C.PRM)
        with pytest.raises(RuntimeError, match="tslam error -1.*n_frames"):
            h.tsdf_align(dev.data_ptr(), 2 * W * H, 3, world_T_cam=np.stack([np.eye(4)] * 3))
        with pytest.raises(RuntimeError, match="tslam error -1.*depth"):
            h.tsdf_align(0, 2 * W * H, 1, world_T_cam=np.eye(4)[None])
        with pytest.raises(RuntimeError, match="tslam error -1.*stride"):
            h.tsdf_align(dev.data_ptr(), W * H, 2, world_T_cam=np.stack([np.eye(4)] * 2))
        with pytest.raises(RuntimeError, match="tslam error -1.*last batch"):
            h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, first_frame=0)   # device poses without a batch
        with pytest.raises(RuntimeError, match="tslam error -1.*n_frames"):
            h.tsdf_integrate_aligned(dev.data_ptr(), 2 * W * H, 1)      # no tsdf_align call yet
        with pytest.raises(RuntimeError, match="tslam error -4.*colour"):
            h.tsdf_integrate_aligned(dev.data_ptr(), 2 * W * H, 1, color_dev_ptr=dev.data_ptr())
        img = torch.zeros((1, 2, W * H), dtype=torch.uint8, device="cuda")
        h.begin_batch(img.data_ptr(), 1)                                 # inside a batch (nothing is launched)
        for call in (lambda: h.tsdf_align(dev.data_ptr(), 2 * W * H, 1, world_T_cam=np.eye(4)[None]),
                     lambda: h.tsdf_integrate_aligned(dev.data_ptr(), 2 * W * H, 1),
                     lambda: h.tsdf_align_init(pair=0, rect=True, max_frames=2, **C.PRM)):
            with pytest.raises(RuntimeError, match="tslam error -4.*inside a batch"):
                call()
        h.end_batch()
        before = h.tsdf_read()
        assert not before[1].any()                                       # the refusals changed nothing
        h.tsdf_align_init(enable=False)                                  # NULL params: freed
        with pytest.raises(RuntimeError, match="tslam error -4"):
            h.tsdf_align_buffers()
    finally:
        h.close()


def test_shifted_window():
    W, H = C.DEVICE_CAM[:2]
    t, w = C.corner()
    h = _analytic_handle()
    try:
        dev, depth = _scene(h, (t, w), C.T_STAR)
        h.tsdf_shift((3, -1, 2), stream=_stream())
        shift, origin = h.tsdf_window()
        assert shift.tolist() == [3, -1, 2]
        t2, w2 = h.tsdf_read()
        poses = np.stack(C.PERTURBED[:2])
        ref = REF.align(t2, w2, tuple(origin), C.S, C.DEVICE_CAM, np.stack([depth] * 2), poses, max_dist=C.MAX_D, **C.PRM)
        unshifted = REF.align(t2, w2, C.ORIGIN, C.S, C.DEVICE_CAM, np.stack([depth] * 2), poses[:1], max_dist=C.MAX_D, **C.PRM)
        assert all(ref["stats"][:, 0] == REF.OK) and ref["stats"][:, 3].min() >= 500
        assert not np.array_equal(unshifted["normal_eq"][0], ref["normal_eq"][0])       # the effective origin matters
        h.tsdf_align_init(pair=0, rect=True, max_frames=2, **C.PRM)
        h.tsdf_align(dev.repeat(2, 1, 1).data_ptr(), 2 * W * H, 2, world_T_cam=poses, stream=_stream())
        got = h.tsdf_align_read()
        err = np.abs(got["world_T_cam"] - ref["world_T_cam"]).max()
        print("shifted window: worst |device - reference|", err, got["stats"].tolist(), ref["stats"].tolist())
        assert err <= POSE_TOL
        np.testing.assert_array_equal(got["stats"][:, :2], ref["stats"][:, :2])
    finally:
        h.close()


# -- (b) the undistortion-table path: a volume integrated on the device -------------------------------
RW, RH = 320, 240
HW = RW * RH
SCENE_ORIGIN, SCENE_DIMS = (-2.025, -1.525, 2.025), (81, 61, 49)      # the room's back wall and the box, 2.2 .. 4.3 m ahead


@functools.lru_cache(maxsize=1)
def _records(n: int):
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    from helpers import DISTORTION

    src = SyntheticRGBDSource(width=RW, height=RH, distortion=DISTORTION)   # a raw camera: the lookup goes through the table
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rec = np.ascontiguousarray(src.render_rgbd_sequence(n)[:, None, :])
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
    h = Handle([rect], cfg, max_batch=n)
    fresh = Handle([rect], cfg, max_batch=2)
    try:
        dev = torch.from_numpy(rec.copy()).cuda()
        s = _stream()
        h.submit(dev.data_ptr(), n, s)
        res = h.read_poses(n)
        T, st = res["T_abs"][:, 0], res["stats"][:, 0, 0]
        used = [bool(s_ == 0 or (s_ == 2 and f == 0)) for f, s_ in enumerate(st)]
        assert sum(used) >= 3
        depth_ptr, stride = dev.data_ptr() + 3 * HW, 5 * HW
        h.tsdf_init(SCENE_ORIGIN, SCENE_DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        h.tsdf_integrate(depth_ptr, stride, n, first_frame=0, stream=s)
        tsdf, weight = h.tsdf_read()
        depth = np.stack([rec[f, 0, 3 * HW:].view(np.uint16).reshape(RH, RW) for f in range(n)])
        tracked = np.stack([T[f] if used[f] else C.NAN for f in range(n)])
        kw = dict(max_dist=C.MAX_D, table=rect.map_left, **C.PRM)
        # one iteration on the device's own model images, bit for bit: 300 blocks, so the solve folds
        # a level of the block tree before its 256 threads take over (the analytic camera has 25 blocks)
        h.tsdf_render_init(*cam, max_views=n, outputs=5, **RENDER)
        h.tsdf_render(tracked, stream=s)
        models = [h.tsdf_render_read(v) for v in range(n)]
        ref1 = REF.align(tsdf, weight, SCENE_ORIGIN, C.S, cam, depth, tracked, models=models, **{**kw, "iterations": 1})
        h.tsdf_align_init(pair=0, rect=False, max_frames=n, **{**C.PRM, "iterations": 1})
        h.tsdf_align(depth_ptr, stride, n, first_frame=0, stream=s)
        got1 = h.tsdf_align_read()
        np.testing.assert_array_equal(got1["stats"], ref1["stats"])
        np.testing.assert_array_equal(_bits(got1["normal_eq"]), _bits(ref1["normal_eq"]))
        h.tsdf_align_init(pair=0, rect=False, max_frames=n, **C.PRM)
        # from NULL: the batch's device poses
        ref = REF.align(tsdf, weight, SCENE_ORIGIN, C.S, cam, depth, tracked, **kw)
        h.tsdf_align(depth_ptr, stride, n, first_frame=0, stream=s)
        got = h.tsdf_align_read()
        print("device poses:", got["stats"].tolist(), "reference", ref["stats"].tolist(), "rms", ref["residuals"].tolist())
        np.testing.assert_array_equal(got["stats"][:, :2], ref["stats"][:, :2])
        sel = [f for f in range(n) if used[f]]
        assert np.abs(got["world_T_cam"][sel] - ref["world_T_cam"][sel]).max() <= POSE_TOL
        assert all(ref["stats"][f, 2] >= 10000 for f in sel)
        with pytest.raises(RuntimeError, match="last batch"):
            h.tsdf_align(depth_ptr, stride, 2, first_frame=3, stream=s)
        # from host poses about 1.5 cm and 1 degree off the tracked ones
        moves = [((0.010, -0.008, 0.007), (0.6 * C.DEG, -0.5 * C.DEG, 0.6 * C.DEG)),
                 ((-0.009, 0.009, -0.008), (-0.5 * C.DEG, 0.7 * C.DEG, 0.5 * C.DEG))]
        start = np.stack([C.moved(tracked[f], *moves[f % 2]) for f in range(n)])
        ref = REF.align(tsdf, weight, SCENE_ORIGIN, C.S, cam, depth, start, **kw)
        h.tsdf_align(depth_ptr, stride, n, world_T_cam=start, stream=s)
        got = h.tsdf_align_read()
        print("host poses:", got["stats"].tolist(), "reference", ref["stats"].tolist(), "rms", ref["residuals"].tolist())
        np.testing.assert_array_equal(got["stats"][:, :2], ref["stats"][:, :2])
        assert np.abs(got["world_T_cam"][sel] - ref["world_T_cam"][sel]).max() <= POSE_TOL
        for f in sel:
            assert ref["stats"][f, 0] == REF.OK and ref["residuals"][f, 1] < ref["residuals"][f, 0]
        # integrate_aligned = integrate with the aligned poses passed as host poses, bit for bit
        zero = np.zeros_like(tsdf)
        h.tsdf_write(zero, zero)                      # a fresh volume that keeps the align state
        h.tsdf_integrate_aligned(depth_ptr, stride, n, stream=s)
        a_t, a_w = h.tsdf_read()
        h.tsdf_write(zero, zero)
        aligned = np.stack([got["world_T_cam"][f] if got["stats"][f, 0] != REF.UNUSED else C.NAN for f in range(n)])
        h.tsdf_integrate(depth_ptr, stride, n, world_T_cam=aligned, stream=s)
        b_t, b_w = h.tsdf_read()
        assert (a_w > 0).sum() > 10000
        np.testing.assert_array_equal(a_w, b_w)
        np.testing.assert_array_equal(a_t.view(np.uint32), b_t.view(np.uint32))
        # an untracked frame: a handle that has seen two blank frames tracks nothing in the second
        blank = torch.zeros((2, 1, 5 * HW), dtype=torch.uint8, device="cuda")
        fresh.submit(blank.data_ptr(), 2, s)
        assert fresh.read_poses(2)["stats"][1, 0, 0] != 0
        fresh.tsdf_init(SCENE_ORIGIN, SCENE_DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        fresh.tsdf_write(tsdf, weight)
        fresh.tsdf_align_init(pair=0, rect=False, max_frames=1, **C.PRM)
        fresh.tsdf_align(depth_ptr, stride, 1, first_frame=1, stream=s)
        assert fresh.tsdf_align_read()["stats"][0].tolist() == [REF.UNUSED, 0, 0, 0]
    finally:
        h.close()
        fresh.close()


# -- (d) engine end to end ---------------------------------------------------------------------------
def test_engine_dense_align():
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=RW, height=RH)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    cfg = HipSlamConfig(rgbd=True, dense_map=True, dense_align=True, batch_size=3, n_features=1000, n_levels=3,
                        tsdf_origin=SCENE_ORIGIN, tsdf_dims=SCENE_DIMS, voxel_size=C.S)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    records, reports = [], []
    try:
        assert eng.get_dense_alignment()["stats"].shape == (0, 4)
        for i in range(6):
            fs = rig.get_synchronized_frames()
            bgr = np.array(fs.frame_sets[src.name].frames[0].image)
            dep = np.array(fs.frame_sets[src.name].frames[1].image)
            records.append(np.concatenate([bgr.reshape(-1), dep.astype(np.uint16).view(np.uint8).reshape(-1)]))
            eng.process_frames(fs)
            if i % 3 == 2:
                eng.flush()
                reports.append(eng.get_dense_alignment())
        dm = eng.get_dense_map()
        rect = eng.rectifications[0]
    finally:
        eng.shutdown()
    assert [r["stats"][:, 0].tolist() for r in reports] == [[REF.NO_MODEL] * 3, [REF.OK] * 3], [r["stats"].tolist() for r in reports]
    print("engine: second batch", reports[1]["stats"].tolist(), reports[1]["residuals"].tolist())
    # the same call sequence on a bare handle
    h = Handle([rect], cfg, max_batch=3)
    try:
        s = _stream()
        h.tsdf_color(True)
        h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                    cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
        h.tsdf_align_init(pair=0, rect=False, max_frames=3, **cfg.dense_align_params())
        for b in range(2):
            dev = torch.from_numpy(np.stack(records[3 * b:3 * b + 3])[:, None, :]).cuda()
            h.submit(dev.data_ptr(), 3, s)
            h.tsdf_align(dev.data_ptr() + 3 * HW, 5 * HW, 3, first_frame=3 * b, stream=s)
            h.tsdf_integrate_aligned(dev.data_ptr() + 3 * HW, 5 * HW, 3, color_dev_ptr=dev.data_ptr(), stream=s)
            want = h.tsdf_align_read()
            for k in want:
                np.testing.assert_array_equal(reports[b][k], want[k], err_msg=f"batch {b} {k}")
        t, w = h.tsdf_read()
        assert (w > 0).sum() > 10000
        np.testing.assert_array_equal(dm["weight"], w)
        np.testing.assert_array_equal(dm["tsdf"].view(np.uint32), t.view(np.uint32))
    finally:
        h.close()


def test_engine_refuses_dense_cameras_and_devices():
    for kw, err in ((dict(dense_cameras="all"), "dense_cameras"), (dict(devices=(0, 1)), "devices")):
        with pytest.raises(ValueError, match=err):
            HipSlamConfig(rgbd=True, dense_map=True, dense_align=True, **kw).validate()
    with pytest.raises(ValueError, match="dense_map"):
        HipSlamConfig(rgbd=True, dense_align=True).validate()
