"""The dense map seen from a pose on the device: ``tslam_tsdf_render_init`` / ``tslam_tsdf_render`` /
``tslam_tsdf_render_buffers`` / ``tslam_tsdf_render_read`` (``k_render_poses`` and ``k_tsdf_render``
in ``k_tsdf_render.hip``) and ``HipSlamEngine.get_dense_view`` against tests/ref_tsdf_render.py.

``depth_m``, ``depth_mm``, ``color`` and the hit mask are bit-exact: the same IEEE f64 operations in
the same order, the ray lengths from a host table.  The normals are compared within 1e-6 per
component with an identical zero / non-zero pattern: their normalisation takes an f64 square root on
the device, the one operation of this rule the project has not pinned against the host's."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import ref_tsdf_render as REF
import tsdf_render_cases as C
from thor_slam_amd.dense_render import view_in_volume
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

W, H = 320, 240
HW = W * H
MAX_D, MAX_W = 10.0, 100.0


@functools.lru_cache(maxsize=2)
def _records(n: int):
    """(rectification, records [n][1][5HW]) of the synthetic RGB-D camera."""
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rec = np.ascontiguousarray(src.render_rgbd_sequence(n)[:, None, :])
    rec.setflags(write=False)
    return rgbd_undistort(cams[ci]), rec


def _handle(n=1):
    from thor_slam_amd._lib import Handle

    rect, _ = _records(4)
    return Handle([rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=n)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _compare(got, want, msg=""):
    """One view of the device against the reference."""
    np.testing.assert_array_equal(got["depth_m"] > 0, want["depth_m"] > 0, err_msg=f"hit mask {msg}")
    np.testing.assert_array_equal(got["depth_m"].view(np.uint32), want["depth_m"].view(np.uint32), err_msg=f"depth_m {msg}")
    np.testing.assert_array_equal(got["depth_mm"], want["depth_mm"], err_msg=f"depth_mm {msg}")
    if "color" in got:
        np.testing.assert_array_equal(got["color"], want["color"], err_msg=f"color {msg}")
    np.testing.assert_array_equal(got["normal"] != 0, want["normal"] != 0, err_msg=f"normal pattern {msg}")
    err = np.abs(got["normal"].astype(np.float64) - want["normal"].astype(np.float64)).max()
    assert err <= 1e-6, (msg, err)
    return err


def _view(ref, v):
    return {k: a[v] for k, a in ref.items()}


def _zero(out):
    return all(not a.any() for a in out.values())


# -- 1. the analytic scene ---------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
def test_analytic_views(color):
    ref = C.reference(C.DIMS, color)
    C.check_not_empty(ref)
    if color:   # hits on voxels with a colour weight and on voxels without
        hit = ref["depth_m"] > 0
        assert ref["color"][hit].any(axis=-1).any() and (~ref["color"][hit].any(axis=-1)).any()
    tsdf, weight = C.volume()
    h = _handle()
    with pytest.raises(RuntimeError, match="render_init"):
        h.tsdf_render_read(0)
    try:
        with pytest.raises(RuntimeError, match="tsdf_init"):
            h.tsdf_render_init(*C.CAM, **C.PRM)
        if color:
            h.tsdf_color(True)
        h.tsdf_init(C.ORIGIN, C.DIMS, C.S, C.TRUNC_VOX, MAX_D, MAX_W)
        with pytest.raises(RuntimeError, match="render_init"):
            h.tsdf_render(np.eye(4)[None])
        for bad in (dict(step_scale=0.0), dict(step_scale=1.5), dict(max_depth=0.0), dict(min_depth=-1.0), dict(min_weight=-1.0),
                    dict(max_views=0), dict(max_views=257), dict(outputs=0), dict(max_depth=float("inf"))):
            with pytest.raises(RuntimeError, match="tslam error -1"):
                h.tsdf_render_init(*C.CAM, **{**C.PRM, **bad})
        with pytest.raises(RuntimeError, match="tslam error -1"):
            h.tsdf_render_init(0, 45, *C.CAM[2:], **C.PRM)
        h.tsdf_write(tsdf, weight)
        if color:
            h.tsdf_write_color(*C.color_layer())
        h.tsdf_render_init(*C.CAM, max_views=5, outputs=15 if color else 7, **C.PRM)
        ptrs, nbytes = h.tsdf_render_buffers()
        assert nbytes == {"depth_m": 4 * 67 * 45, "depth_mm": 2 * 67 * 45, "normal": 12 * 67 * 45, "color": 3 * 67 * 45}
        assert all(ptrs[k] for k in ("depth_m", "depth_mm", "normal")) and bool(ptrs["color"]) == color
        with pytest.raises(RuntimeError, match="n_views"):
            h.tsdf_render(np.stack([np.eye(4)] * 6))
        # the four views and a NaN pose in the middle, one call
        h.tsdf_render(np.stack([C.OUTSIDE, C.INSIDE, C.NAN, C.AWAY, C.IN_SPHERE]), stream=_stream())
        worst = 0.0
        for slot, v in ((0, 0), (1, 1), (3, 2), (4, 3)):
            worst = max(worst, _compare(h.tsdf_render_read(slot), _view(ref, v), f"view {v}"))
        assert _zero(h.tsdf_render_read(2)) and _zero(h.tsdf_render_read(3))
        print("normals: worst |device - reference|", worst)
        # a shorter call leaves the other slots alone; tslam_reset keeps the state and clears the images
        h.tsdf_render(C.INSIDE[None], stream=_stream())
        _compare(h.tsdf_render_read(0), _view(ref, 1), "slot 0 again")
        _compare(h.tsdf_render_read(4), _view(ref, 3), "slot 4 kept")
        h.reset()
        assert _zero(h.tsdf_render_read(0)) and _zero(h.tsdf_render_read(4))
    finally:
        h.close()


# -- 2. whole tiles and a single pixel ---------------------------------------------------------------
@pytest.mark.parametrize("cam", [(64, 48, 60.0, 150.0, 31.5, 23.5), (1, 1, 60.0, 150.0, 0.0, 0.0)], ids=["64x48", "1x1"])
def test_other_cameras(cam):
    tsdf, weight = C.volume()
    poses = np.stack([C.OUTSIDE, C.INSIDE])
    ref = REF.render(tsdf, weight, C.ORIGIN, C.S, cam, poses, **C.PRM)
    hit = ref["depth_m"] > 0
    assert hit[0].mean() >= 0.25 and hit[1].mean() >= 0.25
    h = _handle()
    try:
        h.tsdf_init(C.ORIGIN, C.DIMS, C.S, C.TRUNC_VOX, MAX_D, MAX_W)
        h.tsdf_write(tsdf, weight)
        h.tsdf_render_init(*cam, max_views=2, outputs=7, **C.PRM)
        h.tsdf_render(poses, stream=_stream())
        for v in range(2):
            _compare(h.tsdf_render_read(v), _view(ref, v), f"view {v}")
    finally:
        h.close()


# -- 3. a volume integrated on the device, host poses and the batch's device poses -----------------
SCENE_ORIGIN, SCENE_DIMS = (-2.025, -1.525, 2.025), (81, 61, 49)      # the room's back wall and the box, 2.2 .. 4.3 m ahead


def test_integrated_volume_host_and_device_poses():
    import torch

    from thor_slam_amd._lib import Handle

    n = 4
    rect, rec = _records(n)
    cam = (W, H, rect.fx, rect.fy, rect.cx, rect.cy)
    h = Handle([rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=n)
    fresh = _handle(2)
    try:
        dev = torch.from_numpy(rec.copy()).cuda()
        s = _stream()
        h.submit(dev.data_ptr(), n, s)
        res = h.read_poses(n)
        T, st = res["T_abs"][:, 0], res["stats"][:, 0, 0]
        used = [s_ == 0 or (s_ == 2 and f == 0) for f, s_ in enumerate(st)]
        assert sum(used) >= 3
        h.tsdf_color(True)
        h.tsdf_init(SCENE_ORIGIN, SCENE_DIMS, C.S, C.TRUNC_VOX, MAX_D, MAX_W)
        h.tsdf_integrate_rgbd(dev.data_ptr(), dev.data_ptr() + 3 * HW, 5 * HW, n, first_frame=0, stream=s)
        tsdf, weight = h.tsdf_read()
        col, cw = h.tsdf_read_color()
        poses = np.stack([T[f] if used[f] else C.NAN for f in range(n)])
        ref = REF.render(tsdf, weight, SCENE_ORIGIN, C.S, cam, poses, color=col, color_weight=cw, **C.PRM)
        hit = ref["depth_m"] > 0
        print("integrated volume: hit fractions", hit.reshape(n, -1).mean(axis=1).round(3), "mean samples",
              ref["samples"].reshape(n, -1).mean(axis=1).round(1))
        assert all(hit[f].mean() >= 0.25 for f in range(n) if used[f])
        nz = np.any(ref["normal"] != 0, axis=-1)
        assert (hit & nz).any() and (hit & ~nz).any() and ref["color"][hit].any()
        h.tsdf_render_init(*cam, max_views=n, **C.PRM)
        h.tsdf_render(poses, stream=s)
        host = [h.tsdf_render_read(v) for v in range(n)]
        h.tsdf_render(None, n_views=n, first_frame=0, stream=s)          # world_T_cam = NULL: the batch's device poses
        for v in range(n):
            got = h.tsdf_render_read(v)
            for k in got:
                np.testing.assert_array_equal(got[k], host[v][k], err_msg=f"{k} view {v}: device poses != host poses")
            _compare(got, _view(ref, v), f"view {v}")
        with pytest.raises(RuntimeError, match="last batch"):
            h.tsdf_render(None, n_views=2, first_frame=3, stream=s)
        # an untracked frame: a handle that has seen two blank frames tracks nothing in the second
        blank = torch.zeros((2, 1, 5 * HW), dtype=torch.uint8, device="cuda")
        fresh.submit(blank.data_ptr(), 2, s)
        assert fresh.read_poses(2)["stats"][1, 0, 0] != 0
        fresh.tsdf_init(SCENE_ORIGIN, SCENE_DIMS, C.S, C.TRUNC_VOX, MAX_D, MAX_W)
        fresh.tsdf_write(tsdf, weight)
        fresh.tsdf_render_init(*cam, max_views=1, outputs=7, **C.PRM)
        fresh.tsdf_render(poses[:1], stream=s)
        assert not _zero(fresh.tsdf_render_read(0))
        fresh.tsdf_render(None, n_views=1, first_frame=1, stream=s)
        assert _zero(fresh.tsdf_render_read(0))
    finally:
        h.close()
        fresh.close()


# -- 4. the rolling window ---------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [C.DIMS, (40, 13, 41)])
def test_shifted_window(dims):
    tsdf, weight = C.volume(dims)
    col, cw = C.color_layer(dims)
    poses = np.stack([C.OUTSIDE, C.INSIDE, C.IN_SPHERE])
    h = _handle()
    try:
        h.tsdf_color(True)
        h.tsdf_init(C.ORIGIN, dims, C.S, C.TRUNC_VOX, MAX_D, MAX_W)
        h.tsdf_write(tsdf, weight)
        h.tsdf_write_color(col, cw)
        h.tsdf_shift((4, 0, 0), stream=_stream())        # the move's wide rows where nx % 4 == 0 ...
        h.tsdf_shift((-4, 0, 0), stream=_stream())
        h.tsdf_shift((3, -1, 2), stream=_stream())       # ... and its scalar rows
        h.tsdf_render_init(*C.CAM, max_views=3, **C.PRM)
        h.tsdf_render(poses, stream=_stream())
        shift, origin = h.tsdf_window()
        assert shift.tolist() == [3, -1, 2]
        assert origin.tolist() == [C.ORIGIN[a] + C.S * float(shift[a]) for a in range(3)]
        t2, w2 = h.tsdf_read()
        c2, cw2 = h.tsdf_read_color()
        assert not np.array_equal(w2, weight) and (w2 > 0).sum() > 1000
        ref = REF.render(t2, w2, tuple(origin), C.S, C.CAM, poses, color=c2, color_weight=cw2, **C.PRM)
        assert all((ref["depth_m"][v] > 0).mean() >= 0.25 for v in range(3))
        unshifted = REF.render(t2, w2, C.ORIGIN, C.S, C.CAM, poses[:1], color=c2, color_weight=cw2, **C.PRM)
        assert not np.array_equal(unshifted["depth_m"][0], ref["depth_m"][0])         # the effective origin matters
        for v in range(3):
            _compare(h.tsdf_render_read(v), _view(ref, v), f"view {v}")
    finally:
        h.close()


# -- 5. engine end to end ----------------------------------------------------------------------------
def test_engine_dense_view():
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    def run(dense_map):
        src = SyntheticRGBDSource(width=W, height=H)
        rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
        rig.start()
        cfg = HipSlamConfig(rgbd=True, dense_map=dense_map, batch_size=3, n_features=1000, n_levels=3, tsdf_origin=SCENE_ORIGIN,
                            tsdf_dims=SCENE_DIMS, voxel_size=C.S)
        eng = HipSlamEngine(num_cameras=2, config=cfg)
        eng.initialize(rig.calibration)
        try:
            for _ in range(6):
                eng.process_frames(rig.get_synchronized_frames())
            eng.flush()
            dm = eng.get_dense_map()
            if dm is None:
                return cfg, None, None, eng.get_dense_view(), None, None, None
            last = eng.handle.read_poses(3)              # the handle's own poses of the newest batch
            explicit = dm["world_T_volume"] @ EXPLICIT   # a camera of the published world, near the first frame's
            return cfg, eng.rectifications[0], dm, eng.get_dense_view(), eng.get_dense_view(world_T_view=explicit, size=(96, 64)), explicit, \
                last["T_abs"][2, 0]
        finally:
            eng.shutdown()

    cfg, rect, dm, view, small, explicit, newest = run(True)
    assert view is not None and small is not None
    # the default camera is pair 0's rectified camera at the newest pose: in the volume's frame the
    # tracked world_T_cam of the batch's last frame (the published pose went through a quaternion)
    np.testing.assert_allclose(view_in_volume(view["world_T_volume"], view["world_T_view"]), newest, rtol=0, atol=1e-9)
    assert np.abs(newest[:3, 3]).max() > 1e-3            # and that is not the first frame's
    prm = dict(min_weight=cfg.mesh_integrator_min_weight, min_depth=0.0, max_depth=cfg.tsdf_integrator_max_integration_distance_m,
               step_scale=cfg.dense_view_step_scale, color=dm["color"], color_weight=dm["color_weight"])
    for got, size in ((view, (W, H)), (small, (96, 64))):
        cam = (size[0], size[1]) + tuple(got["intrinsics"])
        vTc = view_in_volume(got["world_T_volume"], got["world_T_view"])
        ref = REF.render_view(dm["tsdf"], dm["weight"], tuple(dm["origin"]), cfg.voxel_size, cam, vTc, **prm)
        assert (ref["depth_m"] > 0).mean() >= 0.25
        assert got["depth"].shape == (size[1], size[0]) and got["colors"].shape == (size[1], size[0], 3)
        _compare({"depth_m": got["depth"], "depth_mm": got["depth_mm"], "normal": got["normals"], "color": got["colors"]}, ref,
                 f"engine {size}")
        np.testing.assert_array_equal(got["origin"], dm["origin"])
        np.testing.assert_array_equal(got["world_T_volume"], dm["world_T_volume"])
        assert got["window_shift"].tolist() == [0, 0, 0]
    assert view["intrinsics"] == (rect.fx, rect.fy, rect.cx, rect.cy)
    np.testing.assert_array_equal(small["world_T_view"], explicit)
    assert run(False)[3] is None


EXPLICIT = C.pose((0.05, -0.02, 0.1), 5.0)             # in the volume's frame
