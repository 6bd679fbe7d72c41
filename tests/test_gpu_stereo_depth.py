"""Dense stereo depth on the device (``k_stereo_depth.hip``) vs its NumPy restatement
(``tests/ref_stereo_depth.py``): depth and disp32 bit-exact at the shapes where the kernel can go
wrong (widths off the 252-column step, heights off the 8-row band, D off a multiple of 32, D > W/2,
images below the handle's size), on a tracking handle's ring-resident rectified images (with and
without distortion, second pair of a two-pair handle), the TSDF integrated from that depth in the
rectified camera, the engine path, and the argument errors."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import ref_stereo_depth as REF
from helpers import DISTORTION
from oracle import numpy_tsdf as TS
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.camera.rig import CameraRig
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticStereoSource

pytestmark = pytest.mark.gpu

W0, H0 = 320, 240
ORIGIN = (-2.0, -1.5, 0.5)
DIMS = (80, 60, 100)
VOX, TRUNC_VOX, MAX_D, MAX_W = 0.05, 4.0, 10.0, 100.0
CFG = dict(n_features=1000, n_levels=3, max_disparity=48)   # 48 candidates keep the reference quick


def _inv(T):
    """cam_T_world with k_tsdf_poses' expression order."""
    out = np.eye(4)
    for r in range(3):
        for k in range(3):
            out[r, k] = T[k, r]
        out[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return out


def _rect_of(src):
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


@functools.lru_cache(maxsize=None)
def _rendered(width, height, baseline, n=2):
    """n rendered pairs [n][2][H][W] and fx * baseline."""
    src = SyntheticStereoSource(width=width, height=height, baseline=baseline)
    frames = np.stack([np.stack([src.render_image(i, 0), src.render_image(i, 1)]) for i in range(n)])
    return frames, float(src.get_intrinsics()[0].matrix[0, 0] * baseline)


@pytest.fixture(scope="module")
def handle():
    from thor_slam_amd._lib import Handle

    h = Handle([_rect_of(SyntheticStereoSource(width=W0, height=H0))], HipSlamConfig(**CFG), max_batch=4)
    yield h
    h.close()


def _run_images(h, frames, fxb, n_disp, uniqueness=10, lr_tol=1):
    import torch

    n, _, hh, ww = frames.shape
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    h.stereo_depth_init(max_frames=n, n_disp=n_disp, uniqueness=uniqueness, lr_tol=lr_tol)
    h.stereo_depth_images(dev.data_ptr(), dev.data_ptr() + ww * hh, 2 * ww * hh, ww, hh, fxb, n,
                          torch.cuda.current_stream().cuda_stream)
    return [h.stereo_depth_read(f) for f in range(n)]


def _check_images(h, frames, fxb, n_disp, uniqueness=10, lr_tol=1, want_valid=True):
    got = _run_images(h, frames, fxb, n_disp, uniqueness, lr_tol)
    for f, (depth, disp32) in enumerate(got):
        want_depth, want_disp = REF.stereo_depth(frames[f, 0], frames[f, 1], n_disp, fxb, uniqueness, lr_tol)
        if want_valid:
            assert (want_depth > 0).mean() > 0.3
        np.testing.assert_array_equal(disp32, want_disp, err_msg=f"disp32 of frame {f}")
        np.testing.assert_array_equal(depth, want_depth, err_msg=f"depth of frame {f}")


# (W, H, D, baseline): below one step and band-ragged; one step with a ragged band and D off 32;
# two steps (320 = 252 + 68) at the handle's size; the default baseline; D > W / 2; then widths and
# heights that are no multiple of 8 (or of 2): odd both ways, one column past the 252-column step,
# and a wide strip of two bands and one row
SHAPES = [(72, 40, 24, 0.3), (200, 136, 40, 0.3), (320, 240, 64, 0.3), (320, 240, 32, 0.075), (96, 64, 64, 0.3),
          (75, 43, 24, 0.3), (101, 67, 40, 0.3), (253, 41, 72, 0.3), (257, 17, 24, 0.3)]


@pytest.mark.parametrize("width,height,n_disp,baseline", SHAPES)
def test_images_bit_exact(handle, width, height, n_disp, baseline):
    frames, fxb = _rendered(width, height, baseline)
    _check_images(handle, frames, fxb, n_disp)


def test_images_no_uniqueness_no_lr_tolerance(handle):
    frames, fxb = _rendered(200, 136, 0.3)
    _check_images(handle, frames, fxb, 40, uniqueness=0, lr_tol=0)


def test_flat_images_give_nothing(handle):
    frames = np.full((2, 2, 136, 200), 117, np.uint8)
    got = _run_images(handle, frames, 50.0, 40)
    for depth, disp32 in got:
        assert not depth.any() and not disp32.any()
    _check_images(handle, frames, 50.0, 40, want_valid=False)


# -- tracking-handle path ------------------------------------------------------------------------
def _level0(h, g, cam):
    blk = h.frame_block("pyramid", h.ring_slot(g), np.uint8).reshape(h.n_cams, h.pyr_bytes)
    return blk[cam, h.pyr_off[0]:h.pyr_off[0] + h.width * h.height].reshape(h.height, h.width)


@functools.lru_cache(maxsize=None)
def _tracked(distorted: bool, n: int = 3):
    """A 320x240 one-pair handle after one batch of n frames, its stereo depth of those frames, and
    the reference depth of the ring's rectified images."""
    import torch

    from thor_slam_amd._lib import Handle

    src = SyntheticStereoSource(width=W0, height=H0, distortion=DISTORTION if distorted else None)
    rect = _rect_of(src)
    assert rect.is_identity != distorted
    cfg = HipSlamConfig(**CFG)
    h = Handle([rect], cfg, max_batch=n)
    dev = torch.from_numpy(np.ascontiguousarray(src.render_stereo_sequence(n))).cuda()
    s = torch.cuda.current_stream().cuda_stream
    h.submit(dev.data_ptr(), n, s)
    h.stereo_depth_init(max_frames=n)           # n_disp = the handle's max_disparity
    h.stereo_depth(0, n, pair=0, stream=s)
    got = [h.stereo_depth_read(f) for f in range(n)]
    n_disp = cfg.max_disparity
    want = [REF.stereo_depth(_level0(h, f, 0), _level0(h, f, 1), n_disp, rect.fx * rect.baseline) for f in range(n)]
    return {"h": h, "rect": rect, "got": got, "want": want, "res": h.read_poses(n), "n": n, "stream": s}


@pytest.mark.parametrize("distorted", [False, True])
def test_tracking_handle_bit_exact(distorted):
    t = _tracked(distorted)
    for f in range(t["n"]):
        assert (t["want"][f][0] > 0).mean() > 0.5
        np.testing.assert_array_equal(t["got"][f][1], t["want"][f][1], err_msg=f"disp32 of frame {f}")
        np.testing.assert_array_equal(t["got"][f][0], t["want"][f][0], err_msg=f"depth of frame {f}")


def test_second_pair_of_a_rig():
    import torch

    from helpers import rig_scene
    from thor_slam_amd._lib import Handle

    sc = rig_scene(n=2, width=W0, height=H0)
    h = Handle(sc["rects"], HipSlamConfig(**CFG), max_batch=2)
    dev = torch.from_numpy(np.ascontiguousarray(sc["frames"])).cuda()
    s = torch.cuda.current_stream().cuda_stream
    h.submit(dev.data_ptr(), 2, s)
    h.stereo_depth_init(max_frames=2, n_disp=48)
    h.stereo_depth(0, 2, pair=1, stream=s)
    rect = sc["rects"][1]
    for f in range(2):
        depth, disp32 = h.stereo_depth_read(f)
        want_depth, want_disp = REF.stereo_depth(_level0(h, f, 2), _level0(h, f, 3), 48, rect.fx * rect.baseline)
        assert (want_depth > 0).mean() > 0.3
        np.testing.assert_array_equal(disp32, want_disp)
        np.testing.assert_array_equal(depth, want_depth)
    h.close()


# -- TSDF from stereo ----------------------------------------------------------------------------
def _oracle_tsdf(rect, depth, world_T_cam, use):
    t = np.zeros(DIMS[::-1], dtype=np.float32)
    w = np.zeros(DIMS[::-1], dtype=np.float32)
    for d, T, u in zip(depth, world_T_cam, use):
        if u:
            TS.integrate(t, w, d, _inv(T), (rect.fx, rect.fy, rect.cx, rect.cy), ORIGIN, VOX, TRUNC_VOX * VOX, MAX_D,
                         MAX_W, None)
    return t, w


def _used(res):
    return [s == 0 or (s == 2 and f == 0) for f, s in enumerate(res["stats"][:, 0, 0])]


@pytest.mark.parametrize("distorted", [False, True])
def test_tsdf_from_stereo_bit_exact(distorted):
    t = _tracked(distorted)
    h, n = t["h"], t["n"]
    depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
    assert frame_bytes == 2 * W0 * H0
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.tsdf_integrate_rect(depth_ptr, frame_bytes, n, first_frame=0, stream=t["stream"])   # device poses
    got_t, got_w = h.tsdf_read()
    want_t, want_w = _oracle_tsdf(t["rect"], [d for d, _ in t["want"]], t["res"]["T_abs"][:, 0], _used(t["res"]))
    assert (want_w > 0).sum() > 10000
    np.testing.assert_array_equal(got_w, want_w)
    np.testing.assert_array_equal(got_t, want_t)
    # the raw-camera entry point looks depth up through the undistortion table: wrong for this depth
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.tsdf_integrate(depth_ptr, frame_bytes, n, first_frame=0, stream=t["stream"])
    raw_t, raw_w = h.tsdf_read()
    same = np.array_equal(raw_t, want_t) and np.array_equal(raw_w, want_w)
    assert same != distorted


# -- engine --------------------------------------------------------------------------------------
def _engine_run(n=4, **kw):
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.slam.hip_engine import HipSlamEngine

    src = SyntheticStereoSource(width=W0, height=H0)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    cfg = HipSlamConfig(**CFG, batch_size=2, tsdf_origin=ORIGIN, tsdf_dims=DIMS, tsdf_integrator_max_integration_distance_m=MAX_D,
                        tsdf_max_weight=MAX_W, enable_loop_closure=False, **kw)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    poses, stamps = [], []
    for _ in range(n):
        fs = rig.get_synchronized_frames()
        stamps.append(float(fs.timestamp))
        p = eng.process_frames(fs)      # the pose published so far (batches of 2)
        poses.append(None if p is None else p.to_4x4_matrix())
    eng.flush()
    poses.append(eng._latest_pose.to_4x4_matrix())
    return eng, src, poses, stamps


def _handle_level_volume(src, frames_used, n=4, batch=2):
    """The handle-level path on the same frames: per batch submit, stereo_depth and
    tsdf_integrate_rect of the chosen frames with the device poses."""
    import torch

    from thor_slam_amd._lib import Handle

    rect = _rect_of(src)
    h = Handle([rect], HipSlamConfig(**CFG), max_batch=batch)
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.stereo_depth_init(max_frames=batch)
    depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
    seq = src.render_stereo_sequence(n)
    s = torch.cuda.current_stream().cuda_stream
    g_last = max(frames_used)
    for b in range(0, n, batch):
        dev = torch.from_numpy(np.ascontiguousarray(seq[b:b + batch])).cuda()
        h.submit(dev.data_ptr(), batch, s)
        for g in range(b, b + batch):
            if g in frames_used:
                h.stereo_depth(g, 1, stream=s)
                h.tsdf_integrate_rect(depth_ptr, frame_bytes, 1, first_frame=g, stream=s)
    vol = h.tsdf_read()
    # the newest matched frame (still in slot 0 and in the ring): device depth and reference depth
    last = (h.stereo_depth_read(0)[0],
            REF.stereo_depth(_level0(h, g_last, 0), _level0(h, g_last, 1), CFG["max_disparity"], rect.fx * rect.baseline)[0])
    h.close()
    return vol, last


def test_engine_dense_map_from_stereo():
    eng, src, poses, stamps = _engine_run(dense_map=True, stereo_depth=True)
    dm = eng.get_dense_map()
    assert "color" not in dm
    (want_t, want_w), (dev_depth, ref_depth) = _handle_level_volume(src, {0, 1, 2, 3})
    assert (want_w > 0).sum() > 10000
    np.testing.assert_array_equal(dm["weight"], want_w)
    np.testing.assert_array_equal(dm["tsdf"], want_t)
    assert eng.get_mesh()["triangles"].shape[0] > 1000
    depth, stamp = eng.get_depth_image()
    assert stamp == stamps[-1]
    np.testing.assert_array_equal(dev_depth, ref_depth)
    np.testing.assert_array_equal(depth, ref_depth)
    eng.shutdown()


def test_engine_interval_and_tracking_untouched():
    eng, src, poses, _ = _engine_run(dense_map=True, stereo_depth=True, stereo_depth_interval=2)
    dm = eng.get_dense_map()
    (want_t, want_w), _ = _handle_level_volume(src, {0, 2})
    np.testing.assert_array_equal(dm["weight"], want_w)
    np.testing.assert_array_equal(dm["tsdf"], want_t)
    (all_t, all_w), _ = _handle_level_volume(src, {0, 1, 2, 3})
    assert not np.array_equal(all_w, want_w)      # frames 1 and 3 were left out
    eng.shutdown()
    plain, _, plain_poses, _ = _engine_run(sync=True)
    assert plain.get_depth_image() is None
    plain.shutdown()
    assert len(poses) == len(plain_poses) == 5 and poses[-1] is not None
    for a, b in zip(poses, plain_poses):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)


# -- errors --------------------------------------------------------------------------------------
def test_errors_launch_nothing(handle):
    import ctypes

    import torch

    from thor_slam_amd import _lib
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import rgbd_pairs, rgbd_undistort
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    lib = _lib.load_library()
    EINVAL, ESTATE = -1, -4

    def init(h, n_disp, frames=2):
        prm = (ctypes.c_int32 * 4)(n_disp, 10, 1, 0)
        return lib.tslam_stereo_depth_init(h.h, ctypes.addressof(prm), frames)

    fresh = Handle([_rect_of(SyntheticStereoSource(width=W0, height=H0))], HipSlamConfig(**CFG), max_batch=2)
    assert lib.tslam_stereo_depth(fresh.h, 0, 0, 1, None) == ESTATE               # before init
    assert lib.tslam_stereo_depth_buffers(fresh.h, None, None, None) == ESTATE
    assert init(fresh, 3) == EINVAL and init(fresh, 257) == EINVAL
    assert lib.tslam_stereo_depth(fresh.h, 0, 0, 1, None) == ESTATE               # a refused init leaves it off
    assert init(fresh, 32) == 0
    img = torch.zeros((3, 2, H0, W0), dtype=torch.uint8, device="cuda")
    args = (ctypes.c_void_p(img.data_ptr()), ctypes.c_void_p(img.data_ptr() + W0 * H0), 2 * W0 * H0)
    assert lib.tslam_stereo_depth_images(fresh.h, *args, W0, H0, 30.0, 3, None) == EINVAL     # n > max_frames
    assert lib.tslam_stereo_depth_images(fresh.h, *args, W0 + 1, H0, 30.0, 1, None) == EINVAL  # above the handle's size
    assert lib.tslam_stereo_depth_images(fresh.h, *args, 8, H0, 30.0, 1, None) == EINVAL
    assert lib.tslam_stereo_depth(fresh.h, 0, 0, 1, None) == EINVAL               # no batch yet: no such frame
    assert lib.tslam_stereo_depth(fresh.h, 1, 0, 0, None) == EINVAL               # no such pair
    assert lib.tslam_last_error()
    fresh.close()

    src = SyntheticRGBDSource(width=W0, height=H0)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rgbd = Handle([rgbd_undistort(cams[ci])], HipSlamConfig(rgbd=True, **CFG), max_batch=1)
    assert init(rgbd, 32) == ESTATE
    rgbd.close()
