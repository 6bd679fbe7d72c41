"""Semi-global aggregation of the dense stereo matcher on the device (``k_sd_sgm.hip``) vs its NumPy
restatement (``tests/ref_stereo_sgm.py``): depth and disp32 bit-exact at the shapes where the
kernels can go wrong (D below and above one lane-load of 64, off a multiple of 32 and of 64, the
largest D, widths off the 64-column step of the winners and the 252-column step of the volume,
heights off the 4-line block and the 8-row band), every path alone and in pairs, the zero-penalty
identity with the box matcher, the widest values u16 has to hold, chunked calls, the tracking
handle's ring-resident images, switching it off again, the engine path and the argument errors."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import ref_stereo_depth as BOX
import ref_stereo_sgm as REF
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.camera.rig import CameraRig
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticStereoSource

pytestmark = pytest.mark.gpu

W0, H0 = 320, 240
ORIGIN = (-2.0, -1.5, 0.5)
DIMS = (80, 60, 100)
MAX_D, MAX_W = 10.0, 100.0
CFG = dict(n_features=1000, n_levels=3, max_disparity=48)   # 48 candidates keep the reference quick
P1, P2 = 100, 1200


def _rect_of(src):
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


@functools.lru_cache(maxsize=None)
def _rendered(width, height, baseline, n=2):
    """n rendered pairs [n][2][H][W] and fx * baseline."""
    src = SyntheticStereoSource(width=width, height=height, baseline=baseline)
    frames = np.stack([np.stack([src.render_image(i, 0), src.render_image(i, 1)]) for i in range(n)])
    frames.setflags(write=False)
    return frames, float(src.get_intrinsics()[0].matrix[0, 0] * baseline)


@functools.lru_cache(maxsize=None)
def _random_pair():
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (1, 2, 40, 72), dtype=np.uint8)
    frames.setflags(write=False)
    return frames


@functools.lru_cache(maxsize=None)
def _want(key, f, n_disp, fxb, p1, p2, paths):
    """The reference's (depth, disp32) of frame f of a cached input, computed once."""
    frames = _random_pair() if key == "random" else _rendered(*key)[0]
    return REF.stereo_depth_sgm(frames[f, 0], frames[f, 1], n_disp, fxb, p1, p2, paths)


@pytest.fixture(scope="module")
def handle():
    from thor_slam_amd._lib import Handle

    h = Handle([_rect_of(SyntheticStereoSource(width=W0, height=H0))], HipSlamConfig(**CFG), max_batch=4)
    yield h
    h.close()


def _run_images(h, frames, fxb, n_disp, sgm=None, init=True):
    """The matcher on caller-supplied images; sgm = keyword arguments of Handle.stereo_depth_sgm or
    None for the box matcher."""
    import torch

    n, _, hh, ww = frames.shape
    dev = torch.from_numpy(np.array(frames)).cuda()      # a writable copy of the cached input
    if init:
        h.stereo_depth_init(max_frames=n, n_disp=n_disp)
    if sgm is not None:
        h.stereo_depth_sgm(**sgm)
    h.stereo_depth_images(dev.data_ptr(), dev.data_ptr() + ww * hh, 2 * ww * hh, ww, hh, fxb, n,
                          torch.cuda.current_stream().cuda_stream)
    return [h.stereo_depth_read(f) for f in range(n)]


def _assert_same(got, want, what=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"disp32 {what}")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"depth {what}")


# (W, H, D): below one step, ragged band, D < 64; D off 32; D > W / 2 and D > 64 off a multiple of
# 64; two steps of the volume at the handle's size; the largest D over three bands.  Baseline 0.3.
# Then widths and heights off every multiple of 8: odd both ways, one column past the 252-column
# step of the box matcher, and a wide strip of 17 rows.
SHAPES = [(72, 40, 24), (200, 136, 40), (96, 64, 72), (320, 240, 64), (320, 24, 256),
          (75, 43, 24), (101, 67, 40), (253, 41, 72), (257, 17, 24)]


@pytest.mark.parametrize("width,height,n_disp", SHAPES)
def test_images_bit_exact(handle, width, height, n_disp):
    key = (width, height, 0.3)
    frames, fxb = _rendered(*key)
    got = _run_images(handle, frames, fxb, n_disp, sgm={})          # default p1, p2, paths
    for f in range(2):
        want = _want(key, f, n_disp, fxb, P1, P2, 15)
        assert (want[0] > 0).mean() > 0.3
        _assert_same(got[f], want, f"of frame {f}")


@pytest.mark.parametrize("paths", [1, 2, 4, 8, 3, 12])
def test_each_path_alone_and_in_pairs(handle, paths):
    key = (200, 136, 0.3)
    frames, fxb = _rendered(*key)
    got = _run_images(handle, frames[:1], fxb, 40, sgm=dict(paths=paths))
    want = _want(key, 0, 40, fxb, P1, P2, paths)
    # a dropped or swapped direction cannot pass: the reference's output for this mask differs from
    # the full mask's, the mirrored mask's (1 <-> 2, 4 <-> 8) and the transposed mask's (1 <-> 4,
    # 2 <-> 8) in hundreds of pixels (the winners; the sub-pixel offsets come from A and do not
    # depend on the mask)
    mirrored = (paths & 1) << 1 | (paths & 2) >> 1 | (paths & 4) << 1 | (paths & 8) >> 1
    transposed = (paths & 3) << 2 | (paths & 12) >> 2
    for other in {15, mirrored, transposed} - {paths}:
        assert (want[1] != _want(key, 0, 40, fxb, P1, P2, other)[1]).sum() >= 100, other
    _assert_same(got[0], want, f"paths {paths}")


def test_zero_penalties_are_the_box_matcher(handle):
    frames, fxb = _rendered(200, 136, 0.3)
    box = _run_images(handle, frames, fxb, 40)
    got = _run_images(handle, frames, fxb, 40, sgm=dict(p1=0, p2=0))
    for f in range(2):
        _assert_same(got[f], box[f], f"vs the device's box matcher, frame {f}")
        _assert_same(got[f], BOX.stereo_depth(frames[f, 0], frames[f, 1], 40, fxb), f"vs the box reference, frame {f}")


@pytest.mark.parametrize("p1,p2", [(2400, 2400), (0, 2400)])
def test_widest_values(handle, p1, p2):
    frames = _random_pair()
    got = _run_images(handle, frames, 50.0, 24, sgm=dict(p1=p1, p2=p2))
    _assert_same(got[0], _want("random", 0, 24, 50.0, p1, p2, 15))


def test_flat_images_give_nothing(handle):
    frames = np.full((2, 2, 136, 200), 117, np.uint8)
    for depth, disp32 in _run_images(handle, frames, 50.0, 40, sgm={}):
        assert not depth.any() and not disp32.any()


def test_chunked_calls(handle):
    key = (72, 40, 0.3, 4)
    frames, fxb = _rendered(*key)
    whole = _run_images(handle, frames, fxb, 24, sgm=dict(chunk_frames=0))
    for f in range(4):
        _assert_same(whole[f], _want(key, f, 24, fxb, P1, P2, 15), f"of frame {f}")
    for chunk in (1, 3):                          # one frame per pass; a ragged last chunk
        got = _run_images(handle, frames, fxb, 24, sgm=dict(chunk_frames=chunk))
        for f in range(4):
            _assert_same(got[f], whole[f], f"of frame {f}, chunk_frames {chunk}")


def test_switching_off(handle):
    frames, fxb = _rendered(72, 40, 0.3)
    box = _run_images(handle, frames, fxb, 24)
    sgm = _run_images(handle, frames, fxb, 24, sgm={})
    assert not np.array_equal(sgm[0][1], box[0][1])
    off = _run_images(handle, frames, fxb, 24, sgm=dict(enable=False), init=False)
    for f in range(2):
        _assert_same(off[f], box[f], f"after enable=False, frame {f}")
    handle.stereo_depth_sgm()
    again = _run_images(handle, frames, fxb, 24)      # stereo_depth_init alone: SGM is off again
    for f in range(2):
        _assert_same(again[f], box[f], f"after a new init, frame {f}")


# -- tracking-handle path ------------------------------------------------------------------------
def _level0(h, g, cam):
    blk = h.frame_block("pyramid", h.ring_slot(g), np.uint8).reshape(h.n_cams, h.pyr_bytes)
    return blk[cam, h.pyr_off[0]:h.pyr_off[0] + h.width * h.height].reshape(h.height, h.width)


def test_tracking_handle_bit_exact():
    import torch

    from thor_slam_amd._lib import Handle

    n = 3
    src = SyntheticStereoSource(width=W0, height=H0)
    rect = _rect_of(src)
    dev = torch.from_numpy(np.ascontiguousarray(src.render_stereo_sequence(n))).cuda()
    s = torch.cuda.current_stream().cuda_stream
    res = []
    for sgm in (False, True):
        h = Handle([rect], HipSlamConfig(**CFG), max_batch=n)
        h.submit(dev.data_ptr(), n, s)
        h.stereo_depth_init(max_frames=n)           # n_disp = the handle's max_disparity
        if sgm:
            h.stereo_depth_sgm()
        h.stereo_depth(0, n, pair=0, stream=s)
        if sgm:
            for f in range(n):
                want = REF.stereo_depth_sgm(_level0(h, f, 0), _level0(h, f, 1), CFG["max_disparity"], rect.fx * rect.baseline,
                                            P1, P2)
                assert (want[0] > 0).mean() > 0.5
                _assert_same(h.stereo_depth_read(f), want, f"of frame {f}")
        res.append(h.read_poses(n))
        h.close()
    for k in ("T_abs", "T_rel", "stats"):
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)


# -- engine --------------------------------------------------------------------------------------
def _engine_run(n=4, **kw):
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.slam.hip_engine import HipSlamEngine

    src = SyntheticStereoSource(width=W0, height=H0)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    cfg = HipSlamConfig(**CFG, batch_size=2, tsdf_origin=ORIGIN, tsdf_dims=DIMS, tsdf_integrator_max_integration_distance_m=MAX_D,
                        tsdf_max_weight=MAX_W, enable_loop_closure=False, dense_map=True, stereo_depth=True, **kw)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    poses = []
    for _ in range(n):
        p = eng.process_frames(rig.get_synchronized_frames())
        poses.append(None if p is None else p.to_4x4_matrix())
    eng.flush()
    poses.append(eng._latest_pose.to_4x4_matrix())
    return eng, src, poses


@functools.lru_cache(maxsize=None)
def _engine_pair():
    """The same 4 frames through the engine with and without SGM: poses, newest depth image, TSDF
    weights, and the reference depth of the SGM run's last matched frame."""
    out = {}
    for sgm in (True, False):
        eng, src, poses = _engine_run(stereo_depth_sgm=sgm)
        r = {"poses": poses, "depth": eng.get_depth_image()[0], "weight": eng.get_dense_map()["weight"]}
        if sgm:
            h, rect = eng._handle, _rect_of(src)
            r["want"] = REF.stereo_depth_sgm(_level0(h, 3, 0), _level0(h, 3, 1), CFG["max_disparity"], rect.fx * rect.baseline,
                                             P1, P2)[0]
        eng.shutdown()
        out[sgm] = r
    return out


def test_engine_depth_with_sgm_and_tracking_untouched():
    run = _engine_pair()
    np.testing.assert_array_equal(run[True]["depth"], run[True]["want"])
    assert not np.array_equal(run[True]["depth"], run[False]["depth"])
    poses, box_poses = run[True]["poses"], run[False]["poses"]
    assert len(poses) == len(box_poses) == 5 and poses[-1] is not None
    for a, b in zip(poses, box_poses):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)


def test_engine_tsdf_observes_no_fewer_voxels_with_sgm():
    """More of every frame carries a depth, so the volume sees at least as many voxels."""
    run = _engine_pair()
    n_sgm, n_box = int((run[True]["weight"] > 0).sum()), int((run[False]["weight"] > 0).sum())
    print(f"observed voxels: SGM {n_sgm}, box {n_box}")
    assert n_box > 10000
    assert n_sgm >= n_box


# -- errors --------------------------------------------------------------------------------------
def test_errors_launch_nothing(handle):
    import torch

    from thor_slam_amd import _lib
    from thor_slam_amd._lib import Handle

    lib = _lib.load_library()
    EINVAL, ESTATE = -1, -4

    def sgm(h, enable=1, p1=100, p2=1200, paths=15, chunk=0, reserved=(0, 0, 0)):
        prm = (ctypes.c_int32 * 8)(enable, p1, p2, paths, chunk, *reserved)
        return lib.tslam_stereo_depth_sgm(h.h, ctypes.addressof(prm))

    fresh = Handle([_rect_of(SyntheticStereoSource(width=W0, height=H0))], HipSlamConfig(**CFG), max_batch=2)
    assert sgm(fresh) == ESTATE                                   # before tslam_stereo_depth_init
    assert sgm(fresh, enable=0) == ESTATE
    fresh.stereo_depth_init(max_frames=2, n_disp=24)
    dev = torch.zeros((1, 2, H0, W0), dtype=torch.uint8, device="cuda")
    fresh.begin_batch(dev.data_ptr(), 1)
    assert sgm(fresh) == ESTATE                                   # inside a batch
    fresh.end_batch()
    assert sgm(fresh) == 0
    fresh.close()

    frames, fxb = _rendered(72, 40, 0.3)
    before = _run_images(handle, frames, fxb, 24, sgm={})
    assert sgm(handle, p1=1201) == EINVAL                         # p1 > p2
    assert sgm(handle, p1=-1) == EINVAL
    assert sgm(handle, p2=2401) == EINVAL
    assert sgm(handle, paths=0) == EINVAL and sgm(handle, paths=16) == EINVAL
    assert sgm(handle, chunk=-1) == EINVAL
    for r in ((1, 0, 0), (0, 0, 7)):
        assert sgm(handle, reserved=r) == EINVAL
    assert lib.tslam_last_error()
    for f in range(2):
        _assert_same(handle.stereo_depth_read(f), before[f], f"after the refused calls, frame {f}")
    # the setting survived them: the same call gives the same output
    after = _run_images(handle, frames, fxb, 24, init=False)
    for f in range(2):
        _assert_same(after[f], before[f], f"of a call after the refused ones, frame {f}")
