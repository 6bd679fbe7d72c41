"""The three entry routes into the frame pipeline agree bit for bit: (a) ``tslam_submit``
(``TSLAM_STAGE_ALL``), (b) the five ``TSLAM_STAGE_*`` codes, (c) the eight ``TSLAM_KERNEL_*`` codes.

Each route runs on a fresh handle over the same input, two batches of two frames, for a stereo
handle at 320x240 with 3 pyramid levels (the smallest shape the library accepts with the default
margin) and for an RGB-D handle of the same size (an even pixel count, as its u16 depth needs).
The pipeline's buffers are compared whole after the last batch, so the ring slots of both batches
are covered.  Route (c) has no rig and no loop store to run, so its pose records match (a)'s too:
``T_rel`` after the pose kernel and ``T_abs`` after the chain kernel.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from helpers import make_source, rig_calibration
from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort, stereo_pairs, stereo_rectify
from thor_slam_amd.camera.rig import CameraRig
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticRGBDSource

pytestmark = pytest.mark.gpu

W, H, BATCH, N = 320, 240, 2, 4
STAGES = ("rectify", "detect", "describe", "match", "pose")
KERNELS = ("rectify_pyramid", "detect", "select", "describe", "match", "match_refine", "pose", "chain")
BUFFERS = {"keypoints": np.uint32, "kcount": np.int32, "desc": np.uint32, "stereo": np.int32, "temporal": np.int32,
           "temporal_uv": np.uint64, "corr": np.uint64, "stats": np.int32, "pose": np.uint64}   # f64 as bits: NaN-safe


@functools.lru_cache(maxsize=None)
def _input(kind: str):
    if kind == "stereo":
        src = make_source(0, W, H)
        cams = extract_cameras(rig_calibration(src), 2)
        (li, ri), = stereo_pairs(cams)
        cfg = HipSlamConfig(n_features=500, n_levels=3)
        return stereo_rectify(cams[li], cams[ri]), cfg, src.render_stereo_sequence(N)
    src = SyntheticRGBDSource(width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    cfg = HipSlamConfig(rgbd=True, n_features=500, n_levels=3)
    return rgbd_undistort(cams[ci]), cfg, src.render_rgbd_sequence(N)[:, None, :]


@functools.lru_cache(maxsize=None)
def _run(kind: str, route: str):
    import torch

    from thor_slam_amd._lib import Handle

    rect, cfg, frames = _input(kind)
    h = Handle([rect], cfg, max_batch=BATCH)
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    for b0 in range(0, N, BATCH):
        if route == "submit":
            h.submit(dev[b0:].data_ptr(), BATCH, s)
            continue
        h.begin_batch(dev[b0:].data_ptr(), BATCH)
        for name in (STAGES if route == "stages" else KERNELS):
            (h.run_stage if route == "stages" else h.run_kernel)(name, s)
        h.end_batch()
    out = {k: h.copy_out(k, 0, h.buffer_info(k)[1], dt).copy() for k, dt in BUFFERS.items()}
    out["poses"] = h.read_poses(BATCH)
    h.close()
    return out


@pytest.mark.parametrize("kind", ["stereo", "rgbd"])
def test_entry_routes_agree(kind):
    a, b, c = _run(kind, "submit"), _run(kind, "stages"), _run(kind, "kernels")
    assert (a["poses"]["stats"][1:, 0, 0] == 0).all(), "the reference route lost tracking: nothing to compare"
    assert (a["kcount"] > 0).any() and (a["temporal"] >= 0).any()
    for k in BUFFERS:
        if k == "stereo" and kind == "rgbd":
            continue   # an RGB-D handle has no stereo matcher: its disparities come from the depth image
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{kind}: {k}, submit vs stage codes")
        if k != "pose":
            np.testing.assert_array_equal(a[k], c[k], err_msg=f"{kind}: {k}, submit vs kernel codes")
    for k in ("T_rel", "T_abs", "cov", "stats"):
        np.testing.assert_array_equal(a["poses"][k], b["poses"][k], err_msg=f"{kind}: read_poses {k}, submit vs stage codes")
    for k in ("T_rel", "T_abs"):
        np.testing.assert_array_equal(a["poses"][k], c["poses"][k], err_msg=f"{kind}: {k}, submit vs kernel codes")
