"""``HipSlamConfig(dense_loop=True)``: the dense map follows the pose graph (thor_slam_amd/dense_loop.py).

The 270-frame circle of tests/test_gpu_loop.py (the body is back at its start at frame 240, so the
engine closes a loop) on a stereo rig with ``stereo_depth``, the volume on the wall the camera faces
at the start and again at the end.  After ``settle()`` the archived frames sit on their nodes' poses
and the device volume equals the archived depth integrated from scratch at the archive's poses
(``oracle.numpy_tsdf``): weights exactly, the tsdf within an f32 rounding per update amplified by the
weight ratio, ``4 (N + 2 moves) N trunc 2^-24``.  The same engine without ``dense_loop`` publishes the
same poses, and its map, integrated on the raw odometry, is not that map."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import ref_tsdf_move as REF
from oracle import numpy_tsdf as TS
from test_gpu_loop import LOOP_FRAMES, _loop_source, _render_many
from thor_slam_amd import dense_loop as DL
from thor_slam_amd.camera import CameraRig, Extrinsics
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

ORIGIN, DIMS, VOX = (-2.0, -1.1, 3.0), (80, 44, 30), 0.05   # the wall ahead of the first frame's camera
TRUNC_VOX, MAX_D, MAX_W = 4.0, 10.0, 100.0
BATCH = 30


@functools.lru_cache(maxsize=1)
def _frames():
    return _render_many(list(range(LOOP_FRAMES)))


def _run(dense_loop: bool):
    """The engine over the loop: (engine, the pose published after every batch)."""
    import torch

    from thor_slam_amd.slam.hip_engine import HipSlamEngine

    src = _loop_source()
    cfg = HipSlamConfig(batch_size=BATCH, enable_loop_closure=True, dense_map=True, stereo_depth=True, stereo_depth_interval=5,
                        dense_color=False, dense_loop=dense_loop, dense_loop_capacity=64, tsdf_max_weight=MAX_W,
                        tsdf_origin=ORIGIN, tsdf_dims=DIMS, voxel_size=VOX)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    eng.initialize(rig.calibration, cfg)
    dev = torch.from_numpy(_frames()).cuda()
    published = []
    for b0 in range(0, LOOP_FRAMES, BATCH):
        eng.process_batch(dev[b0:b0 + BATCH], [src.timestamp(i) for i in range(b0, b0 + BATCH)])
        p = eng._latest_pose
        published.append(None if p is None else p.to_4x4_matrix())
    eng.settle()
    return eng, published


def test_dense_map_follows_the_pose_graph():
    eng, published = _run(True)
    plain, published_plain = _run(False)
    try:
        cfg = eng._config
        assert eng.loop_closures, "no loop closed"
        ar = eng.get_dense_archive()
        pg = eng.pose_graph
        n = len(ar["frames"])
        print("archived", n, "frames; moved_last", ar["moved_last"], "moved_total", ar["moved_total"], "loops", eng.loop_closures)
        assert ar["moved_total"] >= 1 and 1 <= n < min(cfg.dense_loop_capacity, MAX_W)
        assert plain.get_dense_archive() is None
        # every archived frame has a node and sits on its pose, within the selection thresholds
        node = {g: T for g, T in zip(pg["frames"], pg["T"])}
        assert set(ar["frames"].tolist()) == set(node)
        exact = 0
        for g, T in zip(ar["frames"].tolist(), ar["world_T_cam"]):
            assert not DL.moves(DL.pose_entry(T), DL.pose_entry(node[g]), 0.5 * VOX, cfg.dense_loop_min_rotation_rad), g
            exact += int(np.array_equal(T, node[g]))
        assert exact >= ar["moved_last"] >= 1
        # the device volume == the archived depth integrated from scratch at the archive's poses
        r = eng.rectifications[0]
        intr = (r.fx, r.fy, r.cx, r.cy)
        want_t = np.zeros(DIMS[::-1], np.float32)
        want_w = np.zeros(DIMS[::-1], np.float32)
        for i in range(n):
            TS.integrate(want_t, want_w, eng.handle.tsdf_archive_read_depth(i), REF.cam_T_world(ar["world_T_cam"][i]), intr,
                         ORIGIN, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W)
        dm = eng.get_dense_map()
        assert (want_w > 0).sum() > 10000
        np.testing.assert_array_equal(dm["weight"], want_w)
        bound = 4.0 * (n + 2 * ar["moved_total"]) * n * TRUNC_VOX * VOX * 2.0 ** -24
        err = float(np.abs(dm["tsdf"].astype(np.float64) - want_t).max())
        print(f"max |device - rebuild| {err:.3g} m, bound {bound:.3g} m")
        assert err <= bound
        # without dense_loop: the same published poses, and a map that kept the drift
        assert len(published) == len(published_plain)
        for a, b in zip(published, published_plain):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
        pm = plain.get_dense_map()
        both = (pm["weight"] == want_w) & (want_w > 0)
        drift = float(np.abs(pm["tsdf"].astype(np.float64) - want_t)[both].max())
        print(f"without dense_loop: max |map - rebuild| {drift:.3g} m over {int(both.sum())} voxels of equal weight")
        assert drift > VOX
        # reset() clears the archive with the map
        eng.reset()
        a0 = eng.get_dense_archive()
        assert len(a0["frames"]) == 0 and a0["moved_total"] == 0 and not eng.get_dense_map()["weight"].any()
    finally:
        eng.shutdown()
        plain.shutdown()
