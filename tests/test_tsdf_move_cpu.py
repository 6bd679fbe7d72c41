"""The depth archive's rule on the CPU (thor_slam_amd/dense_loop.py through tests/ref_tsdf_move.py):
de-integration inverts integration exactly, a move equals a rebuild at the new poses below
saturation, the selection thresholds, the ring, and ``HipSlamConfig``'s refusals.

Measured on the scenes of tests/tsdf_move_cases.py (max |move - rebuild| of the tsdf, weights
identical): 6 frames / 3 moves 4.5e-8 m against the bound 3.4e-6 m; 12 frames / 6 moves 7.5e-8 m
against 1.4e-5 m.  With ``max_weight = 4`` the 12-frame case differs from the rebuild by up to
0.37 m: the documented limit, so only the rule's own arithmetic is asserted there."""

from __future__ import annotations

import math

import numpy as np
import pytest

import ref_tsdf_move as REF
import tsdf_move_cases as C
from oracle import numpy_tsdf as TS
from thor_slam_amd import dense_loop as DL
from thor_slam_amd.params import HipSlamConfig


def _rebuild(n, max_weight):
    depth, true, _ = C.sequence(n)
    ar = C.archive(max_weight, n)
    ar.integrate(depth, 0, true)
    return ar.tsdf, ar.weight


@pytest.mark.parametrize("n", [6, 12])
def test_removal_is_an_inverse(n):
    depth, _, first = C.sequence(n)
    ar = C.archive(100.0, n)
    ar.integrate(depth, 0, first)
    assert (ar.weight > 0).sum() > 5000 and ar.weight.max() == n
    for e in ar.entries():
        REF.deintegrate(ar.tsdf, ar.weight, e["depth"], e["E"], C.INTR, C.ORIGIN, C.S, C.TRUNC, C.MAX_D)
    assert not ar.weight.any() and not ar.tsdf.any()
    assert not np.signbit(ar.tsdf).any()


@pytest.mark.parametrize("n", [6, 12])
def test_move_equals_rebuild(n):
    t, w, before, moved, entries = C.moved_reference(n, 100.0)
    assert moved == n // 2
    want_t, want_w = _rebuild(n, 100.0)
    assert np.abs(before[0] - want_t).max() > C.S           # the drift was in the map: more than a voxel
    np.testing.assert_array_equal(w, want_w)
    err = float(np.abs(t.astype(np.float64) - want_t.astype(np.float64)).max())
    print(f"{n} frames, {moved} moves: max |move - rebuild| {err:.3g} m, bound {C.bound(n, moved):.3g} m")
    assert err <= C.bound(n, moved)
    _, true, first = C.sequence(n)
    for i, e in enumerate(entries):                          # the archive holds the new poses
        np.testing.assert_array_equal(e["T"], true[i])
        assert e["frame"] == i


def _voxel_by_hand(index, n, max_weight):
    """The rule on one voxel with scalar arithmetic: integrate on the drifted poses, then for each odd
    frame in order the removal on the drifted pose and the insertion on the true pose."""
    depth, true, first = C.sequence(n)
    k, j, i = index
    c = [C.ORIGIN[0] + C.S * (i + 0.5), C.ORIGIN[1] + C.S * (j + 0.5), C.ORIGIN[2] + C.S * (k + 0.5)]
    W, H, fx, fy, cx, cy = C.CAM

    def obs(f, T):
        E = REF.cam_T_world(T)
        p = [((E[r, 0] * c[0] + E[r, 1] * c[1]) + E[r, 2] * c[2]) + E[r, 3] for r in range(3)]
        if not p[2] > 0.0:
            return None
        ix, iy = math.floor(fx * p[0] / p[2] + cx + 0.5), math.floor(fy * p[1] / p[2] + cy + 0.5)
        if not (0 <= ix < W and 0 <= iy < H):
            return None
        d = float(depth[f][iy, ix]) * 0.001
        if not 0.0 < d <= C.MAX_D or d - p[2] < -C.TRUNC:
            return None
        return min(d - p[2], C.TRUNC)

    t, w, steps = np.float32(0.0), np.float32(0.0), 0
    for f in range(n):
        o = obs(f, first[f])
        if o is not None:
            t = np.float32((float(t) * float(w) + o) / (float(w) + 1.0))
            w = np.float32(min(float(w) + 1.0, max_weight))
            steps += 1
    for f in range(1, n, 2):
        o = obs(f, first[f])
        if o is not None:
            w1 = float(w) - 1.0
            t, w = (np.float32((float(t) * float(w) - o) / w1), np.float32(w1)) if w1 > 0.0 else (np.float32(0.0), np.float32(0.0))
            steps += 1
        o = obs(f, true[f])
        if o is not None:
            t = np.float32((float(t) * float(w) + o) / (float(w) + 1.0))
            w = np.float32(min(float(w) + 1.0, max_weight))
            steps += 1
    return t, w, steps


def test_saturated_move_follows_the_rule():
    n, max_weight = 12, 4.0
    t, w, before, moved, _ = C.moved_reference(n, max_weight)
    assert moved == 6 and before[1].max() == max_weight      # the weights did saturate
    want_t, _ = _rebuild(n, max_weight)
    print("saturated: max |move - rebuild|", float(np.abs(t - want_t).max()), "m (the documented limit, not asserted)")
    # voxels at the wall, on the box's edge and where a weight was driven to zero and restarted
    seen = np.argwhere(before[1] == max_weight)
    picks = [tuple(seen[0]), tuple(seen[len(seen) // 2]), tuple(seen[-1])]
    zeroed = np.argwhere((before[1] > 0) & (w < before[1]))
    if len(zeroed):
        picks.append(tuple(zeroed[0]))
    busy = 0
    for idx in picks:
        ht, hw, steps = _voxel_by_hand(idx, n, max_weight)
        assert ht.view(np.uint32) == t[idx].view(np.uint32) and hw == w[idx], (idx, ht, t[idx], hw, w[idx])
        busy = max(busy, steps)
    assert busy > n                                          # a picked voxel took removals and insertions


def test_selection_thresholds():
    T = C.true_pose(2)
    E = REF.cam_T_world(T)
    for scale, want in ((1.0 - 1e-6, False), (1.0 + 1e-6, True)):
        Tt = T.copy()
        Tt[:3, 3] += np.array([0.6, 0.0, 0.8]) * C.MIN_T * scale          # a pure translation of that length
        assert REF.selected(E, REF.cam_T_world(Tt), C.MIN_T, C.MIN_R) is want
        assert DL.moves(DL.pose_entry(T), DL.pose_entry(Tt), C.MIN_T, C.MIN_R) is want
        Tr = T.copy()
        Tr[:3, :3] = T[:3, :3] @ AC_rot(C.MIN_R * scale)                  # the camera turned about its own y axis
        assert REF.selected(E, REF.cam_T_world(Tr), C.MIN_T, C.MIN_R) is want
        assert DL.moves(DL.pose_entry(T), DL.pose_entry(Tr), C.MIN_T, C.MIN_R) is want
    assert not REF.selected(E, E, 0.0, 0.0)                               # an unchanged pose never moves
    np.testing.assert_array_equal(DL.pose_entry(T), np.concatenate([E[:3, :3].reshape(-1), E[:3, 3]]))


def AC_rot(angle):
    return C.AC.rodrigues((0.0, angle, 0.0))


def test_nan_poses_and_unknown_frames_are_ignored():
    n = 6
    depth, true, first = C.sequence(n)
    ar = C.archive(100.0, n)
    ar.integrate(depth, 0, first)
    before = (ar.tsdf.copy(), ar.weight.copy())
    poses = np.stack([np.full((4, 4), np.nan), true[1], true[3]])
    assert ar.move([1, 77, -1], poses, C.MIN_T, C.MIN_R) == 0             # frame 1 with a NaN pose, two unknown ids
    np.testing.assert_array_equal(ar.tsdf.view(np.uint32), before[0].view(np.uint32))
    np.testing.assert_array_equal(ar.weight, before[1])
    assert ar.move([1, 1], np.stack([np.full((4, 4), np.nan), true[1]]), C.MIN_T, C.MIN_R) == 1   # the last entry counts
    assert ar.moved_total == 1


def test_a_skipped_frame_is_not_archived():
    n = 6
    depth, true, _ = C.sequence(n)
    poses = true.copy()
    poses[2] = np.nan
    ar = C.archive(100.0, n, interval=1)
    ar.integrate(depth, 0, poses)
    assert [e["frame"] for e in ar.entries()] == [0, 1, 3, 4, 5]
    every2 = C.archive(100.0, n, interval=2)
    every2.integrate(depth, 0, true)
    assert [e["frame"] for e in every2.entries()] == [0, 2, 4] and every2.weight.max() == 3


def test_ring_evicts_the_oldest():
    n = 6
    t, w, before, moved, entries = C.moved_reference(n, 100.0, capacity=4)
    assert [e["frame"] for e in entries] == [2, 3, 4, 5]
    assert moved == 2                                                      # frames 3 and 5; frame 1 stays baked in
    depth, true, first = C.sequence(n)
    want_t = np.zeros_like(t)
    want_w = np.zeros_like(w)
    for i in range(n):                                                     # the rebuild with frame 1 where it was
        T = first[1] if i == 1 else true[i]
        TS.integrate(want_t, want_w, depth[i], REF.cam_T_world(T), C.INTR, C.ORIGIN, C.S, C.TRUNC, C.MAX_D, 100.0)
    np.testing.assert_array_equal(w, want_w)
    assert np.abs(t.astype(np.float64) - want_t).max() <= C.bound(n, moved)


BASE = dict(rgbd=True, dense_map=True, dense_color=False, dense_loop=True)


def test_config_accepts_the_feature():
    HipSlamConfig(**BASE).validate()
    HipSlamConfig(stereo_depth=True, dense_map=True, dense_loop=True, stereo_depth_interval=5, loop_kf_interval=5).validate()
    cfg = HipSlamConfig()
    assert cfg.dense_loop is False and cfg.dense_loop_capacity == 1024
    assert cfg.dense_loop_min_translation_m is None and cfg.dense_loop_min_rotation_rad == 0.005


@pytest.mark.parametrize("change, message", [
    (dict(dense_map=False), "dense_loop needs dense_map=True"),
    (dict(enable_loop_closure=False), "dense_loop needs enable_loop_closure=True"),
    (dict(devices=(0, 1)), "dense_loop does not run on a sharded rig"),
    (dict(dense_follow=True), "dense_loop does not run with dense_follow"),
    (dict(dense_align=True), "dense_loop does not run with dense_align"),
    (dict(dense_cameras="all"), "dense_loop does not run with dense_cameras"),
    (dict(dense_color=True), "colour is not moved yet"),
    (dict(rgbd=False, stereo_depth=True, stereo_color=True), "colour is not moved yet"),
    (dict(rgbd=False, stereo_depth=True, stereo_depth_interval=2, loop_kf_interval=5), "stereo_depth_interval must divide loop_kf_interval"),
    (dict(dense_loop_capacity=0), "dense_loop_capacity"),
    (dict(dense_loop_min_translation_m=-1.0), "dense_loop_min_translation_m"),
    (dict(dense_loop_min_rotation_rad=4.0), "dense_loop_min_rotation_rad"),
])
def test_config_refusals(change, message):
    with pytest.raises(ValueError, match=message):
        HipSlamConfig(**{**BASE, **change}).validate()
