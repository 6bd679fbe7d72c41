"""The depth archive on the device: ``tslam_tsdf_archive_init`` / ``_integrate`` / ``_move`` /
``_read`` / ``_read_depth`` (``k_tsdf_move_frames.hip``) against tests/ref_tsdf_move.py.

The volume after an integrate and a move is bit-equal to the reference's (``tsdf`` and ``weight``
compared as u32): both apply the same IEEE f64 operations in the same order and store f32 after every
update, below saturation and at it.  Host poses go in, so no images are submitted; the handle is the
rectified analytic one of tests/test_gpu_tsdf_align.py with ``tsdf_align_cases.DEVICE_CAM``."""

from __future__ import annotations

import numpy as np
import pytest

import ref_tsdf_move as REF
import tsdf_move_cases as C
from thor_slam_amd.dense_loop import MOVE_CHUNK
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

W, H = C.CAM[:2]
NAN = np.full((4, 4), np.nan)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _handle(table=None):
    """A handle whose pair-0 camera is DEVICE_CAM, rectified, or with an undistortion table."""
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import StereoRectification

    _, _, fx, fy, cx, cy = C.CAM
    rect = StereoRectification(W, H, fx, fy, cx, cy, 0.1, np.eye(3), np.eye(3), table, table, table is None)
    return Handle([rect], HipSlamConfig(n_features=256, n_levels=1), max_batch=1)


def _upload(depth):
    import torch

    return torch.from_numpy(np.ascontiguousarray(depth).view(np.int16).copy()).cuda()


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _volume(h, max_weight):
    h.tsdf_init(C.ORIGIN, C.DIMS, C.S, C.TRUNC_VOX, C.MAX_D, max_weight)


def _same_volume(h, tsdf, weight):
    t, w = h.tsdf_read()
    np.testing.assert_array_equal(_u32(w), _u32(weight))
    np.testing.assert_array_equal(_u32(t), _u32(tsdf))


@pytest.mark.parametrize("n, max_weight", [(6, 100.0), (12, 100.0), (12, 4.0)])
def test_integrate_and_move_bit_exact(n, max_weight):
    depth, true, first = C.sequence(n)
    want_t, want_w, before, moved, entries = C.moved_reference(n, max_weight)
    h = _handle()
    try:
        _volume(h, max_weight)
        h.tsdf_archive_init(capacity=n, rect=True)
        dev = _upload(depth)
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, n, first_frame=0, world_T_cam=first, stream=_stream())
        _same_volume(h, *before)
        a0 = h.tsdf_archive_read()
        assert a0["count"] == n and a0["moved_last"] == 0 and a0["moved_total"] == 0
        np.testing.assert_array_equal(a0["frames"], np.arange(n))
        np.testing.assert_array_equal(_bits(a0["world_T_cam"]), _bits(first))
        for i in (0, n - 1):
            np.testing.assert_array_equal(h.tsdf_archive_read_depth(i), depth[i])
        h.tsdf_archive_move(np.arange(n), true, C.MIN_T, C.MIN_R, stream=_stream())
        _same_volume(h, want_t, want_w)
        assert (want_w > 0).sum() > 5000
        # the archive: moved frames hold the new poses bit for bit, the others what they had
        a1 = h.tsdf_archive_read()
        assert a1["moved_last"] == moved == n // 2 and a1["moved_total"] == moved
        np.testing.assert_array_equal(_bits(a1["world_T_cam"]), _bits(np.stack([e["T"] for e in entries])))
        np.testing.assert_array_equal(_bits(a1["world_T_cam"][1::2]), _bits(true[1::2]))
        np.testing.assert_array_equal(_bits(a1["world_T_cam"][0::2]), _bits(first[0::2]))
        # nothing to move: the same poses again, NaN poses, unknown frames; the bytes stay
        h.tsdf_archive_move(np.arange(n), true, C.MIN_T, C.MIN_R, stream=_stream())
        h.tsdf_archive_move([1, 500, -3], np.stack([NAN, first[1], first[1]]), C.MIN_T, C.MIN_R, stream=_stream())
        h.tsdf_archive_move([], np.zeros((0, 4, 4)), C.MIN_T, C.MIN_R, stream=_stream())
        _same_volume(h, want_t, want_w)
        a2 = h.tsdf_archive_read()
        assert a2["moved_last"] == 0 and a2["moved_total"] == moved
        np.testing.assert_array_equal(_bits(a2["world_T_cam"]), _bits(a1["world_T_cam"]))
        # tslam_reset empties the ring and the volume, the archive stays on
        h.reset()
        assert h.tsdf_archive_read()["count"] == 0 and not h.tsdf_read()[1].any()
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, 1, first_frame=0, world_T_cam=true[:1], stream=_stream())
        assert h.tsdf_archive_read()["count"] == 1
    finally:
        h.close()


def test_more_selected_frames_than_one_chunk():
    """MOVE_CHUNK + 2 frames, every one of them moved: the order holds across the chunks (the volume
    saturates at max_weight 8, so a wrong order would show)."""
    n = MOVE_CHUNK + 2
    depth6, true6, first6 = C.sequence(6)
    idx = np.arange(n) % 6
    depth, old = depth6[idx], first6[idx].copy()
    new = true6[(idx + 1) % 6].copy()
    for i in range(n):                                   # distinct poses per frame, all past the thresholds
        old[i, 0, 3] += 1e-4 * i
        new[i, 2, 3] += 0.05 + 1e-4 * i
    ar = C.archive(8.0, n)
    ar.integrate(depth, 0, old)
    assert ar.move(np.arange(n), new, C.MIN_T, C.MIN_R) == n
    h = _handle()
    try:
        _volume(h, 8.0)
        h.tsdf_archive_init(capacity=n, rect=True)
        dev = _upload(depth)
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, n, first_frame=0, world_T_cam=old, stream=_stream())
        h.tsdf_archive_move(np.arange(n)[::-1], new[::-1], C.MIN_T, C.MIN_R, stream=_stream())   # the request's order does not matter
        _same_volume(h, ar.tsdf, ar.weight)
        a = h.tsdf_archive_read()
        assert a["moved_last"] == n
        np.testing.assert_array_equal(_bits(a["world_T_cam"]), _bits(new))
    finally:
        h.close()


def test_ring_eviction_interval_and_skipped_frames():
    """Capacity 4 and six frames in two calls: the first two are evicted and stay baked in; then an
    interval of 2 with a NaN pose: only frames 0 and 4 are integrated and archived."""
    n = 6
    depth, true, first = C.sequence(n)
    want_t, want_w, _, moved, entries = C.moved_reference(n, 100.0, capacity=4)
    h = _handle()
    try:
        _volume(h, 100.0)
        h.tsdf_archive_init(capacity=4, rect=True)
        dev = _upload(depth)
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, 5, first_frame=0, world_T_cam=first[:5], stream=_stream())
        h.tsdf_archive_integrate(dev.data_ptr() + 5 * 2 * W * H, 2 * W * H, 1, first_frame=5, world_T_cam=first[5:], stream=_stream())
        h.tsdf_archive_move(np.arange(n), true, C.MIN_T, C.MIN_R, stream=_stream())
        _same_volume(h, want_t, want_w)
        a = h.tsdf_archive_read()
        assert a["count"] == 4 and a["moved_last"] == moved == 2
        np.testing.assert_array_equal(a["frames"], [e["frame"] for e in entries])
        np.testing.assert_array_equal(_bits(a["world_T_cam"]), _bits(np.stack([e["T"] for e in entries])))
        for i, e in enumerate(entries):
            np.testing.assert_array_equal(h.tsdf_archive_read_depth(i), e["depth"])
        assert h.tsdf_archive_read(max_frames=2)["frames"].tolist() == [2, 3]
        # a new ring: interval 2, frame 2's pose NaN
        _volume(h, 100.0)
        assert h.tsdf_archive_read()["count"] == 0              # tslam_tsdf_init turned the archive off
        h.tsdf_archive_init(capacity=4, interval=2, rect=True)
        poses = true.copy()
        poses[2] = np.nan
        ar = C.archive(100.0, 4, interval=2)
        ar.integrate(depth, 0, poses)
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, n, first_frame=0, world_T_cam=poses, stream=_stream())
        _same_volume(h, ar.tsdf, ar.weight)
        a = h.tsdf_archive_read()
        assert a["frames"].tolist() == [0, 4] and ar.weight.max() == 2
    finally:
        h.close()


def test_table_path():
    """rect=0 on a handle with an undistortion table: the depth is looked up through it, at
    integration, at the removal and at the re-insertion."""
    n = 6
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    table = np.stack([32 * xs + np.rint(48 * np.sin(ys / 9.0)), 32 * ys + np.rint(40 * np.cos(xs / 7.0))], axis=-1).astype(np.int32)
    depth, true, first = C.sequence(n)
    ar = C.archive(100.0, n, mp=table)
    ar.integrate(depth, 0, first)
    assert ar.move(np.arange(n), true, C.MIN_T, C.MIN_R) == 3
    plain = C.moved_reference(n, 100.0)
    assert (ar.tsdf != plain[0]).any()                           # the table matters in this scene
    h = _handle(table)
    try:
        _volume(h, 100.0)
        h.tsdf_archive_init(capacity=n, rect=False)
        dev = _upload(depth)
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, n, first_frame=0, world_T_cam=first, stream=_stream())
        h.tsdf_archive_move(np.arange(n), true, C.MIN_T, C.MIN_R, stream=_stream())
        _same_volume(h, ar.tsdf, ar.weight)
        np.testing.assert_array_equal(h.tsdf_archive_read_depth(3), depth[3])
    finally:
        h.close()


def test_selection_thresholds_on_the_device():
    """Frames just inside and just outside each threshold, decided as the rule says."""
    n = 6
    depth, true, _ = C.sequence(n)
    new = true.copy()
    step = np.array([0.6, 0.0, 0.8]) * C.MIN_T
    new[0, :3, 3] += step * (1.0 - 1e-6)
    new[1, :3, 3] += step * (1.0 + 1e-6)
    new[2, :3, :3] = true[2, :3, :3] @ C.AC.rodrigues((0.0, C.MIN_R * (1.0 - 1e-6), 0.0))
    new[3, :3, :3] = true[3, :3, :3] @ C.AC.rodrigues((0.0, C.MIN_R * (1.0 + 1e-6), 0.0))
    ar = C.archive(100.0, n)
    ar.integrate(depth, 0, true)
    assert ar.move(np.arange(n), new, C.MIN_T, C.MIN_R) == 2
    h = _handle()
    try:
        _volume(h, 100.0)
        h.tsdf_archive_init(capacity=n, rect=True)
        dev = _upload(depth)
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, n, first_frame=0, world_T_cam=true, stream=_stream())
        h.tsdf_archive_move(np.arange(n), new, C.MIN_T, C.MIN_R, stream=_stream())
        a = h.tsdf_archive_read()
        assert a["moved_last"] == 2
        changed = [i for i in range(n) if not np.array_equal(a["world_T_cam"][i], true[i])]
        assert changed == [1, 3]
        _same_volume(h, ar.tsdf, ar.weight)
    finally:
        h.close()


def test_refusals():
    depth, true, _ = C.sequence(6)
    h = _handle()
    try:
        with pytest.raises(RuntimeError, match="no TSDF volume"):
            h.tsdf_archive_init(capacity=4, rect=True)
        _volume(h, 100.0)
        dev = _upload(depth)
        with pytest.raises(RuntimeError, match="no depth archive"):
            h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, 1, world_T_cam=true[:1], stream=_stream())
        with pytest.raises(RuntimeError, match="no depth archive"):
            h.tsdf_archive_move([0], true[:1], C.MIN_T, C.MIN_R, stream=_stream())
        with pytest.raises(RuntimeError, match="capacity"):
            h.tsdf_archive_init(capacity=0, rect=True)
        h.tsdf_follow()
        with pytest.raises(RuntimeError, match="does not follow the window"):
            h.tsdf_archive_init(capacity=4, rect=True)
        h.tsdf_follow(enable=False)
        h.tsdf_archive_init(capacity=4, rect=True)
        with pytest.raises(RuntimeError, match="does not follow the window"):
            h.tsdf_follow()
        with pytest.raises(RuntimeError, match="min_rotation"):
            h.tsdf_archive_move([0], true[:1], C.MIN_T, 4.0, stream=_stream())
        # tslam_tsdf_write replaces what the archived frames built: the archive is off until its next init
        h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, 2, world_T_cam=true[:2], stream=_stream())
        assert h.tsdf_archive_read()["count"] == 2
        h.tsdf_write(*h.tsdf_read())
        assert h.tsdf_archive_read()["count"] == 0
        with pytest.raises(RuntimeError, match="no depth archive"):
            h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, 1, world_T_cam=true[:1], stream=_stream())
        h.tsdf_archive_init(capacity=4, rect=True)
        assert h.tsdf_archive_read()["count"] == 0
    finally:
        h.close()
    h = _handle()
    try:   # the colour layer is not moved
        h.tsdf_color(True)
        _volume(h, 100.0)
        with pytest.raises(RuntimeError, match="colour layer"):
            h.tsdf_archive_init(capacity=4, rect=True)
    finally:
        h.close()
