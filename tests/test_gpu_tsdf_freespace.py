"""The free-space layer on the device: ``tslam_tsdf_freespace_init`` / ``_read`` / ``_write``
(``k_tsdf_freespace.hip``), ``tslam_tsdf_dynamic`` with the layer on (``k_tsdf_dynamic.hip``), the
rolling window's move of the layer, and ``HipSlamConfig(dense_dynamic_settle_frames=...)`` against
tests/ref_tsdf_freespace.py.

Layer, mask, depth, stats and volume are equal to the reference's bit for bit: the same IEEE f64
operations in the same order and integer words, and a scene is used only after the guards have shown
that none of its voxels or pixels sits on a gate (tests/tsdf_freespace_cases.py).  Helpers and the
RGB-D records are those of tests/test_gpu_tsdf_dynamic.py."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import ref_tsdf_dynamic as REF
import ref_tsdf_freespace as RF
import test_gpu_tsdf_dynamic as G
import tsdf_dynamic_cases as C
import tsdf_freespace_cases as F
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

RW, RH, HW = G.RW, G.RH, G.HW


def _run(h, frames, poses, cam, n=None):
    """One tslam_tsdf_dynamic call of the frames on host poses; the slots read back."""
    W, H = cam[:2]
    dev = G._upload(frames)
    n = len(frames) if n is None else n
    h.tsdf_dynamic(dev.data_ptr(), 2 * W * H, n, world_T_cam=np.asarray(poses), stream=G._stream())
    return [h.tsdf_dynamic_read(f) for f in range(n)]


def _shifted(a, delta):
    """a [nz][ny][nx] moved as the window moves a layer: out(i, j, k) = a(i + dx, j + dy, k + dz), zeros entering."""
    out = np.zeros_like(a)
    nz, ny, nx = a.shape
    dx, dy, dz = delta
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    ok = (i + dx >= 0) & (i + dx < nx) & (j + dy >= 0) & (j + dy < ny) & (k + dz >= 0) & (k + dz < nz)
    out[ok] = a[(k + dz)[ok], (j + dy)[ok], (i + dx)[ok]]
    return out


# -- 1. the layer after a call, word for word ---------------------------------------------------------------
@pytest.mark.parametrize("cam", [C.CAM, C.CAM2], ids=["67x77", "131x69"])
def test_layer_after_a_call(cam):
    frames, poses, obj, gap = F.call(cam)
    ref = F.call_reference(cam, 2)
    start = F.start_layer(2)
    h = G._analytic_handle(cam)
    try:
        G._volume(h)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=6, **C.PRM)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        assert not h.tsdf_freespace_read().any()                      # a new layer is all zero
        h.tsdf_freespace_write(start)
        np.testing.assert_array_equal(h.tsdf_freespace_read(), start)
        got = _run(h, frames, poses, cam)
        words = h.tsdf_freespace_read()
        diff = int((words != ref["words"]).sum())
        print(cam[:2], "words changed by the call", int((ref["words"] != start).sum()), "differing from the reference", diff,
              "nearest |sdf| to a gate", gap)
        assert words.dtype == np.uint32 and diff == 0
        np.testing.assert_array_equal(words, ref["words"])
        for f in range(6):
            G._same(got[f], {k: ref[k][f] for k in ("mask", "depth", "stats")}, f"frame {f}")
        # the same frames in another order leave another layer: the kernel walks them in order
        h.tsdf_freespace_write(start)
        _run(h, frames[list(F.PERMUTED)], poses[list(F.PERMUTED)], cam)
        other = h.tsdf_freespace_read()
        want = RF.update(start, C.ORIGIN, C.S, cam, frames[list(F.PERMUTED)], poses[list(F.PERMUTED)], C.MAX_D, F.BAND, 2)
        np.testing.assert_array_equal(other, want)
        assert not np.array_equal(other, words)
    finally:
        h.close()


# -- 2. classification uses the layer as found ---------------------------------------------------------------
def test_classification_uses_the_layer_as_found():
    cam = C.CAM2                                                       # the camera on which the preset words leave a mask
    frames, poses, obj, _ = F.call(cam)
    ref = F.call_reference(cam, 2)
    t, w = C.volume()
    h = G._analytic_handle(cam)
    try:
        G._volume(h)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=6, **C.PRM)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        # preset settled words: candidates go, and mask, depth and stats follow the reference
        h.tsdf_freespace_write(F.start_layer(2))
        got = _run(h, frames, poses, cam)
        plain = C.reference(frames[0], cam=cam)
        assert 0 < ref["stats"][0, 2] < plain["stats"][2] and ref["mask"][0].any()
        for f in range(6):
            G._same(got[f], {k: ref[k][f] for k in ("mask", "depth", "stats")}, f"preset layer, frame {f}")
        # a call whose first frames settle the ball: its later frames are still masked, the next call is not
        h.tsdf_freespace_write(np.zeros(F.SHAPE, np.uint32))
        three, at = np.stack([frames[0]] * 3), np.stack([C.T_STAR] * 3)
        first = RF.dynamic(t, w, np.zeros(F.SHAPE, np.uint32), C.ORIGIN, C.S, C.TRUNC, cam, three, at, 2, F.BAND_VOX, max_dist=C.MAX_D,
                           **C.PRM)
        second = RF.dynamic(t, w, first["words"], C.ORIGIN, C.S, C.TRUNC, cam, three[:1], at[:1], 2, F.BAND_VOX, max_dist=C.MAX_D,
                            **C.PRM)
        got = _run(h, three, at, cam)
        for f in range(3):
            G._same(got[f], {k: first[k][f] for k in ("mask", "depth", "stats")}, f"settling call, frame {f}")
            assert got[f]["mask"][obj].all() and got[f]["stats"][2] == obj.sum()
        np.testing.assert_array_equal(h.tsdf_freespace_read(), first["words"])
        assert (first["words"][F.ball_voxels()] & RF.SETTLED_BIT).any()
        nxt = _run(h, three[:1], at[:1], cam)[0]
        G._same(nxt, {k: second[k][0] for k in ("mask", "depth", "stats")}, "the next call")
        print("object pixels", int(obj.sum()), "masked in the settling call", [int(g["mask"][obj].sum()) for g in got],
              "in the next call", int(nxt["mask"][obj].sum()), "candidates", int(nxt["stats"][2]))
        assert not nxt["mask"][obj].any()
    finally:
        h.close()


# -- 3. the resting object ------------------------------------------------------------------------------------
def test_resting_object():
    cam = C.CAM
    W, H = cam[:2]
    steps, frames, obj, gap = F.chain_reference()
    ball = F.ball_voxels()
    t0, w0 = C.volume()
    h = G._analytic_handle(cam)
    try:
        G._volume(h)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)                     # the default radii
        h.tsdf_freespace_init(settle_frames=F.CHAIN_SETTLE, occupied_band_vox=F.BAND_VOX)
        s = G._stream()
        dev = {k: G._upload(v) for k, v in frames.items()}
        for c, name in enumerate(F.CHAIN):
            h.tsdf_dynamic(dev[name].data_ptr(), 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=s)
            h.tsdf_integrate_rect(h.tsdf_dynamic_buffers()[0]["depth"], 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=s)
            got, words, (t, w) = h.tsdf_dynamic_read(0), h.tsdf_freespace_read(), h.tsdf_read()
            st = steps[c]
            changed = int(((t != t0) | (w != w0))[ball].sum())
            print("call", c, name, "object pixels masked", int(got["mask"][obj].sum()), "of", int(obj.sum()), "ball voxels changed",
                  changed, "of", int(ball.sum()), "settled", int((words[ball] & RF.SETTLED_BIT != 0).sum()))
            G._same(got, st, f"call {c}")
            np.testing.assert_array_equal(words, st["words"], err_msg=f"layer after call {c}")
            np.testing.assert_array_equal(w, st["weight"], err_msg=f"weight after call {c}")
            np.testing.assert_array_equal(t.view(np.uint32), st["tsdf"].view(np.uint32), err_msg=f"tsdf after call {c}")
            if c < 3:
                assert got["mask"][obj].all() and changed == 0
            if c == 3:
                assert not got["mask"][obj].any() and changed == 56     # the count tests/test_tsdf_freespace_cpu.py derives
        gone = h.tsdf_freespace_read()
        assert (steps[4]["words"][ball] & RF.SETTLED_BIT).any() and not (gone[ball] & RF.SETTLED_BIT).any()
    finally:
        h.close()


# -- 4. the shifted window ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True], ids=["plain", "with the colour layer"])
def test_shifted_window(color):
    cam = C.CAM
    frames, poses, obj, _ = F.call(cam)
    start = F.start_layer(2)
    delta = (3, -1, 2)
    h = G._analytic_handle(cam)
    try:
        if color:
            h.tsdf_color(True)
        G._volume(h)
        if color:
            rgb = np.random.default_rng(5).uniform(0, 255, (*F.SHAPE, 3)).astype(np.float32)
            h.tsdf_write_color(rgb, C.volume()[1])
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=1, **C.PRM)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)     # before the window's record exists
        h.tsdf_freespace_write(start)
        h.tsdf_shift(delta, stream=G._stream())
        shift, origin = h.tsdf_window()
        assert shift.tolist() == list(delta)
        moved = h.tsdf_freespace_read()
        np.testing.assert_array_equal(moved, _shifted(start, delta))
        assert (moved == 0).sum() > (start == 0).sum()
        t2, w2 = h.tsdf_read()
        np.testing.assert_array_equal(w2, _shifted(C.volume()[1], delta))
        if color:
            c2, cw2 = h.tsdf_read_color()
            np.testing.assert_array_equal(c2, np.stack([_shifted(rgb[..., ch], delta) for ch in range(3)], axis=-1))
        # an update sees the volume at its effective origin
        F.guard(cam, frames[0], C.T_STAR, origin=tuple(origin), vol=(t2, w2))
        ref = RF.dynamic(t2, w2, moved, tuple(origin), C.S, C.TRUNC, cam, frames[:1], poses[:1], 2, F.BAND_VOX, max_dist=C.MAX_D, **C.PRM)
        stale = RF.update(moved, C.ORIGIN, C.S, cam, frames[:1], poses[:1], C.MAX_D, F.BAND, 2)
        assert not np.array_equal(stale, ref["words"])
        got = _run(h, frames[:1], poses[:1], cam)[0]
        G._same(got, {k: ref[k][0] for k in ("mask", "depth", "stats")}, "shifted window")
        np.testing.assert_array_equal(h.tsdf_freespace_read(), ref["words"])
        # a layer made while the record exists moves too (the move's scratch has grown)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        h.tsdf_freespace_write(start)
        h.tsdf_shift((-4, 0, 0), stream=G._stream())
        np.testing.assert_array_equal(h.tsdf_freespace_read(), _shifted(start, (-4, 0, 0)))
    finally:
        h.close()


# -- 5. the undistortion-table path, device and host poses -------------------------------------------------------
def test_rgbd_table_path_device_and_host_poses():
    import torch

    from thor_slam_amd._lib import Handle

    n = 4
    rect, rec = G._records(n)
    assert not rect.is_identity
    cam = (RW, RH, rect.fx, rect.fy, rect.cx, rect.cy)
    dims = tuple(G.ROOM_DIMS)
    cfg = HipSlamConfig(rgbd=True, n_features=1000, n_levels=3)
    prm = {**C.PRM, "min_free_weight": 1.5}
    # frame 0 sits on the identity pose: voxel centres and the room's back wall are whole millimetres
    # apart, so a band of whole millimetres (1.5 voxels = 75 mm) has voxels exactly on its gates and
    # the guard refuses the scene; 1.37 voxels = 68.5 mm lies half a millimetre from every such voxel
    band_vox = 1.37
    band = band_vox * C.S
    h = Handle([rect], cfg, max_batch=n)
    fresh = Handle([rect], cfg, max_batch=2)
    try:
        dev = torch.from_numpy(rec.copy()).cuda()
        s = G._stream()
        h.submit(dev.data_ptr(), n, s)
        res = h.read_poses(n)
        T, st = res["T_abs"][:, 0], res["stats"][:, 0, 0]
        used = [bool(s_ == 0 or (s_ == 2 and f == 0)) for f, s_ in enumerate(st)]
        assert sum(used) >= 3 and used[3]
        depth_ptr, stride = dev.data_ptr() + 3 * HW, 5 * HW
        h.tsdf_init(G.ROOM_ORIGIN, G.ROOM_DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        h.tsdf_integrate(depth_ptr, stride, 3, first_frame=0, stream=s)
        tsdf, weight = h.tsdf_read()
        depth = np.stack([rec[f, 0, 3 * HW:].view(np.uint16).reshape(RH, RW) for f in range(n)])
        tracked = np.stack([T[f] if used[f] else C.NAN for f in range(n)])
        for f in range(n):
            if used[f]:
                ok, gap = RF.guarded(dims, G.ROOM_ORIGIN, C.S, cam, depth[f], tracked[f], C.MAX_D, band, rect.map_left)
                assert ok, (f, gap)
        zero = np.zeros(dims[::-1], np.uint32)
        ref = RF.dynamic(tsdf, weight, zero, G.ROOM_ORIGIN, C.S, C.TRUNC, cam, depth, tracked, 2, band_vox, max_dist=C.MAX_D,
                         table=rect.map_left, **prm)
        plain = RF.update(zero, G.ROOM_ORIGIN, C.S, cam, depth, tracked, C.MAX_D, band, 2)      # without the table
        r, sd = RF.unpack(ref["words"])
        print("table path: runs", np.bincount(r.ravel())[:6].tolist(), "settled", int(sd.sum()), "differ without the table",
              int((plain != ref["words"]).sum()))
        assert sd.sum() > 1000 and (plain != ref["words"]).any()
        h.tsdf_dynamic_init(pair=0, rect=False, max_frames=n, **prm)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=band_vox)
        # from NULL: the batch's device poses
        h.tsdf_dynamic(depth_ptr, stride, n, first_frame=0, stream=s)
        for f in range(n):
            G._same(h.tsdf_dynamic_read(f), {k: ref[k][f] for k in ("mask", "depth", "stats")}, f"device poses, frame {f}")
        np.testing.assert_array_equal(h.tsdf_freespace_read(), ref["words"])
        # from the same poses on the host, on a new layer
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=band_vox)
        h.tsdf_dynamic(depth_ptr, stride, n, world_T_cam=tracked, stream=s)
        np.testing.assert_array_equal(h.tsdf_freespace_read(), ref["words"])
        # an untracked frame leaves the layer alone
        blank = torch.zeros((2, 1, 5 * HW), dtype=torch.uint8, device="cuda")
        fresh.submit(blank.data_ptr(), 2, s)
        assert fresh.read_poses(2)["stats"][1, 0, 0] != 0
        fresh.tsdf_init(G.ROOM_ORIGIN, G.ROOM_DIMS, C.S, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
        fresh.tsdf_write(tsdf, weight)
        fresh.tsdf_dynamic_init(pair=0, rect=False, max_frames=1, **prm)
        fresh.tsdf_freespace_init(settle_frames=2, occupied_band_vox=band_vox)
        fresh.tsdf_freespace_write(ref["words"])
        fresh.tsdf_dynamic(depth_ptr + 3 * stride, stride, 1, first_frame=1, stream=s)
        assert fresh.tsdf_dynamic_read(0)["stats"].tolist() == [REF.UNUSED, 0, 0, 0]
        np.testing.assert_array_equal(fresh.tsdf_freespace_read(), ref["words"])
    finally:
        h.close()
        fresh.close()


# -- 6. off means off ---------------------------------------------------------------------------------------------
def test_off_means_off():
    cam = C.CAM2
    frames, poses, obj, _ = F.call(cam)
    t, w = C.volume()
    today = REF.dynamic(t, w, C.ORIGIN, C.S, C.TRUNC, cam, frames, poses, max_dist=C.MAX_D, **C.PRM)
    assert not np.array_equal(today["mask"], F.call_reference(cam, 2)["mask"])            # the layer would have shown
    never, was_on = G._analytic_handle(cam), G._analytic_handle(cam)
    try:
        for h in (never, was_on):
            G._volume(h)
            h.tsdf_dynamic_init(pair=0, rect=True, max_frames=6, **C.PRM)
        was_on.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        was_on.tsdf_freespace_write(F.start_layer(2))
        was_on.tsdf_freespace_init(enable=False)
        for name, h in (("never on", never), ("switched off", was_on)):
            got = _run(h, frames, poses, cam)
            for f in range(6):
                G._same(got[f], {k: today[k][f] for k in ("mask", "depth", "stats")}, f"{name}, frame {f}")
            with pytest.raises(RuntimeError, match="tslam error -4.*freespace_init"):
                h.tsdf_freespace_read()
    finally:
        never.close()
        was_on.close()


# -- 7. refusals and the life cycle ---------------------------------------------------------------------------------
def test_refusals_and_life_cycle():
    import torch

    from thor_slam_amd._lib import TsdfFreespaceParams

    cam = C.CAM
    W, H = cam[:2]
    frames, poses, obj, _ = F.call(cam)
    start = F.start_layer(2)
    h = G._analytic_handle(cam)

    def after_two_sphere_frames():
        """Two sphere frames from a zero layer settle the ball at settle_frames 2 and at no larger setting."""
        h.tsdf_freespace_write(np.zeros(F.SHAPE, np.uint32))
        _run(h, frames[:2], poses[:2], cam)
        return h.tsdf_freespace_read()

    try:
        # without a volume
        for call in (lambda: h.tsdf_freespace_init(settle_frames=2), lambda: h.tsdf_freespace_init(enable=False),
                     lambda: h.tsdf_freespace_read(), lambda: h.tsdf_freespace_write(start)):
            with pytest.raises(RuntimeError, match="tslam error -4.*tsdf_init"):
                call()
        G._volume(h)
        # without the layer
        for call in (lambda: h.tsdf_freespace_read(), lambda: h.tsdf_freespace_write(start)):
            with pytest.raises(RuntimeError, match="tslam error -4.*freespace_init"):
                call()
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=2, **C.PRM)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        want = RF.update(np.zeros(F.SHAPE, np.uint32), C.ORIGIN, C.S, cam, frames[:2], poses[:2], C.MAX_D, F.BAND, 2)
        np.testing.assert_array_equal(after_two_sphere_frames(), want)
        h.tsdf_freespace_write(start)
        # out-of-range and non-finite parameters, a non-zero reserved
        for bad in (dict(settle_frames=0), dict(settle_frames=-1), dict(settle_frames=65536), dict(occupied_band_vox=0.0),
                    dict(occupied_band_vox=-1.0), dict(occupied_band_vox=float("nan")), dict(occupied_band_vox=float("inf")),
                    dict(occupied_band_vox=C.TRUNC_VOX * (1 + 1e-12))):
            with pytest.raises(RuntimeError, match="tslam error -1.*(settle_frames|occupied_band_vox)"):
                h.tsdf_freespace_init(**{"settle_frames": 5, "occupied_band_vox": 1.0, **bad})
        for slot in range(5):
            res = (ctypes.c_int32 * 5)()
            res[slot] = 1
            prm = TsdfFreespaceParams(1.0, 5, res)
            assert h.lib.tslam_tsdf_freespace_init(h.h, ctypes.addressof(prm)) == -1 and b"reserved" in h.lib.tslam_last_error()
        assert ctypes.sizeof(TsdfFreespaceParams) == 32
        # a word with a bit above 16
        bad = start.copy()
        bad[-1, -1, -1] |= 1 << 17
        with pytest.raises(RuntimeError, match="tslam error -1.*above 16"):
            h.tsdf_freespace_write(bad)
        assert h.lib.tslam_tsdf_freespace_write(h.h, None) == -1
        assert h.lib.tslam_tsdf_freespace_read(h.h, None) == 0
        with pytest.raises(ValueError):
            h.tsdf_freespace_write(start[:-1])
        # inside a batch (nothing is launched)
        img = torch.zeros((1, 2, W * H), dtype=torch.uint8, device="cuda")
        h.begin_batch(img.data_ptr(), 1)
        for call in (lambda: h.tsdf_freespace_init(settle_frames=5), lambda: h.tsdf_freespace_init(enable=False),
                     lambda: h.tsdf_freespace_read(), lambda: h.tsdf_freespace_write(np.zeros(F.SHAPE, np.uint32))):
            with pytest.raises(RuntimeError, match="tslam error -4.*inside a batch"):
                call()
        h.end_batch()
        # every refusal left the layer and its parameters as they were
        np.testing.assert_array_equal(h.tsdf_freespace_read(), start)
        np.testing.assert_array_equal(after_two_sphere_frames(), want)
        # the upper bound itself is allowed, and a new init gives a new, zero layer with the new parameters
        h.tsdf_freespace_write(start)
        h.tsdf_freespace_init(settle_frames=65535, occupied_band_vox=C.TRUNC_VOX)
        assert not h.tsdf_freespace_read().any()
        wide = RF.update(np.zeros(F.SHAPE, np.uint32), C.ORIGIN, C.S, cam, frames[:2], poses[:2], C.MAX_D, C.TRUNC_VOX * C.S, 65535)
        got = after_two_sphere_frames()
        if RF.guarded(F.DIMS, C.ORIGIN, C.S, cam, frames[0], poses[0], C.MAX_D, C.TRUNC_VOX * C.S)[0]:
            np.testing.assert_array_equal(got, wide)
        assert not (got & RF.SETTLED_BIT).any() and (got == 2).any()
        # tslam_tsdf_write does not touch the layer; tslam_reset zeroes it as it zeroes the volume
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        h.tsdf_freespace_write(start)
        h.tsdf_write(*C.uniform_volume())
        np.testing.assert_array_equal(h.tsdf_freespace_read(), start)
        h.reset()
        assert not h.tsdf_freespace_read().any() and not h.tsdf_read()[1].any()
        h.tsdf_write(*C.volume())
        np.testing.assert_array_equal(after_two_sphere_frames(), want)             # the state stayed, and works
        # the follow decision moves the layer with the volume
        h.tsdf_freespace_write(start)
        at = np.floor((C.T_STAR[:3, 3] - np.array(C.ORIGIN)) / C.S).astype(int)   # the camera's voxel: (19, 13, -19)
        h.tsdf_follow(anchor=(int(at[0]) - 2, int(at[1]), int(at[2])), margin=1, step=1)
        blank = G._upload(np.zeros((H, W), np.uint16))                              # integrates nothing: the move alone
        h.tsdf_integrate_rect(blank.data_ptr(), 2 * W * H, 1, world_T_cam=C.T_STAR[None], stream=G._stream())
        shift, _ = h.tsdf_window()
        assert shift.tolist() == [2, 0, 0]
        np.testing.assert_array_equal(h.tsdf_freespace_read(), _shifted(start, tuple(int(d) for d in shift)))
        # tslam_tsdf_init frees it
        G._volume(h)
        with pytest.raises(RuntimeError, match="tslam error -4.*freespace_init"):
            h.tsdf_freespace_read()
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=2, **C.PRM)
        h.tsdf_freespace_init(settle_frames=2, occupied_band_vox=F.BAND_VOX)
        np.testing.assert_array_equal(after_two_sphere_frames(), want)             # a new layer on the new volume
        # NULL params frees it
        h.tsdf_freespace_init(enable=False)
        with pytest.raises(RuntimeError, match="tslam error -4.*freespace_init"):
            h.tsdf_freespace_write(start)
    finally:
        h.close()


# -- 8. the engine end to end -----------------------------------------------------------------------------------------
SETTLE, BATCHES = 3, 4
ENGINE = dict(G.ENGINE, dense_dynamic_settle_frames=SETTLE, dense_dynamic_band_vox=F.BAND_VOX)
CENTRE = (slice(115, 125), slice(140, 160))          # well inside the object of the records (rows 100..140, columns 120..180)


def _check_engine(eng_out, want, fs, dm, cfg):
    newest, t, w, words = want
    G._same(eng_out, newest, "newest frame")
    assert (w > 0).sum() > 10000
    np.testing.assert_array_equal(dm["weight"], w)
    np.testing.assert_array_equal(dm["tsdf"].view(np.uint32), t.view(np.uint32))
    assert sorted(fs) == ["origin", "run", "settled", "window_shift", "world_T_volume"]
    assert fs["run"].dtype == np.uint16 and fs["settled"].dtype == bool
    np.testing.assert_array_equal(fs["run"], (words & 0xFFFF).astype(np.uint16))
    np.testing.assert_array_equal(fs["settled"], (words >> 16) == 1)
    np.testing.assert_array_equal(fs["origin"], dm["origin"])
    np.testing.assert_array_equal(fs["window_shift"], dm["window_shift"])
    np.testing.assert_array_equal(fs["world_T_volume"], dm["world_T_volume"])
    assert fs["settled"].sum() > 1000


def test_engine_rgbd():
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    n = 3 * BATCHES
    _, rec = G._records(n, distorted=False)                          # the object is there from frame 3 on
    src = SyntheticRGBDSource(width=RW, height=RH)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    cfg = HipSlamConfig(rgbd=True, dense_color=False, **ENGINE)
    off = HipSlamEngine(num_cameras=2, config=HipSlamConfig(rgbd=True, dense_color=False, **G.ENGINE))
    off.initialize(rig.calibration)
    try:
        assert off.get_freespace() is None                           # None unless the option is on
    finally:
        off.shutdown()
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    stamps = [0.1 * f for f in range(n)]
    masks = []
    try:
        assert not eng.get_freespace()["settled"].any()
        for b in range(BATCHES):
            eng.process_batch(torch.from_numpy(rec[3 * b:3 * b + 3].copy()).cuda(), timestamps=stamps[3 * b:3 * b + 3])
            masks.append(eng.get_dynamic_mask())
        dm, fs = eng.get_dense_map(), eng.get_freespace()
        rect = eng.rectifications[0]
    finally:
        eng.shutdown()
    centre = [int(m["mask"][CENTRE].sum()) for m in masks]
    print("engine, RGB-D: masked pixels of the object's centre, newest frame of every batch", centre, "stats",
          [m["stats"].tolist() for m in masks])
    assert centre[1] == 200 and centre[-1] == 0                      # masked when it appears, released once it has rested
    h = Handle([rect], cfg, max_batch=3)
    try:
        s = G._stream()
        h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                    cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
        h.tsdf_dynamic_init(pair=0, rect=False, max_frames=3, **cfg.dense_dynamic_params())
        h.tsdf_freespace_init(settle_frames=SETTLE, occupied_band_vox=F.BAND_VOX)
        for b in range(BATCHES):
            dev = torch.from_numpy(rec[3 * b:3 * b + 3].copy()).cuda()
            h.submit(dev.data_ptr(), 3, s)
            h.tsdf_dynamic(dev.data_ptr() + 3 * HW, 5 * HW, 3, first_frame=3 * b, stream=s)
            h.tsdf_integrate_rect(h.tsdf_dynamic_buffers()[0]["depth"], 2 * HW, 3, first_frame=3 * b, stream=s)
        want = (h.tsdf_dynamic_read(2), *h.tsdf_read(), h.tsdf_freespace_read())
    finally:
        h.close()
    _check_engine(masks[-1], want, fs, dm, cfg)


def _with_patch(seq):
    """The stereo frames with a textured square at disparity 10 (1.44 m) from frame 3 on: rows 100..140,
    columns 120..180 of the left image, 110..170 of the right one."""
    out = seq.copy()
    tex = np.random.default_rng(11).integers(0, 256, (40, 60), dtype=np.uint8)
    out[3:, 0, 100:140, 120:180] = tex
    out[3:, 1, 100:140, 110:170] = tex
    return out


def test_engine_stereo_depth():
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticStereoSource

    n = 3 * BATCHES
    src = SyntheticStereoSource(width=RW, height=RH)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    seq = _with_patch(np.ascontiguousarray(src.render_stereo_sequence(n)))
    cfg = HipSlamConfig(stereo_depth=True, max_disparity=48, **ENGINE)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    stamps = [0.1 * f for f in range(n)]
    masks = []
    try:
        for b in range(BATCHES):
            eng.process_batch(torch.from_numpy(seq[3 * b:3 * b + 3].copy()).cuda(), timestamps=stamps[3 * b:3 * b + 3])
            masks.append(eng.get_dynamic_mask())
        dm, fs = eng.get_dense_map(), eng.get_freespace()
    finally:
        eng.shutdown()
    centre = [int(m["mask"][CENTRE].sum()) for m in masks]
    print("engine, stereo: masked pixels of the patch's centre, newest frame of every batch", centre, "stats",
          [m["stats"].tolist() for m in masks])
    assert centre[1] == 200 and centre[-1] == 0                      # masked when it appears, released once it has rested
    cams = extract_cameras(rig.calibration, 2)
    (li, ri), = stereo_pairs(cams)
    h = Handle([stereo_rectify(cams[li], cams[ri])], cfg, max_batch=3)
    try:
        s = G._stream()
        h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                    cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
        h.tsdf_dynamic_init(pair=0, rect=True, max_frames=3, **cfg.dense_dynamic_params())
        h.tsdf_freespace_init(settle_frames=SETTLE, occupied_band_vox=F.BAND_VOX)
        h.stereo_depth_init(max_frames=3, uniqueness=cfg.stereo_depth_uniqueness, lr_tol=cfg.stereo_depth_lr_tol)
        depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
        for b in range(BATCHES):
            dev = torch.from_numpy(seq[3 * b:3 * b + 3].copy()).cuda()
            h.submit(dev.data_ptr(), 3, s)
            h.stereo_depth(3 * b, 3, pair=0, stream=s)
            h.tsdf_dynamic(depth_ptr, frame_bytes, 3, first_frame=3 * b, stream=s)
            h.tsdf_integrate_rect(h.tsdf_dynamic_buffers()[0]["depth"], 2 * HW, 3, first_frame=3 * b, stream=s)
        want = (h.tsdf_dynamic_read(2), *h.tsdf_read(), h.tsdf_freespace_read())
    finally:
        h.close()
    _check_engine(masks[-1], want, fs, dm, cfg)
