"""The brick store behind the rolling window on the device: ``tslam_tsdf_store_init`` / ``_stats`` /
``_read`` (``k_tsdf_store_out`` / ``k_tsdf_store_in`` around ``k_tsdf_move``) and
``HipSlamConfig.dense_store`` against tests/ref_tsdf_store.py.  Everything is bit-exact: voxels move
as 32-bit words.

Dims 37 x 13 x 41 and 40 x 13 x 41 (test_gpu_tsdf_follow.py's): off the 8-voxel store grid on every
axis, so the window's edges cut store bricks, off the integrator's 16 x 4 x 4 bricks, and 40 adds the
move's wide-vector path."""

from __future__ import annotations

import numpy as np
import pytest

import ref_tsdf_follow as REF
import ref_tsdf_store as RS
from test_gpu_tsdf_follow import DIMS, H, MAX_D, MAX_W, ORIGIN, TRUNC_VOX, VOX, W, _Cam, _pose
from thor_slam_amd import dense_store as DS
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

DIMS40 = (40, 13, 41)
PLAIN, COLOR = ("tsdf", "weight"), ("tsdf", "weight", "color_weight", "color")
STAT_KEYS = ("bricks_allocated", "bricks", "voxels_stored", "voxels_dropped", "moves", "words_per_voxel")
P0 = np.stack([_pose((0.0, 0.0, 0.0)), _pose((0.02, 0.0, 0.0))])


class _SCam(_Cam):
    """test_gpu_tsdf_follow's camera with the store on (``capacity`` None: never initialised)."""

    def __init__(self, capacity=4096, freespace=False, **kw):
        super().__init__(**kw)
        self.freespace = freespace
        if freespace:
            self.h.tsdf_freespace_init(settle_frames=3)
        if capacity is not None:
            self.h.tsdf_store_init(capacity)

    @property
    def layers(self):
        return (COLOR if self.color else PLAIN) + (("freespace",) if self.freespace else ())

    def window(self, **kw):
        return RS.StoreWindow(ORIGIN, self.dims, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W, layers=self.layers, **kw)

    def read(self):
        out = super().read()
        if self.freespace:
            out["freespace"] = self.h.tsdf_freespace_read()
        return out

    def check(self, win, msg=""):
        """The window, tsdf_window(), store_read and store_stats against the model."""
        got = self.read()
        shift, origin = self.h.tsdf_window()
        assert shift.tolist() == list(win.shift), (msg, shift, win.shift)
        np.testing.assert_array_equal(origin, np.array(win.origin), err_msg=str(msg))
        for k in self.layers:
            np.testing.assert_array_equal(got[k].view(np.uint32), win.vol[k].view(np.uint32), err_msg=f"{k} {msg}")
        bricks, words = self.h.tsdf_store_read()
        want_b, want_w = win.content()
        np.testing.assert_array_equal(bricks, want_b, err_msg=f"bricks {msg}")
        np.testing.assert_array_equal(words, want_w, err_msg=f"words {msg}")
        st, want = self.h.tsdf_store_stats(), win.stats()
        assert {k: st[k] for k in STAT_KEYS} == {k: want[k] for k in STAT_KEYS}, msg
        return st

    def both(self, win, f0, poses, msg=""):
        """One integrate call on host poses, on the device and in the model."""
        poses = np.stack(poses)
        self.integrate(f0, len(poses), poses)
        win.call(self.views(f0, poses))
        return self.check(win, msg)

    def shift(self, win, delta, msg=""):
        self.h.tsdf_shift(delta, stream=self.stream)
        win.shift_by(delta)
        return self.check(win, msg or delta)


# -- 1. out and back is the identity --------------------------------------------------------------------
@pytest.mark.parametrize("dims", [DIMS, DIMS40])
@pytest.mark.parametrize("color", [False, True])
def test_round_trip(color, dims):
    c = _SCam(n=2, color=color, dims=dims)
    win = c.window()
    try:
        c.both(win, 0, P0, "integrated")
        before = c.read()
        assert (before["weight"] > 0).sum() > 2000
        st = c.shift(win, (5, -3, 9))
        assert st["bricks"] > 8 and st["voxels_stored"] == win.left_nonzero > 500 and st["voxels_dropped"] == 0
        st = c.shift(win, (-5, 3, -9))
        after = c.read()
        for k in c.layers:
            np.testing.assert_array_equal(after[k].view(np.uint32), before[k].view(np.uint32), err_msg=k)
        bricks, words = c.h.tsdf_store_read()
        assert len(bricks) == 0 and words.shape == (0, 6 if color else 2, 8, 8, 8)
        assert st["bricks"] == 0 and st["voxels_stored"] == 0 and st["moves"] == 2 and st["capacity"] == 4096
    finally:
        c.close()


# -- 2. a sequence of moves on every axis -----------------------------------------------------------------
@pytest.mark.parametrize("color,dims", [(False, DIMS), (True, DIMS40)])
def test_multi_axis_sequence(color, dims):
    c = _SCam(n=4, color=color, dims=dims)
    win = c.window()
    big = dims[0] + 30                                # |delta| >= dim: the whole window goes out, past what the store holds
    try:
        c.both(win, 0, P0, "call 0")
        c.shift(win, (-16, 4, -4))                    # absolute x and z below zero from here on
        c.both(win, 1, [_pose((-0.7, 0.2, -0.2))], "call 1")
        c.shift(win, (3, -9, 0))                      # y below zero
        c.shift(win, (0, 0, 12))
        c.both(win, 2, [_pose((-0.6, -0.2, 0.4)), _pose((-0.6, -0.2, 0.42), (0.0, 0.03, 0.0))], "call 2")
        st = c.shift(win, (big, 0, 0))
        assert not win.words().any() and st["voxels_stored"] > 2000
        c.both(win, 3, [_pose((2.9, -0.2, 0.4))], "call 3, away")
        c.shift(win, (-big, 5, -8))
        c.both(win, 0, [_pose((-0.6, 0.0, 0.0))], "call 4, back")
        st = c.shift(win, (7, -1, 3))
        assert win.shift == [-6, -1, 3] and st["moves"] == 6 and st["voxels_dropped"] == 0
        lo = np.array(win.shift)
        assert (lo < 0).sum() >= 2 and st["bricks"] > 8 and (win.content()[0] < 0).any()
        assert (win.vol["weight"] > 0).sum() > 2000
    finally:
        c.close()


# -- 3. the follow decision on tracked device poses ----------------------------------------------------------
def test_camera_driven_following():
    n = 4
    c = _SCam(n=n, color=True, track=True)
    T, st = c.res["T_abs"][:, 0], c.res["stats"][:, 0, 0]
    used = [s == 0 or (s == 2 and f == 0) for f, s in enumerate(st)]
    assert sum(used) >= n - 1
    # the camera's voxel is (8, 6, -45): anchors that put it 5, 4 and 6 voxels off make the calls move
    anchors = [(8, 6, -45), (13, 2, -39), (8, 6, -45), (4, 11, -50)]
    win = c.window(margin=3, step=2)
    try:
        for i, anchor in enumerate(anchors):
            f0 = 2 * (i % 2)
            c.h.tsdf_follow(anchor=anchor, margin=3, step=2)      # toggling leaves the store alone
            win.anchor = anchor
            c.integrate(f0, 2)                                     # world_T_cam = NULL: the batch's device poses
            win.call(c.views(f0, T[f0:f0 + 2], used[f0:f0 + 2]))
            stats = c.check(win, f"call {i}")
    finally:
        c.close()
    print("moves", win.moves, "stats", stats)
    assert win.moves[0] == (0, 0, 0) and sum(any(d) for d in win.moves) == 3
    assert all(d[a] != 0 for d in win.moves[1:] for a in range(3))          # every move on all three axes
    assert {int(np.sign(d[a])) for d in win.moves[1:] for a in range(3)} == {-1, 1}
    assert stats["moves"] == 3 and stats["voxels_stored"] > 500


# -- 4. the free-space layer's words leave and return with the voxel ----------------------------------------
def test_freespace_layer_travels():
    c = _SCam(n=2, color=False, freespace=True)
    win = c.window()
    rng = np.random.default_rng(7)
    try:
        c.both(win, 0, P0, "integrated")
        fs = rng.integers(0, 1 << 17, size=DIMS[::-1]).astype(np.uint32)
        fs[(win.vol["weight"] == 0) & (rng.random(DIMS[::-1]) < 0.9)] = 0      # some voxels hold only a free-space word
        c.h.tsdf_freespace_write(fs)
        win.vol["freespace"] = fs.copy()
        only_fs = int(((fs != 0) & (win.vol["weight"] == 0) & (win.vol["tsdf"] == 0)).sum())
        assert only_fs > 100
        st = c.shift(win, (-6, 2, 11))
        assert st["words_per_voxel"] == 3 and st["voxels_stored"] > 1000
        assert (win.content()[1][:, 2] != 0).sum() > 100
        c.shift(win, (9, 0, -3))
        c.shift(win, (-3, -2, -8))
        assert win.shift == [0, 0, 0] and len(win.content()[0]) == 0
        np.testing.assert_array_equal(c.h.tsdf_freespace_read(), fs)
    finally:
        c.close()


# -- 5. a pool that is too small: probe collisions and overflow --------------------------------------------
def test_probe_collisions_and_overflow():
    c = _SCam(n=2, color=False, capacity=8)          # a table of 16 cells
    full = c.window()                                # the unbounded model
    try:
        c.integrate(0, 2, P0)
        full.call(c.views(0, P0))
        for delta in ((DIMS[0], 0, 0), (0, 0, 0)):    # everything leaves; a call that does not move changes nothing
            c.h.tsdf_shift(delta, stream=c.stream)
            full.shift_by(delta)
        st = c.h.tsdf_store_stats()
        print("capacity 8:", st, "unbounded:", full.stats())
        assert full.stats()["bricks"] > 8 and st["capacity"] == 8 and st["bricks_allocated"] == 8 and st["moves"] == 1
        assert st["voxels_dropped"] > 0 and st["voxels_dropped"] == full.left_nonzero - st["voxels_stored"]
        bricks, words = c.h.tsdf_store_read()
        assert 0 < len(bricks) <= 8 and bricks.tolist() == sorted(bricks.tolist(), key=lambda b: (b[2], b[1], b[0]))
        want = dict(zip(map(tuple, full.content()[0].tolist()), full.content()[1]))
        for b, brick in zip(bricks.tolist(), words):  # every stored brick is one of the model's, with exact words
            np.testing.assert_array_equal(brick, want[tuple(b)], err_msg=str(b))
        assert int(sum(w.any(axis=0).sum() for w in words)) == st["voxels_stored"]
        c.h.tsdf_shift((-DIMS[0], 0, 0), stream=c.stream)
        full.shift_by((-DIMS[0], 0, 0))
        got = c.read()
        back = np.stack([got["tsdf"].view(np.uint32), got["weight"].view(np.uint32)])
        same = (back == full.words()).all(axis=0)
        assert (same | ~back.any(axis=0)).all()      # the unbounded model's value, or zero
        assert int((~same).sum()) == st["voxels_dropped"]
        st = c.h.tsdf_store_stats()
        assert st["bricks"] == 0 and st["voxels_stored"] == 0 and st["bricks_allocated"] == 8
    finally:
        c.close()


# -- 6. lifecycle ---------------------------------------------------------------------------------------------
def test_lifecycle_and_refusals():
    from thor_slam_amd._lib import Handle
    from test_gpu_tsdf_follow import _records

    c = _SCam(n=2, color=False)
    win = c.window()
    try:
        c.both(win, 0, P0)
        c.shift(win, (6, 0, -5))
        assert c.h.tsdf_store_stats()["voxels_stored"] > 500
        c.h.reset()                                  # tslam_reset: an empty store that stays on
        st = c.h.tsdf_store_stats()
        assert st["bricks_allocated"] == 0 and st["voxels_stored"] == 0 and st["moves"] == 0 and st["capacity"] == 4096
        win = c.window()
        c.both(win, 0, P0, "after reset")
        c.shift(win, (6, 0, -5), "after reset")
        c.h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)   # a new volume: the same
        assert c.h.tsdf_store_stats()["bricks_allocated"] == 0 and len(c.h.tsdf_store_read()[0]) == 0
        win = c.window()
        c.both(win, 0, P0, "after init")
        c.shift(win, (-3, 2, 7), "after init")
        # a layer configured after store_init: refused, nothing changes
        with pytest.raises(RuntimeError, match="brick store"):
            c.h.tsdf_freespace_init(settle_frames=3)
        with pytest.raises(RuntimeError, match="brick store"):
            c.h.tsdf_archive_init(4)
        with pytest.raises(RuntimeError, match="capacity"):
            c.h.tsdf_store_init(-1)
        c.check(win, "after refused calls")
        c.h.tsdf_store_init(0)                       # freed: a move drops what leaves, as without the store
        with pytest.raises(RuntimeError, match="no brick store"):
            c.h.tsdf_store_stats()
        c.h.tsdf_freespace_init(settle_frames=3)     # and the layer may be added again
        c.h.tsdf_freespace_init(enable=False)
        plain = REF.Window(ORIGIN, DIMS, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W)
        plain.vol = {k: v.copy() for k, v in win.vol.items()}
        plain.shift = list(win.shift)
        c.h.tsdf_shift((-5, 3, 6), stream=c.stream)
        plain.shift_by((-5, 3, 6))
        _Cam.check(c, plain, "store freed")
        assert (plain.vol["weight"] > 0).sum() < (win.vol["weight"] > 0).sum()
        c.h.tsdf_archive_init(4)                     # the archive on: the store is refused
        with pytest.raises(RuntimeError, match="archive"):
            c.h.tsdf_store_init(16)
    finally:
        c.close()
    _, rect, _ = _records(False, 2)
    h = Handle([rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=2)
    try:
        with pytest.raises(RuntimeError, match="no TSDF volume"):
            h.tsdf_store_init(16)
    finally:
        h.close()


# -- 7. store off ------------------------------------------------------------------------------------------------
def test_store_off_is_the_rolling_window():
    c = _SCam(n=2, color=True, capacity=None)        # never initialised
    win = REF.Window(ORIGIN, DIMS, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W)
    try:
        c.integrate(0, 2, P0)
        win.call(c.views(0, P0))
        for delta in ((5, -3, 9), (-5, 3, -9)):
            c.h.tsdf_shift(delta, stream=c.stream)
            win.shift_by(delta)
            _Cam.check(c, win, delta)
        with pytest.raises(RuntimeError, match="no brick store"):
            c.h.tsdf_store_read()
    finally:
        c.close()


# -- 8. engine end to end ------------------------------------------------------------------------------------------
def test_engine_keeps_what_leaves():
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    n, per, anchor = 18, 6, (8, 6, -46)              # the camera travels a third of a voxel per frame in z
    src = SyntheticRGBDSource(width=W, height=H)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    kw = dict(rgbd=True, dense_map=True, dense_follow=True, dense_follow_step=1, dense_follow_margin=1, batch_size=per,
              dense_follow_anchor=anchor, n_features=1000, n_levels=3, tsdf_origin=ORIGIN, tsdf_dims=DIMS, voxel_size=VOX,
              tsdf_integrator_max_integration_distance_m=MAX_D, tsdf_max_weight=MAX_W)
    eng = HipSlamEngine(num_cameras=2, config=HipSlamConfig(dense_store=True, dense_store_bricks=4096, **kw))
    eng.initialize(rig.calibration)
    rect = eng.rectifications[0]
    win = RS.StoreWindow(ORIGIN, DIMS, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W, layers=COLOR, anchor=anchor, margin=1, step=1)
    lo, hi = (-8, -8, -8), tuple(d + 16 for d in DIMS)
    try:
        for g0 in range(0, n, per):
            views = []
            for _ in range(per):
                fs = rig.get_synchronized_frames()
                views.append({"depth": np.array(fs.frame_sets[src.name].frames[1].image),
                              "bgr": np.array(fs.frame_sets[src.name].frames[0].image),
                              "intr": (rect.fx, rect.fy, rect.cx, rect.cy), "map": None if rect.is_identity else rect.map_left})
                eng.process_frames(fs)
            eng.flush()
            res = eng.handle.read_poses(per)
            for k, v in enumerate(views):
                s = int(res["stats"][k, 0, 0])
                v["cTw"] = REF.cam_T_world(res["T_abs"][k, 0])
                v["used"] = s == 0 or (s == 2 and g0 + k == 0)
            win.call(views)
            dm, st = eng.get_dense_map(), eng.get_dense_store()
            assert dm["window_shift"].tolist() == win.shift, (g0, win.moves)
            want_b, want_w = win.content()
            np.testing.assert_array_equal(st["bricks"], want_b)
            assert st["tsdf"].shape == (len(want_b), 8, 8, 8) and st["color"].shape == (len(want_b), 8, 8, 8, 3)
            assert {k: st["stats"][k] for k in STAT_KEYS} == {k: win.stats()[k] for k in STAT_KEYS}
            assert st["origin"].tolist() == list(ORIGIN) and st["voxel_size"] == VOX
            np.testing.assert_array_equal(st["world_T_volume"], dm["world_T_volume"])
            got, want = DS.assemble(dm, st, lo, hi), win.assemble(lo, hi)
            for k in COLOR:
                np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=f"{k} batch at {g0}")
        print("moves", win.moves, "stats", st["stats"])
        assert sum(any(d) for d in win.moves) >= 2 and st["stats"]["voxels_stored"] > 500
        assert all(abs(k) < 8 for k in win.shift)
        eng.reset()
        assert len(eng.get_dense_store()["bricks"]) == 0 and eng.get_dense_store()["stats"]["moves"] == 0
    finally:
        eng.shutdown()
    off = HipSlamEngine(num_cameras=2, config=HipSlamConfig(**kw))
    off.initialize(rig.calibration)
    try:
        assert off.get_dense_store() is None
    finally:
        off.shutdown()
