"""The dense map's rolling window on the device: ``tslam_tsdf_follow`` / ``tslam_tsdf_shift`` /
``tslam_tsdf_window`` (``k_tsdf_follow``, ``k_tsdf_shift``, ``k_tsdf_move`` and the effective origin
in ``k_tsdf_integrate``) and ``HipSlamConfig.dense_follow`` against tests/ref_tsdf_follow.py.
Everything is bit-exact: the same IEEE f64 operations in the same order, whole-voxel moves.

Dims 37 x 13 x 41 are off every multiple of the 16 x 4 x 4 brick and of 4 (tail rows, the scalar
path of the move, the brick clamp); 40 x 13 x 41 adds the move's wide-vector path (rows of 40 and
120 floats, x moves that are multiples of 4 voxels, and x moves that are not)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

import ref_tsdf_follow as REF
import ref_tsdf_rig as RIG
import tsdf_rig_cases as C
from helpers import DISTORTION
from oracle import numpy_dense as DN
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

W, H = 320, 240
HW = W * H
DIMS = (37, 13, 41)
VOX, TRUNC_VOX, MAX_D, MAX_W = 0.05, 4.0, 10.0, 100.0
# rect world (frame-0 camera, RDF): the room's back wall and the box on the right, 2.2 .. 4.3 m ahead.
# The camera's voxel is (8, 6, -45), half a voxel from every voxel border.
ORIGIN = (-0.425, -0.325, 2.225)
KEYS = ("weight", "tsdf", "color_weight", "color")


@functools.lru_cache(maxsize=2)
def _records(distorted: bool, n: int):
    """(source, product undistortion, records [n][1][5HW]) of the synthetic RGB-D camera."""
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=W, height=H, distortion=DISTORTION if distorted else None)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rec = np.ascontiguousarray(src.render_rgbd_sequence(n)[:, None, :])
    rec.setflags(write=False)
    return src, rgbd_undistort(cams[ci]), rec


class _Cam:
    """A handle on one RGB-D camera with n rendered frames on the device."""

    def __init__(self, distorted=False, n=4, color=False, dims=DIMS, track=False):
        import torch

        from thor_slam_amd._lib import Handle

        _, self.rect, rec = _records(distorted, n)
        self.h = Handle([self.rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=n)
        self.dev = torch.from_numpy(rec.copy()).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.depth = [rec[f, 0, 3 * HW:].view(np.uint16).reshape(H, W) for f in range(n)]
        self.bgr = [rec[f, 0, :3 * HW].reshape(H, W, 3) for f in range(n)]
        self.color, self.dims = color, dims
        self.res = None
        if track:
            self.h.submit(self.dev.data_ptr(), n, self.stream)
            self.res = self.h.read_poses(n)
        if color:
            self.h.tsdf_color(True)
        self.h.tsdf_init(ORIGIN, dims, VOX, TRUNC_VOX, MAX_D, MAX_W)

    def window(self, **kw):
        return REF.Window(ORIGIN, self.dims, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W, **kw)

    def integrate(self, f0, n, poses=None, color=None):
        """Frames f0 .. f0 + n - 1 of the records: host poses, or the tracked device poses."""
        base = self.dev.data_ptr() + f0 * 5 * HW
        kw = dict(world_T_cam=poses) if poses is not None else dict(first_frame=f0)
        if self.color if color is None else color:
            self.h.tsdf_integrate_rgbd(base, base + 3 * HW, 5 * HW, n, stream=self.stream, **kw)
        else:
            self.h.tsdf_integrate(base + 3 * HW, 5 * HW, n, stream=self.stream, **kw)

    def views(self, f0, poses, used=None, color=None):
        color = self.color if color is None else color
        used = [bool(np.isfinite(T[0, 0])) for T in poses] if used is None else used
        return [{"cTw": REF.cam_T_world(np.asarray(T, float)), "used": bool(u), "depth": self.depth[f0 + i],
                 "intr": (self.rect.fx, self.rect.fy, self.rect.cx, self.rect.cy),
                 "map": None if self.rect.is_identity else self.rect.map_left, "bgr": self.bgr[f0 + i] if color else None}
                for i, (T, u) in enumerate(zip(poses, used))]

    def read(self):
        t, w = self.h.tsdf_read()
        out = {"tsdf": t, "weight": w}
        if self.color:
            out["color"], out["color_weight"] = self.h.tsdf_read_color()
        return out

    def check(self, win, msg=""):
        got = self.read()
        shift, origin = self.h.tsdf_window()
        assert shift.tolist() == list(win.shift), (msg, shift, win.shift)
        np.testing.assert_array_equal(origin, np.array(win.origin), err_msg=str(msg))
        for k in KEYS:
            if k in got:
                np.testing.assert_array_equal(got[k], win.vol[k], err_msg=f"{k} {msg}")

    def close(self):
        self.h.close()


def _pose(t, rot=(0.0, 0.0, 0.0)):
    a = np.asarray(rot, float)
    T = np.eye(4)
    th = np.linalg.norm(a)
    if th > 0:
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        T[:3, :3] = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
    T[:3, 3] = t
    return T


NAN = np.full((4, 4), np.nan)


# -- 1. explicit moves -------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [DIMS, (40, 13, 41)])
@pytest.mark.parametrize("color", [True, False])
def test_explicit_moves(color, dims):
    c = _Cam(n=1, color=color, dims=dims)
    rng = np.random.default_rng(1)
    win = c.window()

    def write():
        shape = dims[::-1]
        for k in KEYS:
            win.vol[k] = rng.normal(size=shape + ((3,) if k == "color" else ())).astype(np.float32)
        c.h.tsdf_write(win.vol["tsdf"], win.vol["weight"])
        if color:
            c.h.tsdf_write_color(win.vol["color"], win.vol["color_weight"])

    try:
        write()
        for delta in ((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 5), (-16, 4, -4), (4, 0, 0), (dims[0], 0, 0), (-40, 20, 50)):
            c.h.tsdf_shift(delta, stream=c.stream)
            win.shift_by(delta)
            c.check(win, delta)
            if delta[0] == dims[0]:
                assert not win.vol["weight"].any()       # the volume is empty: fill it again
                write()
        assert win.shift == [dims[0] - 51, 23, 51]
        # following (on or off) does not change what an explicit move does
        c.h.tsdf_follow(margin=3, step=2)
        write()
        c.h.tsdf_shift((-3, 1, 2), stream=c.stream)
        win.shift_by((-3, 1, 2))
        c.check(win, "with following on")
        with pytest.raises(RuntimeError, match="delta"):
            c.h.tsdf_shift((2 ** 30, 0, 0), stream=c.stream)
        for bad in (dict(margin=1, step=2), dict(margin=3, step=0), dict(margin=2 ** 30, step=1), dict(anchor=(0, 2 ** 30, 0))):
            with pytest.raises(RuntimeError, match="margin|anchor"):
                c.h.tsdf_follow(**bad)
        c.check(win, "after refused calls")
    finally:
        c.close()


# -- 2. host poses, one camera -----------------------------------------------------------------------
# (first record frame, world_T_cam per frame) of every call: translations in metres; voxels of 5 cm,
# margin 2, step 2, the default anchor = the camera's voxel at the tracking world's origin
HOST_CALLS = [
    (0, [_pose((0.0, 0.0, 0.0)), _pose((0.02, 0.0, 0.0))]),                                   # stays
    (1, [_pose((0.22, 0.0, 0.0), (0.0, 0.05, 0.0))]),                                          # x: e = 4 -> +4
    (0, [NAN, _pose((0.22, 0.01, 0.16))]),                                                     # from the 2nd frame: z e = 3 -> +2
    (1, [_pose((0.26, 0.0, 0.17)), _pose((0.3, 0.0, 0.17)), _pose((0.32, 0.0, 0.2), (0.03, 0.0, 0.0))]),   # stays
    (2, [NAN, NAN]),                                                                           # nothing at all
    (0, [_pose((-0.13, 0.0, 0.17))]),                                                          # x: e = -7 -> -6 (toward zero)
    (2, [_pose((-0.1, -0.16, 0.17), (0.0, 0.0, 0.04)), _pose((-0.1, -0.16, 0.17))]),           # y: e = -3 -> -2
    (3, [_pose((-0.1, -0.14, 0.15))]),                                                         # stays
    (1, [_pose((-0.1, -0.14, -0.22), (0.0, -0.04, 0.0)), _pose((-0.12, -0.14, -0.22))]),       # z: e = -6 -> -6
]


@pytest.mark.parametrize("distorted", [False, True])
def test_host_poses_one_camera(distorted):
    c = _Cam(distorted, n=4, color=distorted)
    win = c.window(margin=2, step=2)
    try:
        c.h.tsdf_follow(margin=2, step=2)
        for i, (f0, poses) in enumerate(HOST_CALLS):
            poses = np.stack(poses)
            before = win.vol["weight"].copy()
            c.integrate(f0, len(poses), poses)
            win.call(c.views(f0, poses))
            c.check(win, f"call {i}")
            if not np.isfinite(poses[:, 0, 0]).any():
                assert win.moves[-1] == (0, 0, 0) and np.array_equal(win.vol["weight"], before)
    finally:
        c.close()
    print("moves", win.moves, "shift", win.shift, "observed", int((win.vol["weight"] > 0).sum()))
    moved = [d for d in win.moves if any(d)]
    assert len(moved) >= 3 and len(win.moves) - len(moved) >= 2
    signs = {(a, int(np.sign(d[a]))) for d in moved for a in range(3) if d[a]}
    assert len({a for a, _ in signs}) >= 2 and {s for _, s in signs} == {-1, 1}
    assert win.moves[2] != (0, 0, 0)                 # the NaN first frame left the decision to the second
    assert (win.vol["weight"] > 0).sum() > 2000 and ((win.vol["weight"] > 0) & (win.vol["tsdf"] < 0)).sum() > 200


# -- 3. device poses ---------------------------------------------------------------------------------
def test_device_poses():
    n, per = 24, 6
    c = _Cam(n=n, color=True, track=True)
    # the anchor one voxel behind the camera along its travel (+z of the camera, about 2 voxels per 6 frames)
    win = c.window(anchor=(8, 6, -46), margin=2, step=2)
    try:
        T, st = c.res["T_abs"][:, 0], c.res["stats"][:, 0, 0]
        used = [s == 0 or (s == 2 and f == 0) for f, s in enumerate(st)]
        assert sum(used) >= n - 2
        c.h.tsdf_follow(anchor=(8, 6, -46), margin=2, step=2)
        for f0 in range(0, n, per):
            c.integrate(f0, per)                     # world_T_cam = NULL: the batch's device poses
            win.call(c.views(f0, T[f0:f0 + per], used[f0:f0 + per]))
            c.check(win, f"frames {f0}..")
    finally:
        c.close()
    print("travel (voxels)", (T[-1][:3, 3] / VOX).round(2), "moves", win.moves)
    assert sum(any(d) for d in win.moves) >= 2
    assert (win.vol["weight"] > 0).sum() > 2000


# -- 4. more than 256 frames in one call ----------------------------------------------------------------
def test_one_decision_for_a_call_of_260_frames():
    import torch

    n = 260
    c = _Cam(n=1)
    rng = np.random.default_rng(4)
    depth = rng.integers(2500, 4001, size=(n, H, W), dtype=np.uint16)
    poses = np.stack([_pose((0.22 + 0.0005 * f, 0.0, 0.0)) for f in range(n)])
    poses[256:, :3, 3] = (1.0, 0.0, 0.5)             # chunk 1 starts far away: a second decision would move again
    win = c.window(margin=2, step=2)
    try:
        dev = torch.from_numpy(depth.view(np.int16)).cuda()
        c.h.tsdf_follow(margin=2, step=2)
        c.h.tsdf_integrate(dev.data_ptr(), 2 * HW, n, world_T_cam=poses, stream=c.stream)
        c.depth = list(depth)
        win.call(c.views(0, poses, color=False))
        c.check(win)
    finally:
        c.close()
    assert win.moves == [(4, 0, 0)]
    assert REF.decide([(v["cTw"], True) for v in c.views(0, poses[256:], color=False)], ORIGIN, VOX, win.shift, win.anchor, 2, 2) != (0, 0, 0)
    assert win.vol["weight"].max() == MAX_W


# -- 5. rig --------------------------------------------------------------------------------------------
def test_rig_decides_from_the_first_selected_camera():
    import torch

    from thor_slam_amd._lib import Handle

    n, pairs = 2, (1, 3)
    s, origin = 0.1, (-1.85, -0.65, -2.05)
    sc = C.rgbd_scene(W, H, 4, False)
    P = len(sc["rects"])
    h = Handle(sc["rects"], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=4)
    win = REF.Window(origin, DIMS, s, TRUNC_VOX * s, MAX_D, MAX_W, margin=2, step=2)
    body = sc["world_T_base"]
    calls = [np.stack([body[0], body[1]]),
             np.stack([NAN, _pose((0.5, 0.0, 0.3)) @ body[1]]),       # the first used frame is the second
             np.stack([_pose((0.55, 0.0, 0.3)) @ body[0], _pose((-1.0, 0.0, 0.0)) @ body[1]]),
             np.stack([_pose((-0.2, 0.22, 0.3)) @ body[0], body[1]])]
    try:
        h.set_rig(sc["E"])
        dev = torch.from_numpy(np.ascontiguousarray(sc["records"])).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        h.tsdf_color(True)
        h.tsdf_init(origin, DIMS, s, TRUNC_VOX, MAX_D, MAX_W)
        h.tsdf_follow(margin=2, step=2)
        cams = [dict(pair=p, depth=dev.data_ptr() + p * 5 * HW + 3 * HW, stride_bytes=5 * HW * P, color=dev.data_ptr() + p * 5 * HW)
                for p in pairs]
        for i, wtb in enumerate(calls):
            h.tsdf_integrate_rig(cams, n, world_T_base=wtb, stream=stream)
            used = RIG.used_host(wtb)
            views = [(RIG.cam_T_world(RIG.world_T_cam(sc["E"], wtb[f], p)), used[f]) for f in range(n) for p in pairs]
            delta = REF.decide(views, origin, s, win.shift, win.anchor, 2, 2)
            win.shift_by(delta)
            win.moves.append(delta)
            RIG.integrate_rig(win.vol, list(pairs), [[sc["depth"][f][p] for p in pairs] for f in range(n)], wtb, used, sc["E"],
                              sc["rects"], win.origin, s, TRUNC_VOX * s, MAX_D, MAX_W,
                              bgr=[[sc["bgr"][f][p] for p in pairs] for f in range(n)])
            t, w = h.tsdf_read()
            col, cw = h.tsdf_read_color()
            shift, o = h.tsdf_window()
            assert shift.tolist() == win.shift, (i, shift, win.shift)
            np.testing.assert_array_equal(o, np.array(win.origin))
            for got, k in ((w, "weight"), (t, "tsdf"), (cw, "color_weight"), (col, "color")):
                np.testing.assert_array_equal(got, win.vol[k], err_msg=f"{k} call {i}")
    finally:
        h.close()
    print("moves", win.moves)
    assert win.moves[0] == (0, 0, 0) and sum(any(d) for d in win.moves) >= 2
    # camera 1 sits 18 cm behind and 8 cm beside pair 0's camera: the decision is not pair 0's
    views0 = [(RIG.cam_T_world(RIG.world_T_cam(sc["E"], calls[1][1], 0)), True)]
    views1 = [(RIG.cam_T_world(RIG.world_T_cam(sc["E"], calls[1][1], 1)), True)]
    assert REF.centre(views0[0][0]) != REF.centre(views1[0][0])
    assert (win.vol["weight"] > 0).sum() > 2000


# -- 6. outputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [True, False])
def test_mesh_and_esdf_of_the_moved_window(color):
    c = _Cam(n=4, color=color)
    win = c.window(margin=2, step=2)
    try:
        c.h.tsdf_follow(margin=2, step=2)
        for f0, poses in HOST_CALLS[:3]:
            poses = np.stack(poses)
            c.integrate(f0, len(poses), poses)
            win.call(c.views(f0, poses))
        assert win.shift == [4, 0, 2]
        want = DN.extract_mesh(win.vol["tsdf"], win.vol["weight"], win.origin, VOX, 1e-4, color=win.vol["color"] if color else None)
        got = c.h.mesh(1e-4, stream=c.stream, colors=color)
        if color:
            np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            got, want = got[0], want[0]
        assert want.shape[0] > 200
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        moved_by = np.array(win.origin) - np.array(ORIGIN)
        assert got[..., 0].min() >= win.origin[0] and moved_by[0] > 0.19      # metres in the tracking world
        np.testing.assert_array_equal(c.h.esdf(2.0).view(np.uint32),
                                      DN.esdf(win.vol["tsdf"], win.vol["weight"], VOX, 2.0).view(np.uint32))
        c.check(win)
    finally:
        c.close()


# -- 7. off means off ------------------------------------------------------------------------------------
def test_off_means_off_and_reset():
    c = _Cam(n=4)
    far = np.stack([_pose((0.4, -0.3, 0.5)), _pose((0.45, -0.3, 0.5))])
    plain = c.window()                               # never follows: test_gpu_tsdf.py's oracle at ORIGIN
    plain.call(c.views(0, far))
    try:
        c.integrate(0, 2, far)                       # following never enabled
        c.check(plain, "never enabled")
        c.h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
        c.h.tsdf_follow(margin=2, step=2)
        c.h.tsdf_follow(enable=False)                # enabled, then disabled
        c.integrate(0, 2, far)
        c.check(plain, "enabled then disabled")
        # on: the same call moves; off again: the window stays where it is and integrates there
        win = c.window(margin=2, step=2)
        win.vol = {k: v.copy() for k, v in plain.vol.items()}
        c.h.tsdf_follow(margin=2, step=2)
        c.integrate(0, 2, far)
        win.call(c.views(0, far))
        assert win.moves == [(8, -6, 10)]
        c.check(win, "on")
        c.h.tsdf_follow(enable=False)
        win.margin = None
        c.integrate(2, 2, np.stack([_pose((0.0, 0.0, 0.0))] * 2))
        win.call(c.views(2, [_pose((0.0, 0.0, 0.0))] * 2))
        c.check(win, "off after a move")
        c.h.reset()                                  # tslam_reset: shift 0, an empty volume
        shift, origin = c.h.tsdf_window()
        assert shift.tolist() == [0, 0, 0] and origin.tolist() == list(ORIGIN)
        assert not c.h.tsdf_read()[1].any()
        c.h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)   # a new volume does not follow
        c.integrate(0, 2, far)
        c.check(plain, "after reset and init")
    finally:
        c.close()


# -- 8. engine end to end ----------------------------------------------------------------------------------
def test_engine_follows():
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    n, per, anchor = 24, 6, (8, 9, -46)              # z as in test_device_poses; y: e = -3 at the start -> -2
    src = SyntheticRGBDSource(width=W, height=H)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    cfg = HipSlamConfig(rgbd=True, dense_map=True, dense_follow=True, dense_follow_step=2, dense_follow_margin=2, batch_size=per,
                        dense_follow_anchor=anchor, n_features=1000, n_levels=3, tsdf_origin=ORIGIN, tsdf_dims=DIMS,
                        voxel_size=VOX, tsdf_integrator_max_integration_distance_m=MAX_D, tsdf_max_weight=MAX_W,
                        esdf_slice_min_height=-0.2, esdf_slice_max_height=0.2)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    rect = eng.rectifications[0]
    win = REF.Window(ORIGIN, DIMS, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W, anchor=anchor, margin=2, step=2)
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
            res = eng.handle.read_poses(per)             # the engine's own poses of this batch
            for k, v in enumerate(views):
                s = int(res["stats"][k, 0, 0])
                v["cTw"] = REF.cam_T_world(res["T_abs"][k, 0])
                v["used"] = s == 0 or (s == 2 and g0 + k == 0)
            win.call(views)
            dm = eng.get_dense_map()
            assert dm["window_shift"].tolist() == win.shift, (g0, win.moves)
            np.testing.assert_array_equal(dm["origin"], np.array(win.origin))
            for k in KEYS:
                np.testing.assert_array_equal(dm[k], win.vol[k], err_msg=f"{k} batch at {g0}")
        print("moves", win.moves)
        assert any(win.shift) and win.shift[1] != 0 and (win.vol["weight"] > 0).sum() > 2000
        sl = eng.get_esdf_slice()
        band = lambda y: (int(np.clip(np.floor((-0.2 - y) / VOX), 0, DIMS[1] - 1)), int(np.ceil((0.2 - y) / VOX)))
        y0, y1 = band(win.origin[1])
        y1 = int(np.clip(y1, y0 + 1, DIMS[1]))
        assert sl["band"] == (y0, y1) and band(ORIGIN[1])[0] != y0
        assert sl["window_shift"].tolist() == win.shift and sl["origin"].tolist() == list(win.origin)
        want = DN.esdf_slice(win.vol["tsdf"], win.vol["weight"], VOX, cfg.esdf_integrator_max_distance_m, y0, y1)
        np.testing.assert_array_equal(sl["distance"].view(np.uint32), want.view(np.uint32))
        es = eng.get_esdf()
        assert es["window_shift"].tolist() == win.shift and es["origin"].tolist() == list(win.origin)
        mesh = eng.get_mesh()
        want_m, want_c = DN.extract_mesh(win.vol["tsdf"], win.vol["weight"], win.origin, VOX, cfg.mesh_integrator_min_weight,
                                         color=win.vol["color"])
        np.testing.assert_array_equal(mesh["triangles"].view(np.uint32), want_m.view(np.uint32))
        np.testing.assert_array_equal(mesh["colors"].view(np.uint32), want_c.view(np.uint32))
        eng.reset()
        dm = eng.get_dense_map()
        assert dm["window_shift"].tolist() == [0, 0, 0] and dm["origin"].tolist() == list(ORIGIN) and not dm["weight"].any()
    finally:
        eng.shutdown()
