"""The dense map from every camera of a rig on the device: ``tslam_tsdf_integrate_rig``
(``k_tsdf_rig_poses`` + ``k_tsdf_integrate<true>``), ``tslam_stereo_depth_slots`` and
``HipSlamConfig.dense_cameras`` against tests/ref_tsdf_rig.py — TSDF, weight, colour and colour
weight bit-exact (the same IEEE f64 operations in the same order, f32 storage after every view)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import ref_tsdf_rig as REF
import tsdf_rig_cases as C
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 3
SCENE_N = 4                      # the device-pose test tracks 4 frames; the others use the first 3
ALL = (0, 1, 2, 3)
CFG = dict(rgbd=True, n_features=1000, n_levels=3)
KEYS = ("weight", "tsdf", "color_weight", "color")


def _scene(distorted=False):
    return C.rgbd_scene(W, H, SCENE_N, distorted)


def _want(pairs=ALL, distorted=False, max_weight=C.MAX_W, order="frame"):
    return C.host_reference(W, H, N, distorted, tuple(pairs), max_weight, order, SCENE_N)


class _Rig:
    """A handle on the bracket RGB-D rig with the scene's records on the device."""

    def __init__(self, distorted=False, color=False, max_weight=C.MAX_W, dims=C.DIMS, origin=C.ORIGIN):
        import torch

        from thor_slam_amd._lib import Handle

        self.sc = _scene(distorted)
        self.h = Handle(self.sc["rects"], HipSlamConfig(**CFG), max_batch=SCENE_N)
        self.h.set_rig(self.sc["E"])
        self.dev = torch.from_numpy(np.ascontiguousarray(self.sc["records"])).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.color = color
        if color:
            self.h.tsdf_color(True)
        self.init = lambda: self.h.tsdf_init(origin, dims, C.VOX, C.TRUNC_VOX, C.MAX_D, max_weight)
        self.init()

    def cams(self, pairs, frame0=0, color=None):
        hw, P = W * H, len(self.sc["rects"])
        base = self.dev.data_ptr() + frame0 * 5 * hw * P
        color = self.color if color is None else color
        return [dict(pair=p, depth=base + p * 5 * hw + 3 * hw, stride_bytes=5 * hw * P,
                     color=base + p * 5 * hw if color else None) for p in pairs]

    def read(self):
        t, w = self.h.tsdf_read()
        out = {"tsdf": t, "weight": w}
        if self.color:
            out["color"], out["color_weight"] = self.h.tsdf_read_color()
        return out

    def close(self):
        self.h.close()


def _assert_equal(got, want, keys=None):
    for k in keys or [k for k in KEYS if k in got]:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# -- host poses ----------------------------------------------------------------------------------
@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("distorted", [False, True])
def test_host_poses_all_cameras_bit_exact(distorted, color):
    r = _Rig(distorted, color)
    try:
        r.h.tsdf_integrate_rig(r.cams(ALL), N, world_T_base=r.sc["world_T_base"][:N], stream=r.stream)
        got = r.read()
    finally:
        r.close()
    want = _want(ALL, distorted)
    assert (want["weight"] > 0).sum() > 40000 and want["weight"].max() > N
    assert ("color" in got) == color
    if color:
        assert (want["color_weight"] > 0).sum() > 1000 and got["color"].max() > 10.0
    _assert_equal(got, want)


def test_host_poses_subset_of_cameras():
    r = _Rig(True, True)
    try:
        r.h.tsdf_integrate_rig(r.cams((1, 3)), N, world_T_base=r.sc["world_T_base"][:N], stream=r.stream)
        got = r.read()
    finally:
        r.close()
    want = _want((1, 3), True)
    assert not np.array_equal(want["weight"], _want(ALL, True)["weight"])
    _assert_equal(got, want)


def test_order_is_frame_major_camera_minor():
    """max_weight = 2: the volume is the frame-major one, which the camera-major order (one launch
    per camera) does not give (tests/test_tsdf_rig_cpu.py::test_order_discriminates)."""
    r = _Rig(False, False, max_weight=2.0)
    try:
        r.h.tsdf_integrate_rig(r.cams(ALL), N, world_T_base=r.sc["world_T_base"][:N], stream=r.stream)
        got = r.read()
    finally:
        r.close()
    want, other = _want(ALL, False, 2.0, "frame"), _want(ALL, False, 2.0, "camera")
    assert (want["tsdf"] != other["tsdf"]).sum() > 100
    _assert_equal(got, want)


# -- device poses --------------------------------------------------------------------------------
def test_device_poses_batch_and_nan():
    r = _Rig(False, True)
    n = SCENE_N
    try:
        h = r.h
        h.submit(r.dev.data_ptr(), n, r.stream)
        rp = h.read_rig_poses(n)
        used = REF.used_device(rp["stats"][:, 0])
        print("rig status per frame", rp["stats"][:, 0].tolist())
        assert used[0] and int(rp["stats"][0, 0]) == 2 and sum(used) >= 2
        want = C.reference(r.sc, ALL, n=n, world_T_base=rp["T_abs"], used=used)
        h.tsdf_integrate_rig(r.cams(ALL), n, first_frame=0, stream=r.stream)          # world_T_base = NULL
        _assert_equal(r.read(), want)
        # one call per frame, device poses, and then the same poses from the host
        for host in (False, True):
            r.init()                                     # a fresh, zeroed volume and colour layer
            for f in range(n):
                if host:
                    T = rp["T_abs"][f:f + 1] if used[f] else np.full((1, 4, 4), np.nan)
                    h.tsdf_integrate_rig(r.cams(ALL, frame0=f), 1, world_T_base=T, stream=r.stream)
                else:
                    h.tsdf_integrate_rig(r.cams(ALL, frame0=f), 1, first_frame=f, stream=r.stream)
            _assert_equal(r.read(), want)
        # a NaN host pose skips every view of its frame
        r.init()
        poses = r.sc["world_T_base"][:N].copy()
        poses[1] = np.nan
        h.tsdf_integrate_rig(r.cams(ALL), N, world_T_base=poses, stream=r.stream)
        want_nan = C.reference(r.sc, ALL, n=N, world_T_base=poses)
        assert not np.array_equal(want_nan["weight"], _want(ALL)["weight"])
        _assert_equal(r.read(), want_nan)
        # frames outside the last batch are refused
        with pytest.raises(RuntimeError, match="last batch"):
            h.tsdf_integrate_rig(r.cams(ALL), n, first_frame=1, stream=r.stream)
    finally:
        r.close()


# -- chunking ------------------------------------------------------------------------------------
def test_chunks_of_whole_frames():
    """3 cameras x 90 frames = 270 views: two launches, of 85 and of 5 whole frames, in order
    (weights run into max_weight, so a chunk out of order or a view twice would show)."""
    import torch

    n, pairs = 90, (0, 1, 3)
    dims, origin = (32, 16, 32), (-1.6, -0.8, -1.6)
    r = _Rig(False, False, dims=dims, origin=origin)
    rng = np.random.default_rng(11)
    depth = rng.integers(1000, 4001, size=(len(pairs), n, H, W), dtype=np.uint16)
    poses = np.tile(np.eye(4), (n, 1, 1))
    for f in range(n):
        a = rng.normal(size=3) * 0.2
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        th = np.linalg.norm(a)
        poses[f, :3, :3] = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        poses[f, :3, 3] = rng.normal(size=3) * 0.2
    try:
        dev = torch.from_numpy(depth.view(np.int16)).cuda()      # the bytes are what matters
        cams = [dict(pair=p, depth=dev[ci].data_ptr(), stride_bytes=2 * W * H) for ci, p in enumerate(pairs)]
        r.h.tsdf_integrate_rig(cams, n, world_T_base=poses, stream=r.stream)
        got = r.read()
    finally:
        r.close()
    want = REF.integrate_rig(REF.new_volume(dims), list(pairs), [[depth[ci, f] for ci in range(len(pairs))] for f in range(n)],
                             poses, [True] * n, r.sc["E"], r.sc["rects"], origin, C.VOX, C.TRUNC_VOX * C.VOX, C.MAX_D, C.MAX_W)
    assert want["weight"].max() == C.MAX_W and (want["weight"] > 0).mean() > 0.5
    _assert_equal(got, want)


# -- refusals ------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from thor_slam_amd._lib import TsdfRigCamera, Handle

    EINVAL, ESTATE = -1, -4
    r = _Rig(False, True)
    try:
        h = r.h
        h.tsdf_integrate_rig(r.cams(ALL), 1, world_T_base=r.sc["world_T_base"][:1], stream=r.stream)
        before = r.read()
        poses = np.ascontiguousarray(r.sc["world_T_base"][:N])

        def call(handle, cams, n_cams=None, n=N):
            arr = (TsdfRigCamera * 16)()
            for i, c in enumerate(cams):
                arr[i] = TsdfRigCamera(c["pair"], 0, c["depth"] or None, c.get("color") or None, c["stride_bytes"])
            return handle.lib.tslam_tsdf_integrate_rig(handle.h, ctypes.addressof(arr), len(cams) if n_cams is None else n_cams,
                                                       n, 0, poses.ctypes.data, ctypes.c_void_p(r.stream))

        good = r.cams(ALL)
        mixed = [dict(c, color=None if i == 2 else c["color"]) for i, c in enumerate(good)]
        short = [dict(c, stride_bytes=2 * W * H - 2) for c in good]
        null = [dict(c, depth=0) for c in good]
        assert call(h, [good[1], good[0]]) == EINVAL               # pairs not ascending
        assert call(h, [good[1], good[1]]) == EINVAL
        assert call(h, [dict(good[0], pair=4)]) == EINVAL          # out of range
        assert call(h, mixed) == EINVAL                            # colour for some cameras only
        assert call(h, short) == EINVAL and call(h, null) == EINVAL
        assert call(h, good, n_cams=0) == EINVAL and call(h, good * 2 + good[:1], n_cams=9) == EINVAL
        _assert_equal(r.read(), before)
        # no rig; no volume; colour without the colour layer
        bare = Handle(r.sc["rects"], HipSlamConfig(**CFG), max_batch=1)
        try:
            bare.tsdf_init(C.ORIGIN, C.DIMS, C.VOX, C.TRUNC_VOX, C.MAX_D, C.MAX_W)
            assert call(bare, r.cams(ALL, color=False)) == ESTATE
            bare.set_rig(r.sc["E"])
            assert call(bare, good) == EINVAL                      # colour pointers, no colour layer
            assert not bare.tsdf_read()[1].any()
            assert call(bare, r.cams(ALL, color=False)) == 0
            assert bare.tsdf_read()[1].any()
        finally:
            bare.close()
        novol = Handle(r.sc["rects"], HipSlamConfig(**CFG), max_batch=1)
        try:
            novol.set_rig(r.sc["E"])
            assert call(novol, r.cams(ALL, color=False)) == ESTATE
        finally:
            novol.close()
    finally:
        r.close()


# -- stereo depth into slots ---------------------------------------------------------------------
SW, SH, SD = 328, 244, 32        # off the matcher's 252-column step and 8-row bands


@pytest.fixture(scope="module")
def stereo():
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticStereoSource

    src = SyntheticStereoSource(width=SW, height=SH)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    h = Handle([stereo_rectify(cams[li], cams[ri])], HipSlamConfig(n_features=1000, n_levels=3, max_disparity=48), max_batch=2)
    dev = torch.from_numpy(src.render_stereo_sequence(2)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    h.submit(dev.data_ptr(), 2, stream)
    h.read_poses(2)
    yield h, stream
    h.close()


@pytest.mark.parametrize("mode", ["box", "sgm", "median_speckle"])
def test_stereo_depth_first_slot(stereo, mode):
    """Slots k .. hold what slots 0 .. of a plain call hold, every other slot's depth and disp32
    stay as they were, for the last slots too (where the median's plane lies over the right-winner
    half of the scratch)."""
    h, stream = stereo
    frames, k = 5, 3

    def init():
        h.stereo_depth_init(max_frames=frames, n_disp=SD)
        if mode == "sgm":
            h.stereo_depth_sgm()
        if mode == "median_speckle":
            h.stereo_depth_filter(median=5, speckle_size=50, speckle_range=32)

    init()
    h.stereo_depth(0, 2, stream=stream)                       # the plain call: slots 0, 1
    plain = [h.stereo_depth_read(s) for s in range(2)]
    assert all((d > 0).mean() > 0.3 for d, _ in plain) and not np.array_equal(plain[0][0], plain[1][0])
    init()
    for s in range(frames):                                   # every slot: frame 1
        h.stereo_depth(1, 1, stream=stream, first_slot=s)
    for s in range(frames):
        for a, b in zip(h.stereo_depth_read(s), plain[1]):
            np.testing.assert_array_equal(a, b)
    h.stereo_depth(0, 2, stream=stream, first_slot=k)         # frames 0, 1 into the last two slots
    for s in range(frames):
        want = plain[s - k] if s >= k else plain[1]
        for a, b, name in zip(h.stereo_depth_read(s), want, ("depth", "disp32")):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} of slot {s}")
    for first, n in ((4, 2), (5, 1), (-1, 1)):
        with pytest.raises(RuntimeError, match="first_slot"):
            h.stereo_depth(0, n, stream=stream, first_slot=first)
    h.stereo_depth(1, 1, stream=stream, first_slot=4)         # the last slot alone is fine


# -- engine --------------------------------------------------------------------------------------
def _rgbd_engine(sets, batch, **kw):
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import synthetic_rgbd_rig

    _, rig = synthetic_rgbd_rig(C.joints(), C.NAMES, W, H)
    cfg = HipSlamConfig(**CFG, batch_size=batch, dense_map=True, tsdf_origin=C.ORIGIN, tsdf_dims=C.DIMS, voxel_size=C.VOX,
                        enable_loop_closure=False, **kw)
    eng = HipSlamEngine(num_cameras=8, config=cfg)
    eng.initialize(rig.calibration)
    for fs in sets:
        eng.process_frames(fs)
    eng.flush()
    return eng


def test_engine_rgbd_rig_all_cameras():
    from thor_slam_amd.synthetic import synthetic_rgbd_rig

    n = 4
    _, rig = synthetic_rgbd_rig(C.joints(), C.NAMES, W, H)
    rig.start()
    sets = [rig.get_synchronized_frames() for _ in range(n)]
    eng = _rgbd_engine(sets, n, dense_cameras="all")
    assert eng._dense_pairs == ALL
    dm = eng.get_dense_map()
    rp = eng.handle.read_rig_poses(n)
    names = [eng._cameras[l].source_name for l, _ in eng._pairs]
    depth = [[np.asarray(fs.frame_sets[nm].frames[1].image) for nm in names] for fs in sets]
    bgr = [[np.asarray(fs.frame_sets[nm].frames[0].image) for nm in names] for fs in sets]
    want = REF.integrate_rig(REF.new_volume(C.DIMS), list(ALL), depth, rp["T_abs"], REF.used_device(rp["stats"][:, 0]),
                             eng._base_T_rects, eng.rectifications, C.ORIGIN, C.VOX, C.TRUNC_VOX * C.VOX, C.MAX_D, C.MAX_W,
                             bgr=bgr)
    _assert_equal(dm, want, KEYS)
    eng.shutdown()
    # the default: pair 0 on its own pose, the same volume frame, less than half of the voxels
    plain = _rgbd_engine(sets, n)
    pm = plain.get_dense_map()
    plain.shutdown()
    np.testing.assert_array_equal(dm["world_T_volume"], pm["world_T_volume"])
    print("observed voxels: all cameras", int((dm["weight"] > 0).sum()), "default", int((pm["weight"] > 0).sum()))
    assert (dm["weight"] > 0).sum() >= 2 * (pm["weight"] > 0).sum() > 0
    # the volume does not depend on the batch size
    one = _rgbd_engine(sets, 1, dense_cameras=tuple(reversed(C.NAMES)))
    om = one.get_dense_map()
    one.shutdown()
    _assert_equal(om, dm, KEYS)


def test_engine_stereo_rig_all_cameras():
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import synthetic_rig

    n = 2
    _, rig = synthetic_rig(C.joints(), C.NAMES, W, H)
    rig.start()
    cfg = HipSlamConfig(n_features=1000, n_levels=3, max_disparity=48, batch_size=n, dense_map=True, stereo_depth=True,
                        dense_cameras="all", tsdf_origin=C.ORIGIN, tsdf_dims=C.DIMS, voxel_size=C.VOX, enable_loop_closure=False)
    eng = HipSlamEngine(num_cameras=8, config=cfg)
    eng.initialize(rig.calibration)
    stamps = []
    for _ in range(n):
        fs = rig.get_synchronized_frames()
        stamps.append(float(fs.timestamp))
        eng.process_frames(fs)
    eng.flush()
    dm = eng.get_dense_map()
    assert "color" not in dm
    rp = eng.handle.read_rig_poses(n)
    depth = [[eng.handle.stereo_depth_read(ci * n + f)[0] for ci in range(4)] for f in range(n)]   # camera ci: slots ci n ..
    assert all((d > 0).mean() > 0.2 for fr in depth for d in fr)
    want = REF.integrate_rig(REF.new_volume(C.DIMS), list(ALL), depth, rp["T_abs"], REF.used_device(rp["stats"][:, 0]),
                             eng._base_T_rects, eng.rectifications, C.ORIGIN, C.VOX, C.TRUNC_VOX * C.VOX, C.MAX_D, C.MAX_W,
                             rect=True)
    assert (want["weight"] > 0).sum() > 1000
    _assert_equal(dm, want, ("weight", "tsdf"))
    img, stamp = eng.get_depth_image(pair=2)
    assert stamp == stamps[-1]
    np.testing.assert_array_equal(img, depth[n - 1][2])
    assert not np.array_equal(img, eng.get_depth_image()[0])
    eng.shutdown()
