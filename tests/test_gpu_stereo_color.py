"""MI355X: the coloured dense map of a stereo rig.  Handle level: ``tslam_stereo_depth_images`` ->
``tslam_depth_register`` -> ``tslam_tsdf_integrate_rect_color`` (and ``_rig_color``) against the
restatements chained the same way (tests/ref_stereo_depth.py, tests/ref_depth_register.py,
oracle/numpy_tsdf.py), every layer bit for bit.  Engine: ``HipSlamConfig(stereo_color=True)`` end to
end on ``SyntheticStereoColorSource``."""

import functools

import numpy as np
import pytest

import ref_depth_register as R
import ref_stereo_depth as SD
import ref_tsdf_rig as RIG
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.camera.rig import CameraRig
from thor_slam_amd.depth_register import color_camera, compose_color_T_rect
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticStereoColorSource, default_intrinsics

pytestmark = pytest.mark.gpu

W0, H0, WC, HC = 320, 200, 640, 400
ORIGIN = (-2.0, -1.5, 0.5)
DIMS = (80, 60, 100)
VOX, TRUNC_VOX, MAX_D, MAX_W = 0.05, 4.0, 10.0, 100.0
CFG = dict(n_features=1000, n_levels=3, max_disparity=48)
LAYERS = ("tsdf", "weight", "color", "color_weight")
_IMAGES: dict = {}


class _Source(SyntheticStereoColorSource):
    """The rendered images of a frame are the same in every run: rendered once per process."""

    def render_image(self, i, cam):
        key = (i, cam)
        if key not in _IMAGES:
            _IMAGES[key] = super().render_image(i, cam)
        return _IMAGES[key]

    def render_color(self, i, noise=True):
        key = (i, "color", noise)
        if key not in _IMAGES:
            _IMAGES[key] = super().render_color(i, noise)
        return _IMAGES[key]


def _source():
    return _Source(width=W0, height=H0, color_width=WC, color_height=HC)


def _rect_of(src):
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


def _inv(T):
    return RIG.cam_T_world(np.asarray(T, dtype=np.float64))


def _read(h):
    t, w = h.tsdf_read()
    c, cw = h.tsdf_read_color()
    return {"tsdf": t, "weight": w, "color": c, "color_weight": cw}


def _same(got, want, keys=LAYERS):
    for k in keys:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@functools.lru_cache(maxsize=None)
def _chain(n=3):
    """The restatements chained: stereo depth, registration, masked colour integration on the
    ground-truth poses of n frames."""
    src = _source()
    rect = _rect_of(src)
    assert rect.is_identity
    frames = src.render_stereo_sequence(n)
    colors = np.stack([src.render_color(f) for f in range(n)])
    ccam = color_camera(src.get_rgbd_intrinsics()[0])
    T = compose_color_T_rect(src.left_T_color().to_4x4_matrix(), rect.left_optical_T_rect())
    fxb = rect.fx * rect.baseline
    depth = [SD.stereo_depth(frames[f, 0], frames[f, 1], CFG["max_disparity"], fxb)[0] for f in range(n)]
    cam = (rect.fx, rect.fy, rect.cx, rect.cy)
    reg = [R.register(depth[f], colors[f], cam, ccam, T) for f in range(n)]
    inv0 = np.linalg.inv(src.camera_pose(0, 0))
    poses = np.stack([inv0 @ src.camera_pose(f, 0) for f in range(n)])
    vol = RIG.new_volume(DIMS)
    for f in range(n):
        R.integrate_color_masked(vol, depth[f], _inv(poses[f]), cam, ORIGIN, VOX, TRUNC_VOX * VOX, MAX_D, MAX_W,
                                 bgr=reg[f]["bgr"], mask=reg[f]["mask"])
    return dict(src=src, rect=rect, frames=frames, colors=colors, ccam=ccam, T=T, fxb=fxb, depth=depth, reg=reg, poses=poses,
                vol=vol, cam=cam)


def _handle(c, n):
    from thor_slam_amd._lib import Handle

    h = Handle([c["rect"]], HipSlamConfig(**CFG), max_batch=n)
    h.tsdf_color(True)
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.stereo_depth_init(max_frames=n)
    cc = c["ccam"]
    h.depth_register_init(cc["width"], cc["height"], cc["f_c"], cc["cxc"], cc["cyc"], c["T"], map=cc["map"], max_frames=n)
    return h


def test_handle_chain_bit_exact():
    import torch

    n = 3
    c = _chain(n)
    h = _handle(c, n)
    s = torch.cuda.current_stream().cuda_stream
    dev = torch.from_numpy(np.ascontiguousarray(c["frames"])).cuda()
    col = torch.from_numpy(np.ascontiguousarray(c["colors"])).cuda()
    h.stereo_depth_images(dev.data_ptr(), dev.data_ptr() + W0 * H0, 2 * W0 * H0, W0, H0, c["fxb"], n, s)
    depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
    h.depth_register(depth_ptr, frame_bytes, col.data_ptr(), 3 * WC * HC, n, stream=s)
    ptrs, nb = h.depth_register_buffers()
    h.tsdf_integrate_rect_color(ptrs["bgr"], nb["bgr"], ptrs["mask"], nb["mask"], depth_ptr, frame_bytes, n,
                                world_T_cam=c["poses"], stream=s)
    got = _read(h)
    for f in range(n):
        np.testing.assert_array_equal(h.stereo_depth_read(f)[0], c["depth"][f])
        out = h.depth_register_read(f)
        for k in ("depth", "bgr", "mask"):
            np.testing.assert_array_equal(out[k], c["reg"][f][k], err_msg=f"{k} of frame {f}")
        assert 0.5 < c["reg"][f]["mask"].mean() < 1.0
    assert (c["vol"]["weight"] > 0).sum() > 10000 and (c["vol"]["color_weight"] > 0).sum() > 1000
    _same(got, c["vol"])
    # the geometry is tslam_tsdf_integrate_rect's, bit for bit
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.tsdf_integrate_rect(depth_ptr, frame_bytes, n, world_T_cam=c["poses"], stream=s)
    plain = _read(h)
    _same(plain, got, ("tsdf", "weight"))
    assert not plain["color_weight"].any()
    # a null mask through the new entry is today's colour integration of the same BGR: the records
    # [BGR | depth] through tslam_tsdf_integrate_rgbd (this pair's table is the identity)
    rec = np.zeros((n, 5 * W0 * H0), np.uint8)
    for f in range(n):
        rec[f, :3 * W0 * H0] = c["reg"][f]["bgr"].reshape(-1)
        rec[f, 3 * W0 * H0:] = c["depth"][f].reshape(-1).view(np.uint8)
    rdev = torch.from_numpy(rec).cuda()
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.tsdf_integrate_rgbd(rdev.data_ptr(), rdev.data_ptr() + 3 * W0 * H0, 5 * W0 * H0, n, world_T_cam=c["poses"], stream=s)
    today = _read(h)
    h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
    h.tsdf_integrate_rect_color(ptrs["bgr"], nb["bgr"], None, 0, depth_ptr, frame_bytes, n, world_T_cam=c["poses"], stream=s)
    _same(_read(h), today)
    assert not np.array_equal(today["color_weight"], got["color_weight"])   # the mask left voxels out
    _same(today, got, ("tsdf", "weight"))
    h.close()


def _level0(h, g, cam):
    blk = h.frame_block("pyramid", h.ring_slot(g), np.uint8).reshape(h.n_cams, h.pyr_bytes)
    return blk[cam, h.pyr_off[0]:h.pyr_off[0] + h.width * h.height].reshape(h.height, h.width)


def test_rig_one_pair_coloured():
    """The same chain on a two-pair rig: tslam_stereo_depth_slots of both pairs -> tslam_depth_register
    of pair 0 -> tslam_tsdf_integrate_rig_color, pair 1 with a black image and a zero mask, against
    the restatements chained the same way; the geometry against tslam_tsdf_integrate_rig; and NULL
    masks through _rig_color against today's tslam_tsdf_integrate_rig colour of the same BGR."""
    import torch

    import tsdf_rig_cases as TR
    from helpers import rig_scene
    from thor_slam_amd._lib import Handle

    n = 2
    sc = rig_scene(n=n, width=W0, height=H0)
    rects, E = sc["rects"], sc["E"]
    h = Handle(rects, HipSlamConfig(**CFG), max_batch=n)
    h.set_rig(E)
    h.tsdf_color(True)
    h.tsdf_init(TR.ORIGIN, TR.DIMS, TR.VOX, TR.TRUNC_VOX, TR.MAX_D, TR.MAX_W)
    s = torch.cuda.current_stream().cuda_stream
    fdev = torch.from_numpy(np.ascontiguousarray(sc["frames"])).cuda()
    h.submit(fdev.data_ptr(), n, s)
    h.stereo_depth_init(max_frames=2 * n)
    for p in (0, 1):
        h.stereo_depth(0, n, pair=p, stream=s, first_slot=p * n)
    depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
    # the restatements, chained: stereo depth of the rectified images, registration, masked integration
    depth = np.zeros((2, n, H0, W0), np.uint16)
    for p in (0, 1):
        for f in range(n):
            depth[p, f] = SD.stereo_depth(_level0(h, f, 2 * p), _level0(h, f, 2 * p + 1), CFG["max_disparity"],
                                          rects[p].fx * rects[p].baseline)[0]
            np.testing.assert_array_equal(h.stereo_depth_read(p * n + f)[0], depth[p, f])
    assert (depth > 0).mean() > 0.2
    colors = np.random.default_rng(5).integers(0, 256, size=(n, HC, WC, 3), dtype=np.uint8)
    ccam = color_camera(default_intrinsics(WC, HC))
    lTc = np.eye(4)
    lTc[0, 3] = 0.0375
    T = compose_color_T_rect(lTc, rects[0].left_optical_T_rect())
    cam0 = (rects[0].fx, rects[0].fy, rects[0].cx, rects[0].cy)
    reg = [R.register(depth[0, f], colors[f], cam0, ccam, T) for f in range(n)]
    wtb = np.stack([np.linalg.inv(sc["traj"][0]) @ sc["traj"][f] for f in range(n)])
    black = np.zeros((H0, W0, 3), np.uint8)

    def reference(masked):
        vol = RIG.new_volume(TR.DIMS)
        for f in range(n):
            for p in (0, 1):
                r = rects[p]
                mask = None if not masked else reg[f]["mask"] if p == 0 else np.zeros((H0, W0), np.uint8)
                R.integrate_color_masked(vol, depth[p, f], RIG.cam_T_world(RIG.world_T_cam(E, wtb[f], p)),
                                         (r.fx, r.fy, r.cx, r.cy), TR.ORIGIN, TR.VOX, TR.TRUNC_VOX * TR.VOX, TR.MAX_D, TR.MAX_W,
                                         bgr=reg[f]["bgr"] if p == 0 else black, mask=mask)
        return vol

    vol = reference(True)
    assert (vol["color_weight"] > 0).sum() > 1000

    h.depth_register_init(ccam["width"], ccam["height"], ccam["f_c"], ccam["cxc"], ccam["cyc"], T, max_frames=n)
    cdev = torch.from_numpy(colors).cuda()
    hw = W0 * H0
    h.depth_register(depth_ptr, frame_bytes, cdev.data_ptr(), 3 * WC * HC, n, stream=s)
    ptrs, nb = h.depth_register_buffers()
    bdev = torch.zeros((n, H0, W0, 3), dtype=torch.uint8, device="cuda")
    zero = torch.zeros((n, H0, W0), dtype=torch.uint8, device="cuda")
    base = [dict(pair=p, rect=True, depth=depth_ptr + p * n * frame_bytes, stride_bytes=frame_bytes) for p in (0, 1)]
    cams = [dict(base[0], color=ptrs["bgr"], color_stride=nb["bgr"], mask=ptrs["mask"], mask_stride=nb["mask"]),
            dict(base[1], color=bdev.data_ptr(), color_stride=3 * hw, mask=zero.data_ptr(), mask_stride=hw)]
    h.tsdf_integrate_rig_color(cams, n, world_T_base=wtb, stream=s)
    got = _read(h)
    _same(got, vol)
    h.tsdf_init(TR.ORIGIN, TR.DIMS, TR.VOX, TR.TRUNC_VOX, TR.MAX_D, TR.MAX_W)
    h.tsdf_integrate_rig(base, n, world_T_base=wtb, stream=s)
    _same(_read(h), got, ("tsdf", "weight"))
    # NULL masks: today's colour integration of the same BGR, which takes [BGR | depth] records of one stride
    rec = np.zeros((2, n, 5 * hw), np.uint8)
    for p in (0, 1):
        for f in range(n):
            rec[p, f, :3 * hw] = (reg[f]["bgr"] if p == 0 else black).reshape(-1)
            rec[p, f, 3 * hw:] = depth[p, f].reshape(-1).view(np.uint8)
    rdev = torch.from_numpy(rec).cuda()
    h.tsdf_init(TR.ORIGIN, TR.DIMS, TR.VOX, TR.TRUNC_VOX, TR.MAX_D, TR.MAX_W)
    h.tsdf_integrate_rig([dict(pair=p, rect=True, depth=rdev.data_ptr() + p * n * 5 * hw + 3 * hw, stride_bytes=5 * hw,
                               color=rdev.data_ptr() + p * n * 5 * hw) for p in (0, 1)], n, world_T_base=wtb, stream=s)
    today = _read(h)
    _same(today, reference(False))
    h.tsdf_init(TR.ORIGIN, TR.DIMS, TR.VOX, TR.TRUNC_VOX, TR.MAX_D, TR.MAX_W)
    h.tsdf_integrate_rig_color([dict(cams[0], mask=None, mask_stride=0), dict(cams[1], mask=None, mask_stride=0)], n,
                               world_T_base=wtb, stream=s)
    _same(_read(h), today)
    assert not np.array_equal(today["color_weight"], got["color_weight"])
    h.close()


# -- engine --------------------------------------------------------------------------------------
def _engine(batch, stereo_color=True):
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.slam.hip_engine import HipSlamEngine

    src = _source()
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    cfg = HipSlamConfig(**CFG, batch_size=batch, tsdf_origin=ORIGIN, tsdf_dims=DIMS, tsdf_integrator_max_integration_distance_m=MAX_D,
                        tsdf_max_weight=MAX_W, enable_loop_closure=False, dense_map=True, stereo_depth=True,
                        stereo_color=stereo_color)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    if stereo_color:
        eng.set_color_camera(src.name, src.get_rgbd_intrinsics()[0], src.left_T_color())
    return eng, src, rig


def _feed(eng, src, rig, i, color="in time"):
    fs = rig.get_synchronized_frames()
    if color == "in time":
        eng.push_color(0, src.render_color(i), float(fs.timestamp) + 0.01)
    elif color == "late":
        eng.push_color(0, src.render_color(i), float(fs.timestamp) + 0.1)
    eng.process_frames(fs)
    return float(fs.timestamp)


def _run(batch, stereo_color=True, n=6):
    eng, src, rig = _engine(batch, stereo_color)
    stamps = [_feed(eng, src, rig, i, "in time" if stereo_color else None) for i in range(n)]
    eng.flush()
    return eng, src, stamps


def test_engine_end_to_end():
    eng, src, stamps = _run(3)
    dm = eng.get_dense_map()
    plain, _, _ = _run(3, stereo_color=False)
    pm = plain.get_dense_map()
    assert "color" not in pm and plain.get_registered_depth() is None
    _same(dm, pm, ("tsdf", "weight"))
    plain.shutdown()
    seen, col = dm["weight"] > 0, dm["color_weight"] > 0
    assert seen.sum() > 10000 and not (col & ~seen).any()
    near = seen & (np.abs(dm["tsdf"]) < 0.5 * dm["truncation_m"])     # voxels the surface passes through
    frac = float(col[near].mean())
    print(f"coloured share of the voxels near the surface: {frac:.3f} of {int(near.sum())}")
    assert frac > 0.5
    g = dm["color"][col]
    assert g[:, 1].std() > 5.0                                         # the room's texture, not a constant
    mesh = eng.get_mesh()
    assert mesh["colors"].shape == mesh["triangles"].shape and mesh["triangles"].shape[0] > 1000
    view = eng.get_dense_view()
    assert view["colors"].shape == (H0, W0, 3) and view["colors"].any()
    # the registered depth of the newest frame: the restatement on the engine's own stereo depth
    depth, stamp = eng.get_depth_image()
    reg, rstamp = eng.get_registered_depth()
    assert stamp == rstamp == stamps[-1]
    rect = eng.rectifications[0]
    ccam = color_camera(src.get_rgbd_intrinsics()[0])
    T = compose_color_T_rect(src.left_T_color().to_4x4_matrix(), rect.left_optical_T_rect())
    want = R.register(depth, src.render_color(5), (rect.fx, rect.fy, rect.cx, rect.cy), ccam, T)
    assert reg.shape == (HC, WC) and (reg > 0).mean() > 0.3
    np.testing.assert_array_equal(reg, want["depth"])
    # the result does not depend on the batch size
    one, _, _ = _run(1)
    _same(one.get_dense_map(), dm)
    np.testing.assert_array_equal(one.get_registered_depth()[0], reg)
    one.shutdown()
    eng.shutdown()


def test_engine_frames_without_colour():
    """A frame whose colour was not pushed, or came 0.1 s late, leaves the colour layer as it was
    while the geometry advances."""
    eng, src, rig = _engine(1)
    for i in range(2):
        _feed(eng, src, rig, i)
    stamps = [_feed(eng, src, rig, i) for i in range(2)]
    last, last_stamp = eng.get_registered_depth()
    assert last_stamp == stamps[1] and (last > 0).mean() > 0.3
    for i, how in ((2, None), (3, "late")):
        before = eng.get_dense_map()
        assert (before["color_weight"] > 0).sum() > 1000
        _feed(eng, src, rig, i, how)
        after = eng.get_dense_map()
        _same(after, before, ("color", "color_weight"))
        assert not np.array_equal(after["weight"], before["weight"])
        reg, stamp = eng.get_registered_depth()      # still the newest REGISTERED frame, under its own timestamp
        assert stamp == last_stamp
        np.testing.assert_array_equal(reg, last)
    before = eng.get_dense_map()
    t4 = _feed(eng, src, rig, 4)
    assert not np.array_equal(eng.get_dense_map()["color_weight"], before["color_weight"])
    reg, stamp = eng.get_registered_depth()
    assert stamp == t4 and not np.array_equal(reg, last)
    eng.shutdown()
    # and what the map holds is the same as a run that skips the same frames' colour in one batch of 3
    full, src, rig = _engine(3)
    for i, how in enumerate(("in time", "in time", None, "late", "in time", "in time")):
        _feed(full, src, rig, i, how)
    ref, src, rig = _engine(1)
    for i, how in enumerate(("in time", "in time", None, "late", "in time", "in time")):
        _feed(ref, src, rig, i, how)
    _same(full.get_dense_map(), ref.get_dense_map())
    # batches [T, T, F] and [late, T, T]: the colourless frames leave the registered planes alone
    (fr, fs_), (rr, rs) = full.get_registered_depth(), ref.get_registered_depth()
    assert fs_ == rs
    np.testing.assert_array_equal(fr, rr)
    full.shutdown()
    ref.shutdown()


def test_engine_rig_one_source_coloured():
    """``dense_cameras="all"`` on a two-source stereo rig of which the second has a colour camera:
    one ``tslam_tsdf_integrate_rig_color`` per batch, against the restatements on the engine's own
    stereo depth and body poses; the geometry is that of the run without colour."""
    import tsdf_rig_cases as TR
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import synthetic_rig

    n, names = 2, ("192.168.2.21", "192.168.2.25")
    colors = np.random.default_rng(8).integers(0, 256, size=(n, HC, WC, 3), dtype=np.uint8)
    intr = default_intrinsics(WC, HC)
    lTc = np.eye(4)
    lTc[0, 3] = 0.0375

    def run(stereo_color):
        from thor_slam_amd.camera import Extrinsics

        _, rig = synthetic_rig(TR.joints(), names, W0, H0)
        rig.start()
        cfg = HipSlamConfig(**CFG, batch_size=n, dense_map=True, stereo_depth=True, dense_cameras="all", tsdf_origin=TR.ORIGIN,
                            tsdf_dims=TR.DIMS, voxel_size=TR.VOX, enable_loop_closure=False, stereo_color=stereo_color)
        eng = HipSlamEngine(num_cameras=4, config=cfg)
        eng.initialize(rig.calibration)
        if stereo_color:
            eng.set_color_camera(names[1], intr, Extrinsics.from_4x4_matrix(lTc))
        for f in range(n):
            fs = rig.get_synchronized_frames()
            if stereo_color:
                eng.push_color(names[1], colors[f], float(fs.timestamp))
            eng.process_frames(fs)
        eng.flush()
        return eng

    eng = run(True)
    dm = eng.get_dense_map()
    rp = eng.handle.read_rig_poses(n)
    used = RIG.used_device(rp["stats"][:, 0])
    assert all(used)
    rects, E = eng.rectifications, eng._base_T_rects
    depth = [[eng.handle.stereo_depth_read(ci * n + f)[0] for ci in range(2)] for f in range(n)]
    ccam = color_camera(intr)
    T = compose_color_T_rect(lTc, rects[1].left_optical_T_rect())
    vol = RIG.new_volume(TR.DIMS)
    tol = int(round(TR.VOX * 1000))          # stereo_color_tol_m None: one voxel of this map, 100 mm
    for f in range(n):
        for p in (0, 1):
            r = rects[p]
            cam = (r.fx, r.fy, r.cx, r.cy)
            reg = R.register(depth[f][p], colors[f], cam, ccam, T, tol_mm=tol) if p == 1 else None
            R.integrate_color_masked(vol, depth[f][p], RIG.cam_T_world(RIG.world_T_cam(E, rp["T_abs"][f], p)), cam, TR.ORIGIN,
                                     TR.VOX, TR.TRUNC_VOX * TR.VOX, TR.MAX_D, TR.MAX_W,
                                     bgr=reg["bgr"] if p == 1 else np.zeros((H0, W0, 3), np.uint8),
                                     mask=reg["mask"] if p == 1 else np.zeros((H0, W0), np.uint8))
    assert (vol["color_weight"] > 0).sum() > 100
    _same(dm, vol)
    np.testing.assert_array_equal(eng.get_registered_depth(1)[0], R.register(depth[n - 1][1], colors[n - 1],
                                  (rects[1].fx, rects[1].fy, rects[1].cx, rects[1].cy), ccam, T, tol_mm=tol)["depth"])
    assert eng.get_registered_depth(0) is None
    eng.shutdown()
    plain = run(False)
    _same(plain.get_dense_map(), dm, ("tsdf", "weight"))
    plain.shutdown()


def test_process_batch_is_geometry_only():
    """``process_batch`` takes device images only, so no colour comes with them: with a colour camera
    set the batch is integrated for its geometry, and the colour layer and the registration slots stay."""
    import torch

    eng, src, rig = _engine(2)
    dev = torch.from_numpy(np.ascontiguousarray(src.render_stereo_sequence(2))).cuda()
    eng.process_batch(dev, timestamps=[0.0, 1.0])
    dm = eng.get_dense_map()
    assert (dm["weight"] > 0).sum() > 10000 and not dm["color_weight"].any()
    assert eng.get_registered_depth() is None
    eng.shutdown()
