"""MI355X: ``tslam_depth_register_init`` / ``tslam_depth_register`` / ``tslam_depth_register_buffers`` /
``tslam_depth_register_read`` (``k_dr_clear``, ``k_dr_splat``, ``k_dr_gather`` in
``k_depth_register.hip``) against ``tests/ref_depth_register.py``, every output bit for bit.  One
small handle runs every case through the depth size in the parameters."""

import ctypes

import numpy as np
import pytest

import depth_register_cases as C
import ref_depth_register as R
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.camera.rig import CameraRig
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticStereoSource

pytestmark = pytest.mark.gpu

CFG = dict(n_features=1000, n_levels=3, max_disparity=48)
OUT = ("depth", "bgr", "mask")


def _rect_of(src):
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


@pytest.fixture(scope="module")
def handle():
    from thor_slam_amd._lib import Handle

    rect = _rect_of(SyntheticStereoSource(width=C.HANDLE_SIZE[0], height=C.HANDLE_SIZE[1]))
    assert (rect.fx, rect.fy, rect.cx, rect.cy) == C.DEPTH_CAM and rect.is_identity
    h = Handle([rect], HipSlamConfig(**CFG), max_batch=2)
    yield h
    h.close()


def _init(h, dsize, ccam, T, max_frames=1, **kw):
    h.depth_register_init(ccam["width"], ccam["height"], ccam["f_c"], ccam["cxc"], ccam["cyc"], T, map=ccam["map"],
                          width=dsize[0], height=dsize[1], max_frames=max_frames, **kw)


def _run(h, depth, color, n=1, first_slot=0, depth_pad=0, color_pad=0):
    """depth [n][H][W] u16 and color [n][Hc][Wc][3] u8 through the device, frames padded apart."""
    import torch

    depth, color = np.asarray(depth).reshape((n,) + depth.shape[-2:]), np.asarray(color).reshape((n,) + color.shape[-3:])
    ds, cs = depth[0].nbytes + depth_pad, color[0].nbytes + color_pad
    dbuf, cbuf = np.full(n * ds, 0xA5, np.uint8), np.full(n * cs, 0x5A, np.uint8)
    for f in range(n):
        dbuf[f * ds:f * ds + depth[f].nbytes] = depth[f].reshape(-1).view(np.uint8)
        cbuf[f * cs:f * cs + color[f].nbytes] = color[f].reshape(-1)
    dd, cd = torch.from_numpy(dbuf).cuda(), torch.from_numpy(cbuf).cuda()
    h.depth_register(dd.data_ptr(), ds, cd.data_ptr(), cs, n, first_slot=first_slot,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _check(h, slot, want):
    got = h.depth_register_read(slot)
    for k in OUT:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (slot, k)
    return got


@pytest.mark.parametrize("shape", ["up", "down", "ragged"])
@pytest.mark.parametrize("distorted,T", [(False, "OFFSET"), (True, "OFFSET"), (True, "BEHIND")])
def test_register_matches_the_restatement(handle, shape, distorted, T):
    """Every shape with an undistorted and a distorted colour camera (the table is not the
    identity), slightly offset and moved so that part of the depth falls behind or outside it;
    invalid depth: 0, above max_depth_mm, 65535."""
    dsize, csize = C.SHAPES[shape]
    ccam = C.color_cam(dsize, csize, C.DISTORTION if distorted else None)
    assert (ccam["map"] is not None) == distorted
    T = getattr(C, T)
    depth, color = C.depth_image(dsize, seed=3), C.color_image(csize, seed=3)
    want = R.register(depth, color, C.DEPTH_CAM, ccam, T, max_depth_mm=40000)
    assert want["mask"].any() and (want["mask"] == 0).any() and (want["depth"] > 0).any()
    _init(handle, dsize, ccam, T, max_depth_mm=40000)
    _run(handle, depth, color)
    _check(handle, 0, want)


@pytest.mark.parametrize("max_splat", [1, 2, 4, 8])
def test_footprint_cap(handle, max_splat):
    """Footprints of 2-3 pixels against the cap; at 8 nothing is clipped."""
    dsize, csize = C.SHAPES["up"]
    ccam = C.color_cam(dsize, csize)
    depth, color = C.depth_image(dsize, seed=4), C.color_image(csize, seed=4)
    want = R.register(depth, color, C.DEPTH_CAM, ccam, C.OFFSET, max_splat=max_splat)
    _init(handle, dsize, ccam, C.OFFSET, max_splat=max_splat)
    _run(handle, depth, color)
    _check(handle, 0, want)
    if max_splat == 1:
        assert (want["depth"] > 0).mean() < 0.3
    if max_splat >= 4:
        assert (want["depth"] > 0).mean() > 0.7


def test_zc_beyond_the_range(handle):
    """Valid depth whose depth in the colour camera exceeds 65535 mm, or is 0 mm, lands nowhere."""
    dsize, csize = C.SHAPES["ragged"]
    ccam = C.color_cam(dsize, csize)
    depth = C.depth_image(dsize, seed=6, holes=False)
    depth[::3, ::2] = 65000
    depth[1::3, 1::2] = 1
    T = C.transform(t=(0.0, 0.0, 0.6))          # 65.0 m + 0.6 m > 65.535 m
    color = C.color_image(csize, seed=6)
    want = R.register(depth, color, C.DEPTH_CAM, ccam, T)
    assert (want["mask"][::3, ::2] == 0).all() and want["mask"].any()
    _init(handle, dsize, ccam, T)
    _run(handle, depth, color)
    _check(handle, 0, want)
    T = C.transform(t=(0.0, 0.0, -0.0008))      # 1 mm - 0.8 mm rounds to 0
    want = R.register(depth, color, C.DEPTH_CAM, ccam, T)
    assert (want["mask"][1::3, 1::2] == 0).all()
    _init(handle, dsize, ccam, T)
    _run(handle, depth, color)
    _check(handle, 0, want)


@pytest.mark.parametrize("tol", [0, 50])
def test_occlusion_scene(handle, tol):
    depth, ccam, T, band = C.occlusion_case()
    color = C.color_image((ccam["width"], ccam["height"]), seed=2)
    want = R.register(depth, color, C.DEPTH_CAM, ccam, T, tol_mm=tol)
    assert abs((want["mask"][5] == 0).sum() - band) <= 1
    _init(handle, (96, 64), ccam, T, tol_mm=tol)
    _run(handle, depth, color)
    _check(handle, 0, want)


def test_slots_and_strides(handle):
    """5 frames of different content, frames further apart than an image, into slots 2..6 while
    slots 0 and 1 keep what an earlier call wrote."""
    dsize, csize = C.SHAPES["ragged"]
    ccam = C.color_cam(dsize, csize, C.DISTORTION)
    _init(handle, dsize, ccam, C.OFFSET, max_frames=7)
    first = [(C.depth_image(dsize, seed=20 + f), C.color_image(csize, seed=20 + f)) for f in range(2)]
    _run(handle, np.stack([d for d, _ in first]), np.stack([c for _, c in first]), n=2)
    frames = [(C.depth_image(dsize, seed=30 + f), C.color_image(csize, seed=30 + f)) for f in range(5)]
    _run(handle, np.stack([d for d, _ in frames]), np.stack([c for _, c in frames]), n=5, first_slot=2, depth_pad=38, color_pad=17)
    for f, (d, c) in enumerate(first):
        _check(handle, f, R.register(d, c, C.DEPTH_CAM, ccam, C.OFFSET))
    for f, (d, c) in enumerate(frames):
        _check(handle, 2 + f, R.register(d, c, C.DEPTH_CAM, ccam, C.OFFSET))
    ptrs, nbytes = handle.depth_register_buffers()
    assert all(ptrs.values())
    assert nbytes == {"depth": 2 * csize[0] * csize[1], "bgr": 3 * dsize[0] * dsize[1], "mask": dsize[0] * dsize[1]}


@pytest.mark.parametrize("size", [(96, 64), (83, 51)])
def test_identity_property(handle, size):
    fx, fy, cx, cy = C.DEPTH_CAM
    ccam = {"width": size[0], "height": size[1], "f_c": fx, "cxc": cx, "cyc": cy, "map": None}
    depth, color = C.depth_image(size, seed=1), C.color_image(size, seed=1)
    _init(handle, size, ccam, C.IDENTITY, max_depth_mm=40000, tol_mm=0)
    _run(handle, depth, color)
    got = handle.depth_register_read(0)
    valid = (depth > 0) & (depth <= 40000)
    assert np.array_equal(got["depth"], np.where(valid, depth, 0))
    assert np.array_equal(got["mask"], valid.astype(np.uint8))
    assert np.array_equal(got["bgr"], np.where(valid[..., None], color, 0))


def test_two_runs_identical(handle):
    """Many depth pixels per colour pixel: the minimum wins, whatever order the atomics arrive in."""
    dsize, csize = C.SHAPES["down"]
    ccam = C.color_cam(dsize, csize)
    depth, color = C.depth_image(dsize, seed=5), C.color_image(csize, seed=5)
    want = R.register(depth, color, C.DEPTH_CAM, ccam, C.OFFSET)
    _init(handle, dsize, ccam, C.OFFSET)
    runs = []
    for _ in range(2):
        _run(handle, depth, color)
        runs.append(_check(handle, 0, want))
    for k in OUT:
        assert np.array_equal(runs[0][k], runs[1][k])


def test_refusals():
    import torch

    from thor_slam_amd import _lib
    from thor_slam_amd._lib import DepthRegisterParams, Handle, TsdfRigCamera, TsdfRigColor
    from thor_slam_amd.calib import rgbd_pairs, rgbd_undistort
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    lib = _lib.load_library()
    EINVAL, ESTATE = -1, -4
    W, H = C.HANDLE_SIZE
    h = Handle([_rect_of(SyntheticStereoSource(width=W, height=H))], HipSlamConfig(**CFG), max_batch=2)
    dsize, csize = C.SHAPES["up"]
    ccam = C.color_cam(dsize, csize)

    def prm(**kw):
        v = dict(width=dsize[0], height=dsize[1], color_width=csize[0], color_height=csize[1], f_c=ccam["f_c"], cxc=ccam["cxc"],
                 cyc=ccam["cyc"], map=None, T=C.OFFSET, max_depth_mm=65535, tol_mm=50, max_splat=4, reserved=0)
        v.update(kw)
        return DepthRegisterParams(v["width"], v["height"], v["color_width"], v["color_height"], v["f_c"], v["cxc"], v["cyc"],
                                   v["map"], (ctypes.c_double * 12)(*[float(x) for x in v["T"]]), v["max_depth_mm"],
                                   v["tol_mm"], v["max_splat"], v["reserved"])

    def init(p, frames=2, pair=0, hh=None):
        return lib.tslam_depth_register_init((hh or h).h, pair, ctypes.addressof(p) if p is not None else None, frames)

    dd = torch.zeros(4 * dsize[0] * dsize[1], dtype=torch.int16, device="cuda")
    cd = torch.zeros(4 * 3 * csize[0] * csize[1], dtype=torch.uint8, device="cuda")
    ds, cs = 2 * dsize[0] * dsize[1], 3 * csize[0] * csize[1]

    def run(n=1, slot=0, depth=dd.data_ptr(), color=cd.data_ptr(), dstride=ds, cstride=cs, pair=0):
        return lib.tslam_depth_register(h.h, pair, depth, dstride, color, cstride, n, slot, None)

    # before init: no state
    assert run() == ESTATE
    assert lib.tslam_depth_register_buffers(h.h, 0, None, None, None, None) == ESTATE
    assert lib.tslam_depth_register_read(h.h, 0, 0, None, None, None) == ESTATE
    assert lib.tslam_depth_register_blank(h.h, 0, 1, 0, None) == ESTATE
    assert lib.tslam_depth_register_profile(h.h, 0, (ctypes.c_double * 3)()) == ESTATE
    # init: every parameter
    assert lib.tslam_depth_register_init(None, 0, ctypes.addressof(prm()), 1) == EINVAL
    assert init(None) == EINVAL
    nan = np.array(C.OFFSET)
    nan[5] = np.nan
    for bad in (dict(width=15), dict(height=15), dict(width=W + 1), dict(height=H + 1), dict(color_width=0), dict(color_height=0),
                dict(color_width=16385), dict(f_c=0.0), dict(f_c=float("nan")), dict(cyc=float("inf")), dict(T=nan),
                dict(max_depth_mm=0), dict(max_depth_mm=65536), dict(tol_mm=-1), dict(tol_mm=65536), dict(max_splat=0),
                dict(max_splat=9), dict(reserved=1)):
        assert init(prm(**bad)) == EINVAL, bad
    assert init(prm(), frames=0) == EINVAL and init(prm(), frames=65536) == EINVAL
    assert init(prm(), pair=1) == EINVAL and init(prm(), pair=-1) == EINVAL
    assert lib.tslam_last_error()
    assert run() == ESTATE                                   # a refused init leaves it off
    assert init(prm()) == 0
    # register: planes, counts, slots, strides
    assert run(depth=None) == EINVAL and run(color=None) == EINVAL
    assert run(n=-1) == EINVAL and run(n=3) == EINVAL
    assert run(n=1, slot=2) == EINVAL and run(n=2, slot=1) == EINVAL and run(slot=-1) == EINVAL
    assert run(n=2, dstride=ds - 2) == EINVAL and run(n=2, cstride=cs - 1) == EINVAL and run(dstride=ds + 1) == EINVAL
    assert run(pair=1) == EINVAL
    assert run(n=0) == 0 and run(n=2) == 0
    blank = lib.tslam_depth_register_blank
    assert blank(h.h, 1, 1, 0, None) == EINVAL and blank(h.h, 0, 3, 0, None) == EINVAL and blank(h.h, 0, -1, 0, None) == EINVAL
    assert blank(h.h, 0, 1, 2, None) == EINVAL and blank(h.h, 0, 2, 1, None) == EINVAL and blank(h.h, 0, 1, -1, None) == EINVAL
    assert lib.tslam_depth_register_read(h.h, 0, 2, None, None, None) == EINVAL
    assert lib.tslam_depth_register_read(h.h, 0, -1, None, None, None) == EINVAL
    assert lib.tslam_depth_register_read(h.h, 0, 1, None, None, None) == 0      # any pointer may be NULL
    assert lib.tslam_depth_register_buffers(h.h, 0, None, None, None, None) == 0
    # a refused call changes nothing: the state and the slots stay
    before = h_read(lib, h, dsize, csize)
    assert init(prm(max_splat=9)) == EINVAL and run(n=3) == EINVAL
    after = h_read(lib, h, dsize, csize)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # inside a batch
    img = torch.zeros((1, 2, H, W), dtype=torch.uint8, device="cuda")
    h.begin_batch(img.data_ptr(), 1)
    assert init(prm()) == ESTATE and run() == ESTATE and blank(h.h, 0, 1, 0, None) == ESTATE
    h.end_batch()
    # tslam_reset keeps the state
    h.reset()
    assert run() == 0
    # blank: bgr and mask of the slot go to zero, its registered depth stays
    _run(h, C.depth_image(dsize, seed=3), C.color_image(csize, seed=3))
    before = h_read(lib, h, dsize, csize)
    assert before[0].any() and before[1].any() and before[2].any()
    assert blank(h.h, 0, 1, 0, None) == 0
    after = h_read(lib, h, dsize, csize)
    assert np.array_equal(after[0], before[0]) and not after[1].any() and not after[2].any()
    # the colour entries of the integrator: strides of their own, at least one image for any n_frames
    rc = lib.tslam_tsdf_integrate_rect_color
    pose = np.eye(4)
    hw = W * H
    big = torch.zeros(2 * 5 * hw, dtype=torch.uint8, device="cuda")
    B = big.data_ptr()

    def rect(hh=h.h, pair=0, color=B, cstride=3 * hw, mask=B, mstride=hw, depth=B, n=1):
        poses = np.stack([pose] * max(n, 1))
        return rc(hh, pair, color, cstride, mask, mstride, depth, 2 * hw, n, 0, poses.ctypes.data, None)

    assert rect() == ESTATE                                   # no colour layer
    h.tsdf_color(True)
    assert rect() == ESTATE                                   # no volume
    h.tsdf_init((-1.0, -1.0, 0.0), (16, 16, 16))
    assert rect(color=None) == EINVAL and rect(hh=None) == EINVAL and rect(pair=1) == EINVAL and rect(depth=None) == EINVAL
    for n in (1, 2):
        assert rect(cstride=3 * hw - 1, n=n) == EINVAL and rect(cstride=0, n=n) == EINVAL and rect(cstride=-3 * hw, n=n) == EINVAL
        assert rect(mstride=hw - 1, n=n) == EINVAL and rect(mstride=0, n=n) == EINVAL and rect(mstride=-hw, n=n) == EINVAL
        assert rect(mask=None, mstride=0, n=n) == 0 and rect(n=n) == 0
    rg = lib.tslam_tsdf_integrate_rig_color
    cam = (TsdfRigCamera * 1)(TsdfRigCamera(0, 1, B, None, 2 * hw))
    col = (TsdfRigColor * 1)(TsdfRigColor(B, 3 * hw, B, hw))
    assert rg(h.h, ctypes.addressof(cam), ctypes.addressof(col), 1, 1, 0, pose.ctypes.data, None) == ESTATE   # no rig
    assert rg(h.h, ctypes.addressof(cam), None, 1, 1, 0, pose.ctypes.data, None) == EINVAL
    h.close()

    # tslam_tsdf_integrate_rig_color on a two-pair rig
    from helpers import rig_scene

    sc = rig_scene(n=2, width=320, height=200)
    r = Handle(sc["rects"], HipSlamConfig(**CFG), max_batch=2)
    r.set_rig(sc["E"])
    r.tsdf_color(True)
    r.tsdf_init((-1.0, -1.0, 0.0), (16, 16, 16))
    hw = 320 * 200

    def rig(colors=((B, 3 * hw, B, hw), (B, 3 * hw, B, hw)), cam_color=(None, None), n=1, pairs=(0, 1)):
        cams = (TsdfRigCamera * 2)(*[TsdfRigCamera(pairs[i], 1, B, cam_color[i], 2 * hw) for i in range(2)])
        cols = (TsdfRigColor * 2)(*[TsdfRigColor(*c) for c in colors])
        poses = np.stack([pose] * max(n, 1))
        return rg(r.h, ctypes.addressof(cams), ctypes.addressof(cols), 2, n, 0, poses.ctypes.data, None)

    ok = (B, 3 * hw, B, hw)
    before = (r.tsdf_read(), r.tsdf_read_color())
    assert rig(cam_color=(B, None)) == EINVAL and rig(cam_color=(None, B)) == EINVAL     # colour comes from the descriptors
    assert rig(colors=(ok, (None, 0, None, 0))) == EINVAL and rig(colors=((None, 0, None, 0), ok)) == EINVAL   # all or none
    for n in (1, 2):
        for bad in ((B, 3 * hw - 1, B, hw), (B, 0, B, hw), (B, -3 * hw, B, hw), (B, 3 * hw, B, hw - 1), (B, 3 * hw, B, -hw)):
            assert rig(colors=(ok, bad), n=n) == EINVAL and rig(colors=(bad, ok), n=n) == EINVAL, bad
    assert rig(pairs=(1, 0)) == EINVAL and rig(n=-1) == EINVAL
    after = (r.tsdf_read(), r.tsdf_read_color())
    assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y))   # a refused call changes nothing
    assert rig() == 0 and rig(n=2) == 0 and rig(colors=((B, 3 * hw, None, 0), (B, 3 * hw, None, 0))) == 0
    assert rig(colors=((None, 0, None, 0), (None, 0, None, 0))) == 0                      # none coloured: geometry only
    r.close()

    src = SyntheticRGBDSource(width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rgbd = Handle([rgbd_undistort(cams[ci])], HipSlamConfig(rgbd=True, **CFG), max_batch=1)
    assert init(prm(), hh=rgbd) == ESTATE
    rgbd.close()


def h_read(lib, h, dsize, csize):
    out = [np.zeros((csize[1], csize[0]), np.uint16), np.zeros((dsize[1], dsize[0], 3), np.uint8),
           np.zeros((dsize[1], dsize[0]), np.uint8)]
    assert lib.tslam_depth_register_read(h.h, 0, 0, *[o.ctypes.data for o in out]) == 0
    return out
