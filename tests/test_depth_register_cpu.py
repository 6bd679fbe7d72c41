"""Depth registration on the CPU: the rule of ``thor_slam_amd/depth_register.py`` as
``tests/ref_depth_register.py`` restates it, against its per-pixel definition, its properties, the
parameter checks, and what it does on scenes whose answer is known."""

import numpy as np
import pytest

import depth_register_cases as C
import ref_depth_register as R
from thor_slam_amd.depth_register import check_register_params, color_camera, compose_color_T_rect
from thor_slam_amd.params import HipSlamConfig

KEYS = ("depth", "bgr", "mask", "Z")


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("shape,distorted,T,max_splat", [
    ("up", False, C.OFFSET, 4), ("up", True, C.OFFSET, 2), ("up", False, C.OFFSET, 1), ("down", False, C.OFFSET, 4),
    ("ragged", True, C.BEHIND, 4), ("down", True, C.BEHIND, 8),
])
def test_restatement_equals_the_per_pixel_definition(shape, distorted, T, max_splat):
    dsize, csize = C.SHAPES[shape]
    ccam = C.color_cam(dsize, csize, C.DISTORTION if distorted else None)
    assert (ccam["map"] is not None) == distorted
    depth, color = C.depth_image(dsize, seed=3), C.color_image(csize, seed=3)
    got = R.register(depth, color, C.DEPTH_CAM, ccam, T, max_depth_mm=40000, tol_mm=50, max_splat=max_splat)
    want = R.register_brute(depth, color, C.DEPTH_CAM, ccam, T, max_depth_mm=40000, tol_mm=50, max_splat=max_splat)
    _same(got, want)
    assert got["mask"].any() and (got["depth"] > 0).any()
    if shape == "up" and max_splat == 4:
        # the footprints fill the image of twice the size: what stays empty is the 8 % of the depth
        # pixels the case makes invalid and the strip the box uncovers, not a grid of holes
        inner = got["depth"][40:100, 20:150]
        assert (inner > 0).mean() > 0.8
        assert (R.register(depth, color, C.DEPTH_CAM, ccam, T, max_depth_mm=40000, max_splat=1)["depth"][40:100, 20:150] > 0).mean() < 0.3


def test_minimum_does_not_depend_on_the_order():
    """(a): the z-buffer filled in a shuffled pixel order is the same, bit for bit."""
    dsize, csize = C.SHAPES["down"]
    ccam = C.color_cam(dsize, csize)
    depth, color = C.depth_image(dsize, seed=5), C.color_image(csize, seed=5)
    a = R.register_brute(depth, color, C.DEPTH_CAM, ccam, C.OFFSET)
    order = np.random.default_rng(9).permutation(dsize[0] * dsize[1])
    _same(a, R.register_brute(depth, color, C.DEPTH_CAM, ccam, C.OFFSET, order=order))
    _same(a, R.register(depth, color, C.DEPTH_CAM, ccam, C.OFFSET))
    # many depth pixels per colour pixel: the registered depth is the minimum of what landed
    assert (a["depth"][a["depth"] > 0] <= depth.max()).all()


@pytest.mark.parametrize("size", [(96, 64), (83, 51)])
def test_identity(size):
    """(b): equal intrinsics, the identity transform, no table."""
    W, H = size
    fx, fy, cx, cy = C.DEPTH_CAM
    ccam = {"width": W, "height": H, "f_c": fx, "cxc": cx, "cyc": cy, "map": None}
    depth, color = C.depth_image(size, seed=1), C.color_image(size, seed=1)
    out = R.register(depth, color, C.DEPTH_CAM, ccam, C.IDENTITY, max_depth_mm=40000, tol_mm=0)
    valid = (depth > 0) & (depth <= 40000)
    assert valid.any() and (~valid).any()
    assert np.array_equal(out["depth"], np.where(valid, depth, 0))
    assert np.array_equal(out["mask"], valid.astype(np.uint8))
    assert np.array_equal(out["bgr"], np.where(valid[..., None], color, 0))


def test_own_footprint_holds_the_nearest_pixel():
    """(c): a single surface with nothing in front of it is never masked, at any footprint cap, even
    with tol_mm = 0; what is masked out lies outside the colour image."""
    dsize, csize = C.SHAPES["up"]
    y, x = np.mgrid[0:dsize[1], 0:dsize[0]]
    depth = (1500 + 4 * x + 3 * y).astype(np.uint16)          # one slanted plane
    color = C.color_image(csize)
    for distorted in (False, True):
        ccam = C.color_cam(dsize, csize, C.DISTORTION if distorted else None)
        for ms in (1, 2, 3, 4, 8):
            out = R.register(depth, color, C.DEPTH_CAM, ccam, C.OFFSET, tol_mm=0, max_splat=ms)
            ok, zc, u, v, nu, nv, s = R._project(depth, C.DEPTH_CAM, ccam, C.OFFSET, 65535)
            inside = ok & (nu >= 0) & (nu < csize[0]) & (nv >= 0) & (nv < csize[1])
            # a slanted plane seen from slightly aside: a neighbour's footprint can put a depth that is a
            # few mm nearer on a pixel's nearest pixel, never one of another surface
            out50 = R.register(depth, color, C.DEPTH_CAM, ccam, C.OFFSET, tol_mm=50, max_splat=ms)
            assert np.array_equal(out50["mask"].reshape(-1), inside.astype(np.uint8))
            assert inside.sum() > 0.9 * inside.size
            Z = out["Z"].astype(np.int64).reshape(-1)
            assert (Z[(nv * csize[0] + nu)[inside]] <= zc[inside]).all()
            if ms == 1:   # every pixel splats its nearest pixel only: what it finds there is its own or nearer
                assert (out["mask"].reshape(-1)[inside & (zc == Z[np.where(inside, nv * csize[0] + nu, 0)])] == 1).all()


def test_parameter_checks():
    ok = dict(width=96, height=64, color_width=192, color_height=128, f_c=384.0, cxc=95.5, cyc=63.5, color_T_rect=C.IDENTITY)
    check_register_params(**ok)
    check_register_params(**ok, handle_size=(96, 64), max_splat=8, tol_mm=0, max_depth_mm=1, max_frames=65535)
    bad = [dict(width=15), dict(height=8), dict(color_width=0), dict(color_height=16385), dict(f_c=0.0), dict(f_c=float("nan")),
           dict(cxc=float("inf")), dict(color_T_rect=np.zeros(11)), dict(color_T_rect=np.full(12, np.nan)), dict(max_depth_mm=0),
           dict(max_depth_mm=65536), dict(tol_mm=-1), dict(max_splat=0), dict(max_splat=9), dict(max_frames=0),
           dict(max_frames=65536), dict(max_splat=2.0), dict(handle_size=(95, 64))]
    for kw in bad:
        with pytest.raises(ValueError):
            check_register_params(**{**ok, **kw})


def test_compose_color_T_rect():
    from scipy.spatial.transform import Rotation

    A = np.eye(4)
    A[:3, :3] = Rotation.from_rotvec([0.02, -0.3, 0.01]).as_matrix()
    A[:3, 3] = [0.0375, 0.002, -0.001]
    B = np.eye(4)
    B[:3, :3] = Rotation.from_rotvec([0.001, 0.004, -0.002]).as_matrix()
    T = compose_color_T_rect(A, B)
    assert np.allclose(T.reshape(3, 4), (np.linalg.inv(A) @ B)[:3], atol=1e-15)
    assert np.array_equal(compose_color_T_rect(np.eye(4)), C.IDENTITY)


def test_validate_rules():
    base = dict(stereo_depth=True, dense_map=True, stereo_color=True)
    HipSlamConfig(**base).validate()
    HipSlamConfig(**base, stereo_color_tol_m=0.1, stereo_color_max_dt=0.0).validate()
    assert HipSlamConfig().stereo_color is False and HipSlamConfig().stereo_color_tol_m is None
    assert HipSlamConfig().stereo_color_max_dt == 0.05
    for kw in (dict(stereo_depth=False, dense_map=False), dict(dense_map=False), dict(stereo_depth=False, rgbd=True),
               dict(devices=(0, 1)), dict(stereo_color_tol_m=-0.1), dict(stereo_color_max_dt=-1.0)):
        with pytest.raises(ValueError):
            HipSlamConfig(**{**base, **kw}).validate()
    with pytest.raises(ValueError, match="dense_align"):
        HipSlamConfig(**base, dense_align=True).validate()


def test_two_plane_occlusion():
    """A wall at 3 m with a box at 1 m in front of it, the colour camera 0.1 m to the right: per row
    the wall pixels behind the box's edge (seen by the depth camera, hidden from the colour camera)
    are a band of fx b (1 / z_near - 1 / z_far) = 12.8 pixels; nothing else is masked."""
    depth, ccam, T, band = C.occlusion_case()
    assert band >= 3.0
    color = C.color_image((ccam["width"], ccam["height"]))
    for tol in (0, 50):
        out = R.register(depth, color, C.DEPTH_CAM, ccam, T, tol_mm=tol)
        masked = out["mask"] == 0
        for row in masked:
            cols = np.nonzero(row)[0]
            assert abs(len(cols) - band) <= 1.0, len(cols)
            assert np.array_equal(cols, np.arange(cols[0], cols[0] + len(cols)))   # one band
            assert cols[-1] + 1 == 40   # the camera sits to the right: it loses the wall left of the box's left edge
        assert (depth[masked] == 3000).all()
        # the registered depth shows the box where the colour camera sees it, the wall elsewhere
        assert set(np.unique(out["depth"])) <= {0, 1000, 3000}
        assert np.array_equal(out["bgr"][masked], np.zeros((masked.sum(), 3), np.uint8))


def test_real_scene_registration():
    """A ``RoomScene`` seen by a stereo source with a centre colour camera (320 x 200 mono, 640 x 400
    colour, 0.0375 m apart): the left camera's noise-free depth, the colour camera's noise-free image
    registered to it, and the G channel of the result against the left camera's own noise-free
    render.  Median absolute difference over the masked-in pixels, in grey levels:

        registered (the calibrated extrinsic)    6.0
        the extrinsic ignored (identity)        34.0

    Both are deterministic; the registered figure is the smaller one."""
    from thor_slam_amd.synthetic import SyntheticStereoColorSource

    src = SyntheticStereoColorSource(width=320, height=200, color_width=640, color_height=400, seed=2, n_frames=4)
    left, z = src.scene.render(src.camera_pose(1, 0), src.get_intrinsics()[0], None, return_depth=True)
    mm = np.floor(z * 1000.0 + 0.5)
    depth = np.where((mm > 0) & (mm <= 65535), mm, 0).astype(np.uint16)
    color = src.render_color(1, noise=False)
    ccam = color_camera(src.get_rgbd_intrinsics()[0])
    k = np.asarray(src.get_intrinsics()[0].matrix)
    cam = (k[0, 0], k[1, 1], k[0, 2], k[1, 2])
    T = compose_color_T_rect(src.left_T_color().to_4x4_matrix())
    assert np.allclose(T.reshape(3, 4)[:, 3], [-0.0375, 0, 0])

    def mad(T):
        out = R.register(depth, color, cam, ccam, T)
        m = out["mask"] == 1
        assert m.mean() > 0.8
        return float(np.median(np.abs(out["bgr"][..., 1][m].astype(np.int64) - left[m].astype(np.int64))))

    reg, ign = mad(T), mad(C.IDENTITY)
    print(f"median |G - left|: registered {reg}, extrinsic ignored {ign}")
    assert reg < ign
    assert (reg, ign) == (REGISTERED_MAD, IGNORED_MAD)


REGISTERED_MAD, IGNORED_MAD = 6.0, 34.0   # as measured when the test was written
