"""Inputs of the depth-registration tests (``tests/test_depth_register_cpu.py`` and
``tests/test_gpu_depth_register.py``): small synthetic depth / colour images, colour cameras and
transforms.  Everything is seeded and cheap; the references come from ``ref_depth_register``.

The depth camera is the rectified left camera of ``SyntheticStereoSource(width=320, height=240)``
(an undistorted pair: f = 0.6 W at the image centre), which is the handle the device tests run on;
a case's depth image is the top-left ``W x H`` part of it, as ``tslam_depth_register_init`` sizes it.
"""

from __future__ import annotations

import numpy as np

from thor_slam_amd.camera.types import Intrinsics
from thor_slam_amd.depth_register import color_camera

HANDLE_SIZE = (320, 240)
DEPTH_CAM = (192.0, 192.0, 159.5, 119.5)      # fx, fy, cx, cy of the handle's pair 0
DISTORTION = np.array([-0.12, 0.05, 0.0008, -0.0006, 0.01])

# depth size -> colour size
SHAPES = {
    "up": ((96, 64), (192, 128)),        # footprints of 2-3 pixels, the cap at max_splat 1, 2, 4
    "down": ((96, 64), (48, 32)),        # many depth pixels per colour pixel: the minimum must win
    "ragged": ((83, 51), (131, 77)),     # nothing a multiple of anything
}


def color_cam(dsize, csize, distortion=None, cam=DEPTH_CAM) -> dict:
    """A colour camera of ``csize`` pixels that looks where the ``dsize`` part of the depth camera
    looks (the depth camera's focal length scaled by the width ratio, pixel centres at integers)."""
    (W, H), (Wc, Hc) = dsize, csize
    ax, ay = Wc / W, Hc / H
    f = cam[0] * ax
    K = np.array([[f, 0.0, (cam[2] + 0.5) * ax - 0.5], [0.0, f, (cam[3] + 0.5) * ay - 0.5], [0.0, 0.0, 1.0]])
    coeffs = np.zeros(14)
    if distortion is not None:
        coeffs[:len(distortion)] = distortion
    return color_camera(Intrinsics(width=Wc, height=Hc, matrix=K, coeffs=coeffs))


def transform(t=(0.0, 0.0, 0.0), rot_y_deg=0.0, rot_x_deg=0.0) -> np.ndarray:
    """color_T_rect [12]: a rotation about y, then about x, and a translation."""
    a, b = np.deg2rad(rot_y_deg), np.deg2rad(rot_x_deg)
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return np.concatenate([Rx @ Ry, np.asarray(t, dtype=np.float64).reshape(3, 1)], axis=1).reshape(12)


IDENTITY = transform()
OFFSET = transform(t=(-0.0375, 0.004, 0.002), rot_y_deg=0.7, rot_x_deg=-0.4)   # a centre colour camera, slightly toed
# moved 1 m forward along the depth camera's view and turned: the box (0.8 m) falls behind the colour
# camera, much of the surface outside its image, the rest is seen with footprints of twice the size
BEHIND = transform(t=(0.55, 0.45, -1.0), rot_y_deg=-5.0)


def depth_image(size, seed=0, holes=True) -> np.ndarray:
    """u16 mm [H][W]: a rolling surface around 2 m, a box at 0.8 m in front of it, and (``holes``)
    invalid pixels: zeros, values above 40 m and 65535."""
    W, H = size
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    rng = np.random.default_rng(seed)
    z = 2000.0 + 350.0 * np.sin(x / 9.0 + seed) + 250.0 * np.cos(y / 7.0) + rng.integers(-20, 21, size=(H, W))
    z[H // 4: H // 4 + H // 3, W // 3: W // 3 + W // 4] = 800.0 + rng.integers(-5, 6, size=(H // 3, W // 4))
    d = z.astype(np.uint16)
    if holes:
        d[rng.random((H, W)) < 0.05] = 0
        d[rng.random((H, W)) < 0.02] = 45000
        d[rng.random((H, W)) < 0.01] = 65535
    return d


def color_image(size, seed=0) -> np.ndarray:
    """u8 [Hc][Wc][3], every pixel different from its neighbours (noise)."""
    Wc, Hc = size
    return np.random.default_rng(1000 + seed).integers(0, 256, size=(Hc, Wc, 3), dtype=np.uint8)


def occlusion_scene(size, z_far=3000, z_near=1000, box=(40, 60)) -> np.ndarray:
    """A fronto-parallel wall at ``z_far`` mm with a nearer box over the columns ``box``, every row."""
    W, H = size
    d = np.full((H, W), z_far, dtype=np.uint16)
    d[:, box[0]:box[1]] = z_near
    return d


def occlusion_case(size=(96, 64), b=0.1, margin=32):
    """The two-plane scene seen by a colour camera with the depth camera's focal length, ``b`` metres
    to its right and ``margin`` pixels wider, so that every depth pixel lands inside its image:
    (depth, colour camera, T, band width in pixels the geometry gives)."""
    W, H = size
    K = np.array([[DEPTH_CAM[0], 0.0, DEPTH_CAM[2] + margin / 2], [0.0, DEPTH_CAM[1], DEPTH_CAM[3]], [0.0, 0.0, 1.0]])
    ccam = color_camera(Intrinsics(width=W + margin, height=H, matrix=K, coeffs=np.zeros(14)))
    depth = occlusion_scene(size)
    band = DEPTH_CAM[0] * b * (1.0 / 1.0 - 1.0 / 3.0)
    return depth, ccam, transform(t=(-b, 0.0, 0.0)), band
