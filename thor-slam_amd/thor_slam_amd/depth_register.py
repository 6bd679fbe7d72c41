"""Depth registration: the depth of a pair's rectified left camera forward-warped into a colour
camera with a z-buffer (``tslam_depth_register_init`` / ``tslam_depth_register`` /
``tslam_depth_register_buffers`` / ``tslam_depth_register_read``; ``k_depth_register.hip``;
``HipSlamConfig.stereo_color``).  It is what a stereo camera does on board when it aligns its depth
to the centre colour camera (the reference's ``depth_align_to_rgb``), and it yields two products:
the depth aligned to the colour camera, and, for every depth pixel, the colour of the colour pixel
that sees it together with a mask that is 0 where a nearer surface hides it from the colour camera.
This file is the spec; ``tests/ref_depth_register.py`` restates it for the tests.

All arithmetic is IEEE f64, one rounding per written operation (no fused multiply-add), sums in the
written order ``((a0 b0 + a1 b1) + a2 b2) + t``.

* **Depth camera.**  ``W x H``, ``fx, fy, cx, cy`` (a pair's rectified left camera); depth ``D`` u16
  mm [H][W], 0 = invalid.  A pixel is *valid* when ``0 < D <= max_depth_mm``.
* **Colour camera.**  A raw BGR image u8 [Hc][Wc][3]; its undistorted pinhole ``f_c, cxc, cyc`` and
  the fixed-point table ``map`` i32 [Hc][Wc][2] (undistorted pixel -> raw pixel times 32) come from
  ``calib.rgbd_undistort`` (``color_camera`` below); no table when it is the identity.
* **Transform.**  ``T = color_T_rect``, 12 doubles, row-major 3 x 4 ``[R | t]``, composed once on
  the host (``compose_color_T_rect``).
* **1. Projection of a valid pixel (x, y).**  ``z = D * 0.001``;
  ``P = (((x - cx) / fx) * z, ((y - cy) / fy) * z, z)``;
  ``Q[r] = ((T[4r] P0 + T[4r+1] P1) + T[4r+2] P2) + T[4r+3]``; skipped unless ``Qz > 0``;
  ``zc = floor(Qz * 1000 + 0.5)``; skipped unless ``1 <= zc <= 65535``;
  ``u = f_c * Qx / Qz + cxc``, ``v = f_c * Qy / Qz + cyc`` (the expression form of
  ``k_tsdf_integrate``); the nearest pixel ``nu = floor(u + 0.5)``, ``nv = floor(v + 0.5)``.
* **2. Footprint.**  The depth pixel's half-widths in the colour image are
  ``hx = (0.5 * (f_c / fx)) * (z / Qz)`` and ``hy = (0.5 * (f_c / fy)) * (z / Qz)``.  Per axis (x
  shown) the pixel covers the colour pixels whose centres lie in ``[u - hx, u + hx)``:
  ``lo = max(ceil(u - hx), nu - 8)``, ``hi = min(ceil(u + hx) - 1, nu + 8)``; it always covers its
  nearest pixel: ``lo = min(lo, nu)``, ``hi = max(hi, nu)``; and at most ``max_splat`` (1..8)
  pixels: when ``hi - lo + 1 > max_splat`` the footprint is ``lo = nu - ((max_splat - 1) >> 1)``,
  ``hi = nu + (max_splat >> 1)``, centred on the nearest pixel.  (The bounds ``nu -+ 8`` change no
  result, they keep every value small: a footprint wider than 8 is clipped anyway.  For the same
  reason a pixel with ``nu < -8``, ``nu >= Wc + 8``, ``nv < -8`` or ``nv >= Hc + 8`` covers nothing.)
* **3. Splat.**  ``Z`` u32 [Hc][Wc] starts empty; for every valid projected pixel
  ``Z[iv][iu] = min(Z[iv][iu], zc)`` over ``lo_x <= iu <= hi_x``, ``lo_y <= iv <= hi_y`` inside
  the image.  ``Z`` is a minimum: the result does not depend on the order of the pixels.
* **4. Gather.**  For every valid pixel, ``zc``, ``nu``, ``nv`` again by the same operations.  The
  pixel is *visible* when it projects (rule 1), ``0 <= nu < Wc``, ``0 <= nv < Hc`` and
  ``zc - Z[nv][nu] <= tol_mm``.  Its colour is the raw pixel through the table, as
  ``k_tsdf_integrate`` samples: ``rx = clamp((map[nv][nu][0] + 16) >> 5, 0, Wc - 1)``, ``ry``
  likewise with ``Hc`` (no table: ``rx = nu, ry = nv``); ``bgr[y][x] = color[ry][rx]`` and
  ``mask[y][x] = 1``.  Every other pixel has ``bgr = 0, 0, 0`` and ``mask = 0``.
* **5. Registered depth.**  ``R[iv][iu] = Z[iv][iu]`` as u16 mm in the undistorted colour camera,
  0 where nothing landed.

What follows from the rule: (a) two runs are identical bit for bit; (b) with equal intrinsics, the
identity transform and no table, ``R == D`` where ``D <= max_depth_mm`` (0 elsewhere), ``bgr`` is
the colour image where ``D`` is valid and ``mask`` is 1 exactly there; (c) a pixel's own footprint
contains its nearest pixel, so ``Z[nv][nu] <= zc`` and a surface with nothing in front of it is
never masked.
"""

from __future__ import annotations

import math

import numpy as np

MAX_SPLAT = 8
MAX_IMAGE = 16384
MAX_FRAMES = 65535
DEFAULT_TOL_MM = 50       # one voxel of the default map
DEFAULT_MAX_SPLAT = 4


def check_register_params(width, height, color_width, color_height, f_c, cxc, cyc, color_T_rect,
                          max_depth_mm=65535, tol_mm=DEFAULT_TOL_MM, max_splat=DEFAULT_MAX_SPLAT, max_frames=1,
                          handle_size=None) -> None:
    """``tslam_depth_register_init`` refuses the same settings (``handle_size`` = (W, H) of the
    handle: the depth image is 16 .. that size per axis)."""
    for v in (width, height, color_width, color_height, max_depth_mm, tol_mm, max_splat, max_frames):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("sizes, max_depth_mm, tol_mm, max_splat and max_frames must be integers")
    if width < 16 or height < 16:
        raise ValueError("the depth image must be at least 16 x 16")
    if handle_size is not None and (width > handle_size[0] or height > handle_size[1]):
        raise ValueError("the depth image must not exceed the handle's size")
    if not (1 <= color_width <= MAX_IMAGE and 1 <= color_height <= MAX_IMAGE):
        raise ValueError(f"the colour image must be 1..{MAX_IMAGE} per axis")
    T = np.asarray(color_T_rect, dtype=np.float64).reshape(-1)
    if T.size != 12:
        raise ValueError("color_T_rect must hold 12 values (3 x 4, row-major)")
    vals = [float(f_c), float(cxc), float(cyc)] + [float(v) for v in T]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("f_c, cxc, cyc and color_T_rect must be finite")
    if not float(f_c) > 0:
        raise ValueError("f_c must be > 0")
    if not 1 <= max_depth_mm <= 65535:
        raise ValueError("max_depth_mm must be 1..65535")
    if not 0 <= tol_mm <= 65535:
        raise ValueError("tol_mm must be 0..65535")
    if not 1 <= max_splat <= MAX_SPLAT:
        raise ValueError(f"max_splat must be 1..{MAX_SPLAT}")
    if not 1 <= max_frames <= MAX_FRAMES:
        raise ValueError(f"max_frames must be 1..{MAX_FRAMES}")


def color_camera(intrinsics) -> dict:
    """The colour camera of the rule from its ``Intrinsics``, exactly as an RGB-D camera's
    (``calib.rgbd_undistort``): ``width``, ``height``, ``f_c``, ``cxc``, ``cyc`` and ``map`` (i32
    [Hc][Wc][2], or None when the table is the identity)."""
    from .calib import rgbd_undistort
    from .camera.types import Extrinsics
    from .slam.interface import CameraConfig

    u = rgbd_undistort(CameraConfig(intrinsics, Extrinsics(np.eye(3), np.zeros(3)), "color", 0))
    return {"width": int(u.width), "height": int(u.height), "f_c": float(u.fx), "cxc": float(u.cx), "cyc": float(u.cy),
            "map": None if u.is_identity else np.ascontiguousarray(u.map_left, dtype=np.int32)}


def compose_color_T_rect(left_T_color: np.ndarray, left_optical_T_rect: np.ndarray | None = None) -> np.ndarray:
    """``color_T_rect`` f64 [12] (3 x 4, row-major) from the colour camera's pose in the left
    camera's optical frame (``left_T_color``, 4 x 4) and the rectification's ``left_optical_T_rect``
    (None: identity): ``inverse(left_T_color) left_optical_T_rect``, rigid inverse, sums in index
    order.  Composed once; the restatement and the device take the same 12 numbers."""
    A = np.asarray(left_T_color, dtype=np.float64).reshape(4, 4)
    B = np.eye(4) if left_optical_T_rect is None else np.asarray(left_optical_T_rect, dtype=np.float64).reshape(4, 4)
    inv = np.eye(4)
    for r in range(3):
        for c in range(3):
            inv[r, c] = A[c, r]
        inv[r, 3] = -((A[0, r] * A[0, 3] + A[1, r] * A[1, 3]) + A[2, r] * A[2, 3])
    out = np.zeros(12)
    for r in range(3):
        for c in range(4):
            out[4 * r + c] = ((inv[r, 0] * B[0, c] + inv[r, 1] * B[1, c]) + inv[r, 2] * B[2, c]) + inv[r, 3] * B[3, c]
    return out
