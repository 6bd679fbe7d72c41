"""Rigid-transform and image helpers of the engine's host side, in plain NumPy."""

from __future__ import annotations

import math

import numpy as np


def bgr_to_gray(img: np.ndarray) -> np.ndarray:
    """8-bit BGR -> gray with the fixed-point BT.601 weights (R 4899, G 9617, B 1868) / 2^14."""
    if img.ndim == 2:
        return img
    b = img[..., 0].astype(np.int32)
    g = img[..., 1].astype(np.int32)
    r = img[..., 2].astype(np.int32)
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def adjoint(t: np.ndarray) -> np.ndarray:
    """SE(3) adjoint of a rigid 4x4 in the solver's (rho, omega) twist order: a left perturbation
    exp(xi) of a pose P becomes exp(Ad_T xi) of T P T^-1, so cov' = Ad cov Ad^T with
    Ad = [[R, [t]x R], [0, R]]."""
    r, tv = t[:3, :3], t[:3, 3]
    tx = np.array([[0.0, -tv[2], tv[1]], [tv[2], 0.0, -tv[0]], [-tv[1], tv[0], 0.0]])
    ad = np.zeros((6, 6))
    ad[:3, :3] = ad[3:, 3:] = r
    ad[:3, 3:] = tx @ r
    return ad


def _quat_xyzw(m: np.ndarray) -> np.ndarray:
    """(x, y, z, w) of a rotation matrix — scipy's ``Rotation.from_matrix(m).as_quat()`` formula
    (the largest of the diagonal and the trace picks the branch; bit-identical on orthonormal input,
    checked in tests/test_boundary.py) in plain floats: the per-frame publish path avoids scipy's
    ~30-60 us of validation per call."""
    m00, m01, m02 = float(m[0, 0]), float(m[0, 1]), float(m[0, 2])
    m10, m11, m12 = float(m[1, 0]), float(m[1, 1]), float(m[1, 2])
    m20, m21, m22 = float(m[2, 0]), float(m[2, 1]), float(m[2, 2])
    tr = m00 + m11 + m22
    d = (m00, m11, m22, tr)
    c = max(range(4), key=d.__getitem__)
    if c == 3:
        q = [m21 - m12, m02 - m20, m10 - m01, 1.0 + tr]
    else:
        M = ((m00, m01, m02), (m10, m11, m12), (m20, m21, m22))
        i = c
        j = (i + 1) % 3
        k = (j + 1) % 3
        q = [0.0, 0.0, 0.0, 0.0]
        q[i] = 1.0 - tr + 2.0 * M[i][i]
        q[j] = M[j][i] + M[i][j]
        q[k] = M[k][i] + M[i][k]
        q[3] = M[k][j] - M[j][k]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return np.array([q[0] / n, q[1] / n, q[2] / n, q[3] / n])


def _invert(t: np.ndarray) -> np.ndarray:
    out = np.eye(4)
    out[:3, :3] = t[:3, :3].T
    out[:3, 3] = -t[:3, :3].T @ t[:3, 3]
    return out
