"""NumPy restatement of the semi-global aggregation of the dense stereo matcher (rule 3a of
thor_slam_amd/stereo_depth.py), written from the rule alone: one whole-plane array operation per
sweep step, nothing shared with the device code.  The box volume, the winners and the depth are
tests/ref_stereo_depth.py's.  The device output must equal it bit for bit
(tests/test_gpu_stereo_sgm.py)."""

from __future__ import annotations

import numpy as np

from ref_stereo_depth import depth_from_disp32, volume, winners

# bit of the mask -> (axis of the sweep in an [H][W][D] volume, sweep direction)
PATHS = {1: (1, +1), 2: (1, -1), 4: (0, +1), 8: (0, -1)}


def path_volume(A: np.ndarray, p1: int, p2: int, bit: int) -> np.ndarray:
    """L_r [D][H][W] (int64) of one path over the aggregated volume A [D][H][W]."""
    axis, sign = PATHS[bit]
    V = np.moveaxis(np.asarray(A, np.int64), 0, -1)        # [H][W][D]
    V = np.moveaxis(V, axis, 0)                            # [steps][lines][D]
    if sign < 0:
        V = V[::-1]
    L = np.empty_like(V)
    L[0] = V[0]                                            # q outside the image
    big = np.int64(1) << 40
    for i in range(1, V.shape[0]):
        q = L[i - 1]
        M = q.min(-1, keepdims=True)
        dn = np.full_like(q, big)
        dn[:, 1:] = q[:, :-1] + p1                         # L_r(q, d - 1) + P1, absent at d = 0
        up = np.full_like(q, big)
        up[:, :-1] = q[:, 1:] + p1                         # L_r(q, d + 1) + P1, absent at d = D - 1
        L[i] = V[i] + np.minimum(np.minimum(q, dn), np.minimum(up, M + p2)) - M
    if sign < 0:
        L = L[::-1]
    return np.moveaxis(np.moveaxis(L, 0, axis), -1, 0)


def sgm_volume(A: np.ndarray, p1: int, p2: int, paths: int = 15) -> np.ndarray:
    """S [D][H][W] (int64): the sum of the enabled paths' L_r."""
    assert 0 <= p1 <= p2 and 1 <= paths <= 15
    S = np.zeros(A.shape, np.int64)
    for bit in PATHS:
        if paths & bit:
            S += path_volume(A, p1, p2, bit)
    return S


def sgm_winners(A: np.ndarray, S: np.ndarray, uniqueness: int, lr_tol: int) -> dict:
    """Rules 4 to 6 on S; rule 7's parabola through A at S's winner d1, the offset clamped to
    [-16, 16] (d1 need not minimise A).  d1, valid, off, disp32."""
    D = A.shape[0]
    w = winners(S, uniqueness, lr_tol)
    d1 = w["d1"]
    a0 = np.take_along_axis(A, np.clip(d1 - 1, 0, D - 1)[None], 0)[0]
    a1 = np.take_along_axis(A, d1[None], 0)[0]
    a2 = np.take_along_axis(A, np.clip(d1 + 1, 0, D - 1)[None], 0)[0]
    den = a0 - 2 * a1 + a2
    sub = (d1 >= 1) & (d1 <= D - 2) & (den > 0)
    off = np.where(sub, np.clip((32 * (a0 - a2) + den) // np.where(sub, 2 * den, 1), -16, 16), 0)   # // floors
    return {"d1": d1, "valid": w["valid"], "off": off, "disp32": np.where(w["valid"], 32 * d1 + off, 0)}


def stereo_depth_sgm(L: np.ndarray, R: np.ndarray, n_disp: int, fxb: float, p1: int, p2: int, paths: int = 15,
                     uniqueness: int = 10, lr_tol: int = 1):
    """(depth u16 mm, disp32 u16) of one rectified pair with semi-global aggregation."""
    A = volume(np.asarray(L, np.uint8), np.asarray(R, np.uint8), int(n_disp))
    w = sgm_winners(A, sgm_volume(A, int(p1), int(p2), int(paths)), int(uniqueness), int(lr_tol))
    return depth_from_disp32(w["disp32"], fxb), w["disp32"].astype(np.uint16)
