"""NumPy restatement of the dense stereo matcher (spec: thor_slam_amd/stereo_depth.py), written
from the rules alone: whole-volume array operations, nothing shared with the device code.  The
device output must equal it bit for bit (tests/test_gpu_stereo_depth.py)."""

from __future__ import annotations

import numpy as np

BIG = 1 << 30


def census(img: np.ndarray) -> np.ndarray:
    """48-bit census 7x7 (u64), replicated border, bit = neighbour < centre."""
    H, W = img.shape
    p = np.pad(img, 3, mode="edge").astype(np.int16)
    ctr = p[3:3 + H, 3:3 + W]
    c = np.zeros((H, W), np.uint64)
    k = 0
    for j in range(7):
        for i in range(7):
            if i == 3 and j == 3:
                continue
            c |= (p[j:j + H, i:i + W] < ctr).astype(np.uint64) << np.uint64(k)
            k += 1
    return c


def popcount(x: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(-1).astype(np.int64)


def volume(L: np.ndarray, R: np.ndarray, D: int) -> np.ndarray:
    """Aggregated cost A [D][H][W] (int64)."""
    H, W = L.shape
    cl, cr = census(L), census(R)
    C = np.full((D, H, W), 48, np.int64)
    for d in range(min(D, W)):
        C[d, :, d:] = popcount(cl[:, d:] ^ cr[:, :W - d])
    P = np.pad(C, ((0, 0), (2, 2), (2, 2)), mode="edge")
    A = np.zeros((D, H, W), np.int64)
    for j in range(5):
        for i in range(5):
            A += P[:, j:j + H, i:i + W]
    return A


def winners(A: np.ndarray, uniqueness: int, lr_tol: int) -> dict:
    """Rules 4-7 on an aggregated volume: d1, m1, m2, dR, off, valid, disp32."""
    D, H, W = A.shape
    d1 = A.argmin(0)                       # first (smallest) d among the minima
    m1 = A.min(0)
    dd = np.arange(D)[:, None, None]
    m2 = np.where(np.abs(dd - d1[None]) > 1, A, BIG).min(0)
    AR = np.full((D, H, W), BIG, np.int64)
    for d in range(min(D, W)):
        AR[d, :, :W - d] = A[d, :, d:]
    dR = AR.argmin(0)
    xs = np.arange(W)[None, :] - d1
    ys = np.broadcast_to(np.arange(H)[:, None], (H, W))
    valid = (d1 >= 1) & (m1 * 100 <= m2 * (100 - uniqueness)) & (xs >= 0)
    valid &= np.abs(dR[ys, np.clip(xs, 0, W - 1)] - d1) <= lr_tol
    inner = (d1 >= 1) & (d1 <= D - 2)
    c0 = np.take_along_axis(A, np.clip(d1 - 1, 0, D - 1)[None], 0)[0]
    c2 = np.take_along_axis(A, np.clip(d1 + 1, 0, D - 1)[None], 0)[0]
    den = c0 - 2 * m1 + c2
    sub = inner & (den > 0)
    off = np.where(sub, (32 * (c0 - c2) + den) // np.where(sub, 2 * den, 1), 0)   # // floors
    disp32 = np.where(valid, 32 * d1 + off, 0)
    return {"d1": d1, "m1": m1, "m2": m2, "dR": dR, "off": off, "valid": valid, "disp32": disp32}


def depth_from_disp32(disp32: np.ndarray, fxb: float) -> np.ndarray:
    ok = disp32 > 0
    mm = np.floor((np.float64(fxb) * 32000.0) / np.where(ok, disp32, 1).astype(np.float64) + 0.5)
    return np.where(ok & (mm <= 65535), mm, 0).astype(np.uint16)


def stereo_depth(L: np.ndarray, R: np.ndarray, n_disp: int, fxb: float, uniqueness: int = 10, lr_tol: int = 1):
    """(depth u16 mm, disp32 u16) of one rectified pair."""
    w = winners(volume(np.asarray(L, np.uint8), np.asarray(R, np.uint8), int(n_disp)), int(uniqueness), int(lr_tol))
    return depth_from_disp32(w["disp32"], fxb), w["disp32"].astype(np.uint16)
