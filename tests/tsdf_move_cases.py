"""The scenes the depth-archive tests share (tests/test_tsdf_move_cpu.py and
tests/test_gpu_tsdf_move.py): a wall with a nearer box in front of it, seen by
``tsdf_align_cases.DEVICE_CAM`` (67 x 77: partial tiles on both edges) from N poses along a short
arc, in a volume whose dimensions are off every multiple of the 16 x 4 x 4 brick.  The depth images
are rendered from the true poses; every second frame is first integrated on a pose that drifted by a
few centimetres and about 0.02 rad, and then moved to its true pose."""

from __future__ import annotations

import functools

import numpy as np

import ref_tsdf_move as REF
import tsdf_align_cases as AC

CAM = AC.DEVICE_CAM                      # W, H, fx, fy, cx, cy
INTR = CAM[2:]
DIMS = (37, 22, 35)
S, TRUNC_VOX = 0.05, 4.0
TRUNC = TRUNC_VOX * S
ORIGIN = (-0.925, -0.55, 1.0)
MAX_D = 10.0
WALL_Z = 2.3
BOX = ((-0.35, -0.2, 1.7), (0.15, 0.45, 2.3))   # min and max corner
MIN_T, MIN_R = 0.5 * S, 0.005            # the engine's defaults: half a voxel, 0.005 rad


def true_pose(i: int) -> np.ndarray:
    return AC.moved(np.eye(4), (0.03 * i - 0.08, 0.01 * (i % 3), 0.02 * i), (0.0, 0.012 * i - 0.03, 0.004 * i))


def drifted(T: np.ndarray, i: int) -> np.ndarray:
    sgn = 1.0 if i % 4 == 1 else -1.0
    return AC.moved(T, (0.03 * sgn, -0.02, 0.025), (0.012 * sgn, -0.014, 0.008))


def render_depth(T: np.ndarray) -> np.ndarray:
    """The scene's depth u16 mm [H][W] from world_T_cam T: the nearer of the wall and the box."""
    W, H, fx, fy, cx, cy = CAM
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))], axis=-1) @ T[:3, :3].T   # world direction per unit of depth
    C = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        best = (WALL_Z - C[2]) / d[..., 2]
        lo = (np.array(BOX[0]) - C) / d
        hi = (np.array(BOX[1]) - C) / d
    near, far = np.minimum(lo, hi).max(axis=-1), np.maximum(lo, hi).min(axis=-1)
    box = (near <= far) & (near > 0)
    best = np.where(box & (near < best), near, best)
    return np.clip(np.rint(best * 1000.0), 0, 65535).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def sequence(n: int):
    """(depth u16 [n][H][W], true poses [n][4][4], integrated poses [n][4][4]): every second frame drifted."""
    true = np.stack([true_pose(i) for i in range(n)])
    first = np.stack([drifted(true[i], i) if i % 2 else true[i] for i in range(n)])
    depth = np.stack([render_depth(T) for T in true])
    for a in (true, first, depth):
        a.setflags(write=False)
    return depth, true, first


def archive(max_weight: float, capacity: int, interval: int = 1, mp=None) -> REF.Archive:
    return REF.Archive(DIMS, ORIGIN, S, TRUNC, MAX_D, max_weight, INTR, capacity, interval, mp)


@functools.lru_cache(maxsize=None)
def moved_reference(n: int, max_weight: float, capacity: int | None = None):
    """The reference after integrating ``sequence(n)`` on the drifted poses and moving every frame to
    its true pose: (tsdf, weight, volume before the move, frames moved, the archive's entries), read-only."""
    depth, true, first = sequence(n)
    ar = archive(max_weight, capacity or n)
    ar.integrate(depth, 0, first)
    before = (ar.tsdf.copy(), ar.weight.copy())
    moved = ar.move(np.arange(n), true, MIN_T, MIN_R)
    for a in (ar.tsdf, ar.weight) + before:
        a.setflags(write=False)
    return ar.tsdf, ar.weight, before, moved, ar.entries()


def bound(n: int, moves: int) -> float:
    """|move - rebuild| per voxel in metres: an f32 rounding (2^-24 relative, of a value below trunc
    times the weight) per update, N + 2 moves updates, amplified by at most the weight ratio w_max = N."""
    return 4.0 * (n + 2 * moves) * n * TRUNC * 2.0 ** -24
