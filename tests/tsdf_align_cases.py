"""The analytic scenes the alignment tests share (tests/test_tsdf_align_cpu.py and
tests/test_gpu_tsdf_align.py): a corner of three mutually non-parallel planes (floor, back wall,
tilted side wall) with a sphere, written as a TSDF, which fixes all six degrees of freedom; a single
fronto-parallel plane, which fixes three; a true pose ``T_STAR`` and initial poses about 1.5 cm and
1 degree off it on mixed axes.  A frame's input depth is the ``depth_mm`` the map renders from
``T_STAR``.  The camera's image has partial 16 x 16 tiles on both edges."""

from __future__ import annotations

import functools

import numpy as np

import ref_tsdf_align as REF
import ref_tsdf_render as RR

DIMS = (37, 29, 41)                      # off every multiple of the 16 x 4 x 4 brick and of 4
S, TRUNC_VOX = 0.05, 4.0
TRUNC = TRUNC_VOX * S
ORIGIN = (-0.925, -0.725, 1.0)
CAM = (67, 45, 60.0, 60.0, 33.0, 22.0)   # W, H, fx, fy, cx, cy
# The device aligns with a handle's own camera, and a handle takes no image below 64 pixels a side:
# the same camera with 32 more rows (partial tiles on both edges still: 67 = 64 + 3, 77 = 64 + 13)
DEVICE_CAM = (67, 77, 60.0, 60.0, 33.0, 38.0)
MAX_D, MAX_W = 10.0, 100.0
PRM = dict(REF.PRM)                      # the defaults; max_distance = two voxels


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


# (a point, the normal into free space); y points down
FLOOR = (np.array([0.0, 0.45, 0.0]), _unit([0.0, -1.0, 0.0]))
BACK = (np.array([0.0, 0.0, 2.7]), _unit([0.1, 0.0, -1.0]))
SIDE = (np.array([0.7, 0.0, 2.0]), _unit([-1.0, 0.0, -0.3]))
SPHERE_C, SPHERE_R = np.array([-0.15, 0.1, 2.0]), 0.22
FRONTO = (np.array([0.0, 0.0, 2.5]), np.array([0.0, 0.0, -1.0]))


def centres(dims=DIMS, origin=ORIGIN, s=S):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([origin[0] + s * (i + 0.5), origin[1] + s * (j + 0.5), origin[2] + s * (k + 0.5)], axis=-1)


def _tsdf(d):
    return np.clip(d, -TRUNC, TRUNC).astype(np.float32), np.where(d < -TRUNC, 0.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=1)
def corner():
    """(tsdf, weight) f32 [nz][ny][nx] of the corner scene: the nearest surface's signed distance."""
    p = centres()
    d = np.linalg.norm(p - SPHERE_C, axis=-1) - SPHERE_R
    for q, n in (FLOOR, BACK, SIDE):
        d = np.minimum(d, (p - q) @ n)
    t, w = _tsdf(d)
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


@functools.lru_cache(maxsize=1)
def plane():
    """(tsdf, weight) of the single fronto-parallel plane."""
    t, w = _tsdf((centres() - FRONTO[0]) @ FRONTO[1])
    t.setflags(write=False)
    w.setflags(write=False)
    return t, w


def empty():
    return np.zeros(DIMS[::-1], np.float32), np.zeros(DIMS[::-1], np.float32)


def rodrigues(w):
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th == 0.0:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * (K @ K)


def moved(T, t, w):
    """T with a left perturbation (rotation vector w, translation t) in the volume's frame."""
    M = np.eye(4)
    M[:3, :3] = rodrigues(w)
    M[:3, 3] = t
    return M @ T


T_STAR = moved(np.eye(4), (0.04, -0.03, 0.08), np.deg2rad([1.5, -3.0, 2.0]))
DEG = np.pi / 180.0
# about 1.5 cm and 1 degree, every axis in some frame
PERTURBED = (moved(T_STAR, (0.010, -0.008, 0.007), (0.6 * DEG, -0.5 * DEG, 0.6 * DEG)),
             moved(T_STAR, (-0.009, 0.009, -0.008), (-0.5 * DEG, 0.7 * DEG, 0.5 * DEG)),
             moved(T_STAR, (0.007, 0.010, 0.009), (0.7 * DEG, 0.6 * DEG, -0.4 * DEG)))
NAN = np.full((4, 4), np.nan)
FIVE = np.stack([PERTURBED[0], PERTURBED[1], T_STAR, NAN, PERTURBED[2]])   # three perturbed, the true pose, a NaN pose


def render(vol, T, cam=CAM, origin=ORIGIN):
    """The reference's view of a volume with the align parameters' marching rule."""
    return RR.render_view(vol[0], vol[1], origin, S, cam, T, min_weight=PRM["min_weight"], min_depth=0.0,
                          max_depth=PRM["max_depth"], step_scale=PRM["step_scale"])


@functools.lru_cache(maxsize=1)
def corner_depth():
    """The input depth u16 [H][W] of every corner-scene frame: the map seen from T_STAR."""
    d = render(corner(), T_STAR)["depth_mm"]
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=1)
def corner_reference():
    """The reference on the five frames, computed once (read-only)."""
    t, w = corner()
    depth = np.stack([corner_depth()] * 5)
    out = REF.align(t, w, ORIGIN, S, CAM, depth, FIVE, max_dist=MAX_D, **PRM)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def pose_error(T, T_ref=T_STAR):
    """(translation error in metres, rotation error in radians) of T against T_ref."""
    d = T @ np.linalg.inv(T_ref)
    c = np.clip((np.trace(d[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(T[:3, 3] - T_ref[:3, 3])), float(np.arccos(c))
