"""The analytic scene the ray-casting tests share (tests/test_tsdf_render_cpu.py and
tests/test_gpu_tsdf_render.py): a tilted plane and a sphere written as a TSDF, with an unobserved
hole, seen from four poses by a camera whose image has partial 16 x 16 tiles on both edges and whose
centre pixel's ray is exactly (0, 0, 1)."""

from __future__ import annotations

import functools

import numpy as np

import ref_tsdf_render as REF

DIMS = (37, 13, 41)                      # off every multiple of the 16 x 4 x 4 brick and of 4
S, TRUNC_VOX = 0.05, 4.0
TRUNC = TRUNC_VOX * S
ORIGIN = (-0.925, -0.325, 1.0)
CAM = (67, 45, 60.0, 150.0, 33.0, 22.0)  # W, H, fx, fy, cx, cy
PLANE_P, PLANE_N = np.array([0.0, 0.0, 2.7]), np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
SPHERE_C, SPHERE_R = np.array([0.1, 0.0, 2.0]), 0.22
HOLE = (slice(10, 16), slice(3, 9), slice(20, 30))     # [k][j][i]: i 20..29, j 3..8, k 10..15
PRM = dict(min_weight=1e-4, min_depth=0.0, max_depth=10.0, step_scale=0.5)


def centres(dims=DIMS, origin=ORIGIN, s=S):
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([origin[0] + s * (i + 0.5), origin[1] + s * (j + 0.5), origin[2] + s * (k + 0.5)], axis=-1)


def volume(dims=DIMS, sphere=True, hole=True):
    """(tsdf, weight) f32 [nz][ny][nx]: min(plane, sphere) clamped to the truncation; weight 1,
    0 deeper than the truncation behind a surface and 0 in the hole."""
    p = centres(dims)
    d = (p - PLANE_P) @ PLANE_N
    if sphere:
        d = np.minimum(d, np.linalg.norm(p - SPHERE_C, axis=-1) - SPHERE_R)
    weight = np.where(d < -TRUNC, 0.0, 1.0).astype(np.float32)
    if hole:
        weight[HOLE] = 0.0
    return np.clip(d, -TRUNC, TRUNC).astype(np.float32), weight


def color_layer(dims=DIMS, seed=7):
    """(colour f32 [nz][ny][nx][3] in [0, 255], colour weight f32 with a third of it 0)."""
    rng = np.random.default_rng(seed)
    shape = dims[::-1]
    col = rng.uniform(0.0, 255.0, size=shape + (3,)).astype(np.float32)
    cw = np.where(rng.random(shape) < 0.33, 0.0, rng.uniform(0.5, 20.0, size=shape)).astype(np.float32)
    return col, cw


def pose(t=(0.0, 0.0, 0.0), yaw_deg=0.0):
    """world_T_cam: a rotation about y (down) by yaw, then the centre t."""
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
    T[:3, 3] = t
    return T


OUTSIDE = pose()                                   # in front of the volume: the slab clip
INSIDE = pose((0.3, 0.05, 1.4), 20.0)
AWAY = pose((0.0, 0.0, 0.0), 180.0)
IN_SPHERE = pose((0.1, 0.0, 2.0))                  # starts unobserved / negative; the back face is no hit
VIEWS = (OUTSIDE, INSIDE, AWAY, IN_SPHERE)
NAN = np.full((4, 4), np.nan)


@functools.lru_cache(maxsize=4)
def reference(dims=DIMS, color=False, cam=CAM):
    """The reference of the four views on the analytic volume, computed once (read-only)."""
    tsdf, weight = volume(dims)
    kw = dict(PRM)
    if color:
        kw["color"], kw["color_weight"] = color_layer(dims)
    out = REF.render(tsdf, weight, ORIGIN, S, cam, np.stack(VIEWS), **kw)
    for v in out.values():
        v.setflags(write=False)
    return out


def check_not_empty(ref, views=VIEWS):
    """The conditions that keep a comparison from being empty, asserted on the reference."""
    hit = ref["depth_m"] > 0
    frac = hit.reshape(hit.shape[0], -1).mean(axis=1)
    for v, T in enumerate(views):
        if T is AWAY:
            assert frac[v] == 0.0
        else:
            assert frac[v] >= 0.25, (v, frac)
        if T is OUTSIDE or T is INSIDE:
            assert frac[v] <= 0.75, (v, frac)
    nz = np.any(ref["normal"] != 0, axis=-1)
    assert (hit & nz).any() and (hit & ~nz).any()
    return frac
