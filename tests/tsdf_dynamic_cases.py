"""The scenes the free-space mask's tests share (tests/test_tsdf_dynamic_cpu.py and
tests/test_gpu_tsdf_dynamic.py): the corner volume of ``tsdf_align_cases`` with its weights scaled to
8 (above the default gate of 5) and one slab of its free voxels at weight 2 (below it); two cameras
whose rows are one and two full 64-bit words plus 3 bits; frames that are the map rendered from
``T_STAR`` with objects composited by ray-sphere or ray-box intersection in the camera frame."""

from __future__ import annotations

import functools

import numpy as np

import ref_tsdf_dynamic as REF
import tsdf_align_cases as A

DIMS, S, TRUNC_VOX, TRUNC, ORIGIN = A.DIMS, A.S, A.TRUNC_VOX, A.TRUNC_VOX * A.S, A.ORIGIN
MAX_D, MAX_W = A.MAX_D, A.MAX_W
T_STAR, PERTURBED, NAN = A.T_STAR, A.PERTURBED, A.NAN
CAM = A.DEVICE_CAM                                 # 67 x 77: one full word plus 3 bits per row, partial tiles
CAM2 = (131, 69, 118.0, 118.0, 65.0, 34.0)         # two words plus 3 bits; about the same field of view
PRM = dict(REF.PRM)
RADII = ((0, 0), (4, 8), (PRM["open_radius"], PRM["dilate_radius"]))
WEIGHT, SLAB_WEIGHT = 8.0, 2.0
SLAB_J = (2, 6)                                    # voxel rows j of the weight-2 slab: y in [-0.625, -0.425)

SPHERE = ((0.25, -0.1, 1.55), 0.12)                # centre (camera frame) and radius: in free space in front of the corner
# a box (camera frame: x, y, z ranges) whose image spans columns 33 .. 66 of CAM, so 63, 64 and the
# last one, placed near the camera: the side wall is close at larger z
EDGE_BOX = ((0.336, 0.72), (-0.10, 0.02), (1.2, 1.3))
# a sphere inside the weight-2 slab: its points lie in y in [-0.585, -0.465] of the volume's frame
SLAB_SPHERE = (tuple((np.linalg.inv(T_STAR) @ np.array([-0.05, -0.525, 1.5, 1.0]))[:3]), 0.06)


def uniform_volume():
    """The same map without the slab: every observed voxel at weight 8."""
    t, w = A.corner()
    return t, (w * np.float32(WEIGHT)).astype(np.float32)


@functools.lru_cache(maxsize=1)
def volume():
    """(tsdf, weight) f32 [nz][ny][nx]: the corner scene seen 8 times, the slab seen twice."""
    t, w = A.corner()
    w = (w * np.float32(WEIGHT)).astype(np.float32)
    w[:, SLAB_J[0]:SLAB_J[1], :] = np.where(w[:, SLAB_J[0]:SLAB_J[1], :] > 0, np.float32(SLAB_WEIGHT), np.float32(0.0))
    w.setflags(write=False)
    return t, w


@functools.lru_cache(maxsize=4)
def static_depth(cam=CAM):
    """The map seen from T_STAR, u16 [H][W]."""
    d = A.render(volume(), T_STAR, cam=cam)["depth_mm"]
    d.setflags(write=False)
    return d


def _rays(cam):
    W, H, fx, fy, cx, cy = cam
    ys, xs = np.mgrid[0:int(H), 0:int(W)]
    return (xs - cx) / fx, (ys - cy) / fy


def _composite(depth, z):
    """The nearer of the static depth and an object's depth z (metres; inf: no hit); (image, object pixels)."""
    mm = np.floor(1000.0 * np.where(np.isfinite(z), z, 0.0) + 0.5)
    hit = np.isfinite(z) & (mm >= 1) & ((depth == 0) | (mm < depth))
    out = depth.copy()
    out[hit] = mm[hit].astype(np.uint16)
    return out, hit


def with_sphere(depth, cam, centre, radius):
    """The frame with a sphere in front of it: the first intersection of every pixel's ray (1 : dc)."""
    d0, d1 = _rays(cam)
    c = np.asarray(centre, np.float64)
    aa = d0 * d0 + d1 * d1 + 1.0
    bb = d0 * c[0] + d1 * c[1] + c[2]
    disc = bb * bb - aa * (c @ c - radius * radius)
    with np.errstate(invalid="ignore"):
        z = np.where(disc >= 0.0, (bb - np.sqrt(np.maximum(disc, 0.0))) / aa, np.inf)
    return _composite(depth, np.where(z > 0, z, np.inf))


def with_box(depth, cam, box):
    """The frame with an axis-aligned box (camera frame) in front of it: the slab test of every ray."""
    d0, d1 = _rays(cam)
    lo = np.full(d0.shape, 0.0)
    hi = np.full(d0.shape, np.inf)
    for d, (a, b) in ((d0, box[0]), (d1, box[1]), (np.ones_like(d0), box[2])):
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = a / d, b / d
        para = d == 0.0
        ta = np.where(para, np.where((a <= 0.0) & (0.0 <= b), -np.inf, np.inf), ta)
        tb = np.where(para, np.where((a <= 0.0) & (0.0 <= b), np.inf, -np.inf), tb)
        lo = np.maximum(lo, np.minimum(ta, tb))
        hi = np.minimum(hi, np.maximum(ta, tb))
    return _composite(depth, np.where((lo <= hi) & (lo > 0), lo, np.inf))


def chebyshev_grow(b, r):
    """The pixels within r (Chebyshev) of a set pixel."""
    return REF.dilation(b.astype(np.uint8), r).astype(bool)


def reference(depth, T=T_STAR, cam=CAM, vol=None, origin=ORIGIN, **kw):
    t, w = volume() if vol is None else vol
    return REF.dynamic_frame(t, w, origin, S, TRUNC, cam, depth, T, max_dist=MAX_D, **{**PRM, **kw})


def guarded(depth, T=T_STAR, cam=CAM, vol=None, origin=ORIGIN, **kw):
    t, w = volume() if vol is None else vol
    return REF.guarded(t, w, origin, S, TRUNC, cam, depth, T, max_dist=MAX_D, **{**PRM, **kw})
