"""Dynamic objects kept out of the dense map: the free-space depth mask
(``tslam_tsdf_dynamic_init`` / ``tslam_tsdf_dynamic`` / ``tslam_tsdf_dynamic_buffers`` /
``tslam_tsdf_dynamic_read``; ``k_tsdf_dynamic.hip``; ``HipSlamConfig.dense_dynamic``).  Depth that
lands in voxels the map has reliably seen empty is treated as a moving object and kept out of the
reconstruction (the job of nvblox's dynamic mode).  This file is the spec, a NumPy reference of every
operation the device performs, restated for the tests in ``tests/ref_tsdf_dynamic.py``.

All arithmetic is IEEE f64, one rounding per written operation (no fused multiply-add), sums in the
written order.  Images and voxels are widened on load.

* **Inputs** per frame: the pose ``T = world_T_cam = (R, C)`` in the volume's frame and its use flag
  (a host pose whose first element is not finite, or an untracked batch frame: UNUSED, as in
  ``dense_render.py``); the depth image u16 [H][W] in millimetres; the pair's rectified camera
  ``W, H, fx, fy, cx, cy``; for a raw RGB-D camera its undistortion table i32 [H][W][2] (5 fractional
  bits); the volume ``tsdf`` / ``weight`` f32 [nz][ny][nx], its voxel size ``s`` and its *effective*
  origin ``o`` (under a rolling window ``o[a] = origin[a] + s * float(shift[a])``,
  thor_slam_amd/dense_follow.py); ``max_dist`` and ``trunc = trunc_vox * s`` of the volume.
* **Parameters**: ``min_free_weight`` > 0; ``free_fraction`` in (0, 1]; ``open_radius`` 0..4;
  ``dilate_radius`` 0..8.  ``thr = free_fraction * trunc``, computed once.
* **1. Lookup.**  Pixel (x, y) of the rectified grid reads ``(ix, iy) = (x, y)``, or through the
  table ``clamp((map[y][x][k] + 16) >> 5, 0, size - 1)`` (``k_tsdf_integrate``'s lookup).
  ``mm = depth[iy][ix]``, ``D = mm * 0.001``; the pixel is *valid* when ``0 < D <= max_dist``.
* **2. Point.**  ``dc = ((x - cx) / fx, (y - cy) / fy)``, ``pc = (D dc0, D dc1, D)``,
  ``p[a] = ((R[a][0] pc0 + R[a][1] pc1) + R[a][2] pc2) + C[a]`` (rule 2 of ``dense_align.py``).
* **3. Voxel.**  ``g[a] = floor((p[a] - o[a]) / s)``; the point is *inside* when
  ``0 <= g[a] <= n[a] - 1`` on all three axes, tested in floating point (a NaN is outside);
  ``v = (g2 * ny + g1) * nx + g0``.
* **4. Candidate**: valid, inside, ``weight[v] >= min_free_weight`` and ``tsdf[v] >= thr``; while
  the free-space layer exists (thor_slam_amd/dense_freespace.py) also ``settled(layer[v]) == 0``.
* **5. Clean-up** with squares of side ``2 r + 1``; everything outside the image counts as 0 in every
  step.  ``E`` = erosion of the candidates by ``open_radius``; ``O`` = dilation of ``E`` by
  ``open_radius``; ``M`` = dilation of ``O`` by ``dilate_radius``.  A radius of 0 is the identity.
* **6. Outputs** per frame: ``mask`` u8 [H][W] = M (0 or 1); ``depth`` u16 [H][W] = ``M ? 0 : mm``,
  always on the rectified grid (an empty mask gives the looked-up input bit for bit); ``stats`` i32
  [4] = status (0 OK, 1 UNUSED), valid pixels, candidates, valid pixels under M.  An UNUSED frame has
  ``mask`` 0, ``depth = mm`` and counts of 0.

The frames of a call are all judged against the volume as it stands before any of them is integrated.

An object that comes to rest in known free space is released to the map by the free-space layer
(``dense_freespace.py``; opt-in): without it the rule has no memory and such an object stays masked.

Out of scope: TSDF decay, colour, rigs, aligned and archived integration, sharded engines,
connected-component size filters.
"""

from __future__ import annotations

import math

import numpy as np

OK, UNUSED = 0, 1
MAX_OPEN, MAX_DILATE = 4, 8
MAX_FRAMES = 256                                                   # TSDF_MAX_FRAMES
DEFAULTS = dict(min_free_weight=5.0, free_fraction=0.75, open_radius=1, dilate_radius=2)


def check_dynamic_params(min_free_weight, free_fraction, open_radius, dilate_radius, max_frames=1) -> None:
    """``tslam_tsdf_dynamic_init`` refuses the same settings."""
    for v in (open_radius, dilate_radius, max_frames):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("open_radius, dilate_radius and max_frames must be integers")
    for v in (min_free_weight, free_fraction):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError("min_free_weight and free_fraction must be finite numbers")
    if not float(min_free_weight) > 0:
        raise ValueError("min_free_weight must be > 0")
    if not 0 < float(free_fraction) <= 1:
        raise ValueError("free_fraction must be in (0, 1]")
    if not 0 <= open_radius <= MAX_OPEN:
        raise ValueError(f"open_radius must be 0..{MAX_OPEN}")
    if not 0 <= dilate_radius <= MAX_DILATE:
        raise ValueError(f"dilate_radius must be 0..{MAX_DILATE}")
    if not 1 <= max_frames <= MAX_FRAMES:
        raise ValueError(f"max_frames must be 1..{MAX_FRAMES}")


def lookup(depth_mm, cam, undistort=None) -> np.ndarray:
    """Step 1: ``mm`` u16 [H][W] on the rectified grid."""
    W, H = int(cam[0]), int(cam[1])
    d = np.asarray(depth_mm, dtype=np.uint16).reshape(H, W)
    if undistort is None:
        return d.copy()
    mp = np.asarray(undistort, dtype=np.int32).reshape(H, W, 2)
    return d[np.clip((mp[..., 1] + 16) >> 5, 0, H - 1), np.clip((mp[..., 0] + 16) >> 5, 0, W - 1)]


def candidates(tsdf, weight, origin, s, cam, mm, T, max_dist, min_free_weight, thr, layer=None):
    """Steps 1-4 on the looked-up image: (valid [H][W], candidate [H][W]), booleans.  ``layer``: the
    free-space words u32 [nz][ny][nx] (bit 16: settled), or None."""
    W, H, fx, fy, cx, cy = int(cam[0]), int(cam[1]), *[float(v) for v in cam[2:]]
    nz, ny, nx = tsdf.shape
    s = float(s)
    D = mm.astype(np.float64) * 0.001
    valid = (D > 0.0) & (D <= float(max_dist))
    dc0 = ((np.arange(W, dtype=np.float64) - cx) / fx)[None, :]
    dc1 = ((np.arange(H, dtype=np.float64) - cy) / fy)[:, None]
    pc = (D * dc0, D * dc1, D)
    inside = np.ones((H, W), dtype=bool)
    g = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a, n in enumerate((nx, ny, nz)):
            p = ((T[a, 0] * pc[0] + T[a, 1] * pc[1]) + T[a, 2] * pc[2]) + T[a, 3]
            ga = np.floor((p - float(origin[a])) / s)
            inside &= (ga >= 0.0) & (ga <= float(n - 1))
            g.append(ga)
    g = [np.where(inside, ga, 0.0).astype(np.int64) for ga in g]
    v = (g[2] * ny + g[1]) * nx + g[0]
    w = weight.reshape(-1)[v].astype(np.float64)
    t = tsdf.reshape(-1)[v].astype(np.float64)
    cand = valid & inside & (w >= float(min_free_weight)) & (t >= float(thr))
    if layer is not None:
        cand &= (np.asarray(layer, dtype=np.uint32).reshape(-1)[v] & np.uint32(0x10000)) == 0
    return valid, cand


def _window_counts(b: np.ndarray, r: int) -> np.ndarray:
    """How many set pixels the (2r + 1)-square around every pixel holds; outside the image: none."""
    H, W = b.shape
    c = np.zeros((H + 2 * r + 1, W + 2 * r + 1), dtype=np.int64)
    c[r + 1:r + 1 + H, r + 1:r + 1 + W] = b
    c = c.cumsum(axis=0).cumsum(axis=1)
    k = 2 * r + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def erode(b: np.ndarray, r: int) -> np.ndarray:
    return b.copy() if r == 0 else _window_counts(b, r) == (2 * r + 1) ** 2


def dilate(b: np.ndarray, r: int) -> np.ndarray:
    return b.copy() if r == 0 else _window_counts(b, r) > 0


def clean(cand: np.ndarray, open_radius: int, dilate_radius: int) -> np.ndarray:
    """Step 5: M [H][W], boolean."""
    return dilate(dilate(erode(cand, open_radius), open_radius), dilate_radius)


def dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm, world_T_cam, max_dist=10.0, undistort=None,
                  layer=None, **params) -> dict:
    """One frame: ``mask`` u8 [H][W], ``depth`` u16 [H][W], ``stats`` i32 [4]; for the tests and
    measurements also ``valid`` and ``candidates`` (booleans [H][W])."""
    prm = {**DEFAULTS, **params}
    check_dynamic_params(**prm)
    H, W = int(cam[1]), int(cam[0])
    tsdf = np.asarray(tsdf, dtype=np.float32)
    weight = np.asarray(weight, dtype=np.float32)
    T = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    mm = lookup(depth_mm, cam, undistort)
    none = np.zeros((H, W), dtype=bool)
    if not math.isfinite(T[0, 0]):
        return {"mask": none.astype(np.uint8), "depth": mm, "stats": np.array([UNUSED, 0, 0, 0], np.int32),
                "valid": none, "candidates": none}
    thr = float(prm["free_fraction"]) * float(trunc)
    valid, cand = candidates(tsdf, weight, origin, s, cam, mm, T, max_dist, prm["min_free_weight"], thr, layer)
    M = clean(cand, prm["open_radius"], prm["dilate_radius"])
    return {"mask": M.astype(np.uint8), "depth": np.where(M, 0, mm).astype(np.uint16),
            "stats": np.array([OK, valid.sum(), cand.sum(), (valid & M).sum()], np.int32), "valid": valid, "candidates": cand}


def dynamic(tsdf, weight, origin, s, trunc, cam, depth_mm, poses, **kw) -> dict:
    """``dynamic_frame`` of every frame, stacked: ``depth_mm`` [n][H][W], ``poses`` [n][4][4]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    res = [dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm[i], poses[i], **kw) for i in range(poses.shape[0])]
    return {k: np.stack([r[k] for r in res]) for k in ("mask", "depth", "stats", "valid", "candidates")}
