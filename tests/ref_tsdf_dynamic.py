"""An independent restatement of the free-space depth mask of thor_slam_amd/dense_dynamic.py (steps
1-6 of its docstring) for the tests: the volume indexed as [k][j][i], the morphology as the minimum /
maximum over shifted copies of a zero-padded image.  IEEE f64, one rounding per operation, sums in
the written order; NumPy's element-wise operations do that.

``thr_scale`` and ``weight_scale`` are the tests' guard: they scale ``thr`` and ``min_free_weight``
after they are formed, to show that no pixel of a scene sits on either gate."""

from __future__ import annotations

import numpy as np

OK, UNUSED = 0, 1
PRM = dict(min_free_weight=5.0, free_fraction=0.75, open_radius=1, dilate_radius=2)


def resample(depth_mm, cam, table=None):
    """Step 1: the depth on the rectified grid."""
    W, H = int(cam[0]), int(cam[1])
    d = np.asarray(depth_mm, np.uint16).reshape(H, W)
    if table is None:
        return d.copy()
    out = np.zeros((H, W), np.uint16)
    t = np.asarray(table, np.int32).reshape(H, W, 2)
    for y in range(H):
        for x in range(W):
            ix = min(max((int(t[y, x, 0]) + 16) >> 5, 0), W - 1)
            iy = min(max((int(t[y, x, 1]) + 16) >> 5, 0), H - 1)
            out[y, x] = d[iy, ix]
    return out


def _shifted(img, dy, dx):
    """img moved so that out[y][x] = img[y + dy][x + dx], zeros from outside."""
    H, W = img.shape
    out = np.zeros_like(img)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = img[ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def erosion(img, r):
    out = img.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out = np.minimum(out, _shifted(img, dy, dx))
    return out


def dilation(img, r):
    out = img.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out = np.maximum(out, _shifted(img, dy, dx))
    return out


def classify(tsdf, weight, origin, s, cam, mm, T, max_dist, min_free_weight, thr):
    """Steps 1-4: (valid, candidate) u8 [H][W]."""
    W, H, fx, fy, cx, cy = cam
    W, H = int(W), int(H)
    nz, ny, nx = tsdf.shape
    ys, xs = np.mgrid[0:H, 0:W]
    D = mm.astype(np.float64) * 0.001
    valid = (D > 0.0) & (D <= max_dist)
    dc0 = (xs.astype(np.float64) - float(cx)) / float(fx)
    dc1 = (ys.astype(np.float64) - float(cy)) / float(fy)
    pc0, pc1, pc2 = D * dc0, D * dc1, D
    R, C = T[:3, :3], T[:3, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        px = ((R[0, 0] * pc0 + R[0, 1] * pc1) + R[0, 2] * pc2) + C[0]
        py = ((R[1, 0] * pc0 + R[1, 1] * pc1) + R[1, 2] * pc2) + C[1]
        pz = ((R[2, 0] * pc0 + R[2, 1] * pc1) + R[2, 2] * pc2) + C[2]
        gi = np.floor((px - origin[0]) / s)
        gj = np.floor((py - origin[1]) / s)
        gk = np.floor((pz - origin[2]) / s)
        inside = (gi >= 0) & (gi <= nx - 1) & (gj >= 0) & (gj <= ny - 1) & (gk >= 0) & (gk <= nz - 1)
    i = np.where(inside, gi, 0).astype(np.intp)
    j = np.where(inside, gj, 0).astype(np.intp)
    k = np.where(inside, gk, 0).astype(np.intp)
    seen = weight[k, j, i].astype(np.float64) >= min_free_weight
    free = tsdf[k, j, i].astype(np.float64) >= thr
    return valid.astype(np.uint8), (valid & inside & seen & free).astype(np.uint8)


def dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm, world_T_cam, max_dist=10.0, table=None,
                  thr_scale=1.0, weight_scale=1.0, **params):
    prm = {**PRM, **params}
    tsdf = np.asarray(tsdf, np.float32)
    weight = np.asarray(weight, np.float32)
    T = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    mm = resample(depth_mm, cam, table)
    zero = np.zeros(mm.shape, np.uint8)
    if not np.isfinite(T[0, 0]):
        return {"mask": zero, "depth": mm, "stats": np.array([UNUSED, 0, 0, 0], np.int32), "valid": zero, "candidates": zero}
    thr = (float(prm["free_fraction"]) * float(trunc)) * thr_scale
    valid, cand = classify(tsdf, weight, [float(o) for o in origin], float(s), cam, mm, T, float(max_dist),
                           float(prm["min_free_weight"]) * weight_scale, thr)
    ro, rd = int(prm["open_radius"]), int(prm["dilate_radius"])
    mask = dilation(dilation(erosion(cand, ro), ro), rd)
    depth = mm.copy()
    depth[mask != 0] = 0
    stats = np.array([OK, int(valid.sum()), int(cand.sum()), int((valid & mask).sum())], np.int32)
    return {"mask": mask, "depth": depth, "stats": stats, "valid": valid, "candidates": cand}


def dynamic(tsdf, weight, origin, s, trunc, cam, depth_mm, poses, **kw):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    res = [dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm[f], poses[f], **kw) for f in range(len(poses))]
    return {k: np.stack([r[k] for r in res]) for k in res[0]}


def guarded(tsdf, weight, origin, s, trunc, cam, depth_mm, world_T_cam, **kw):
    """The guard: True when scaling thr or min_free_weight by 1 +- 1e-9 changes no candidate."""
    base = dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm, world_T_cam, **kw)["candidates"]
    for knob in ("thr_scale", "weight_scale"):
        for scale in (1.0 - 1e-9, 1.0 + 1e-9):
            other = dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm, world_T_cam, **{**kw, knob: scale})
            if not np.array_equal(other["candidates"], base):
                return False
    return True
