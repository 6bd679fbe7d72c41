"""An independent restatement of the free-space layer of thor_slam_amd/dense_freespace.py for the
tests: the voxels as one flat list in storage order, cam_T_world as a 4 x 4 matrix filled element by
element, ``run`` and ``settled`` kept as two arrays and packed at the end, and the mask's extra term
applied on top of tests/ref_tsdf_dynamic.py.  IEEE f64, one rounding per operation, sums in the
written order; NumPy's element-wise operations do that.

``band_scale`` is the tests' guard: it scales ``band`` after it is formed, to show that no voxel of a
scene sits on either gate of the band."""

from __future__ import annotations

import numpy as np

import ref_tsdf_dynamic as REF

NONE, OCCUPIED, FREE = 0, 1, 2
RUN_BITS, SETTLED_BIT, SATURATED = 16, 1 << 16, (1 << 16) - 1


def pack(run, settled):
    return (np.asarray(run, np.uint32) | (np.asarray(settled, bool).astype(np.uint32) << RUN_BITS)).astype(np.uint32)


def unpack(words):
    w = np.asarray(words, np.uint32)
    assert not (w >> (RUN_BITS + 1)).any(), "bits above 16"
    return (w & SATURATED).astype(np.int64), ((w >> RUN_BITS) & 1).astype(bool)


def inverse_pose(T):
    """cam_T_world with k_tsdf_poses' expression order."""
    q = np.eye(4)
    for r in range(3):
        for k in range(3):
            q[r, k] = T[k, r]
        q[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return q


def observations(dims, origin, s, cam, depth_mm, world_T_cam, max_dist, band, table=None, sdf_out=None):
    """What every voxel sees in one frame: i8 [nz][ny][nx] of NONE / OCCUPIED / FREE."""
    W, H, fx, fy, cx, cy = cam
    W, H = int(W), int(H)
    nx, ny, nz = (int(n) for n in dims)
    T = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    out = np.zeros(nx * ny * nz, np.int8)
    if not np.isfinite(T[0, 0]):
        return out.reshape(nz, ny, nx)
    q = inverse_pose(T)
    flat = np.arange(nx * ny * nz)
    i, j, k = flat % nx, (flat // nx) % ny, flat // (nx * ny)
    X = float(origin[0]) + float(s) * (i + 0.5)
    Y = float(origin[1]) + float(s) * (j + 0.5)
    Z = float(origin[2]) + float(s) * (k + 0.5)
    pz = ((q[2, 0] * X + q[2, 1] * Y) + q[2, 2] * Z) + q[2, 3]
    px = ((q[0, 0] * X + q[0, 1] * Y) + q[0, 2] * Z) + q[0, 3]
    py = ((q[1, 0] * X + q[1, 1] * Y) + q[1, 2] * Z) + q[1, 3]
    depth = np.asarray(depth_mm, np.uint16).reshape(H, W)
    # the voxels that survive each step, narrowed step by step
    v = np.nonzero(pz > 0.0)[0]
    fu = np.floor((float(fx) * px[v] / pz[v] + float(cx)) + 0.5)
    fv = np.floor((float(fy) * py[v] / pz[v] + float(cy)) + 0.5)
    keep = (fu >= 0.0) & (fu < W) & (fv >= 0.0) & (fv < H)
    v, ix, iy = v[keep], fu[keep].astype(np.intp), fv[keep].astype(np.intp)
    if table is not None:
        t = np.asarray(table, np.int32).reshape(H, W, 2)[iy, ix].astype(np.int64)
        ix = np.minimum(np.maximum((t[:, 0] + 16) >> 5, 0), W - 1)
        iy = np.minimum(np.maximum((t[:, 1] + 16) >> 5, 0), H - 1)
    d = depth[iy, ix].astype(np.float64) * 0.001
    keep = (d > 0.0) & (d <= max_dist)
    v, d = v[keep], d[keep]
    sdf = d - pz[v]
    if sdf_out is not None:
        sdf_out.extend(sdf.tolist())
    out[v[(sdf >= -band) & (sdf <= band)]] = OCCUPIED
    out[v[sdf > band]] = FREE
    return out.reshape(nz, ny, nx)


def apply(words, obs, settle_frames):
    """The layer after one frame's observations."""
    run, settled = unpack(words)
    occ, free = obs == OCCUPIED, obs == FREE
    run = np.where(occ, np.minimum(run + 1, SATURATED), run)
    settled = settled | (occ & (run >= settle_frames))
    run = np.where(free, 0, run)
    settled = settled & ~free
    return pack(run, settled)


def update(words, origin, s, cam, frames, poses, max_dist, band, settle_frames, table=None):
    """The layer after the frames of a call, in frame order."""
    w = np.array(words, np.uint32)
    for f in range(len(poses)):
        w = apply(w, observations(w.shape[::-1], origin, s, cam, frames[f], poses[f], max_dist, band, table), settle_frames)
    return w


def guarded(dims, origin, s, cam, depth_mm, world_T_cam, max_dist, band, table=None):
    """(True when scaling band by 1 +- 1e-9 changes no observation, the nearest |sdf| to a gate)."""
    sdf = []
    base = observations(dims, origin, s, cam, depth_mm, world_T_cam, max_dist, band, table, sdf_out=sdf)
    same = all(np.array_equal(base, observations(dims, origin, s, cam, depth_mm, world_T_cam, max_dist, band * scale, table))
               for scale in (1.0 - 1e-9, 1.0 + 1e-9))
    sdf = np.array(sdf)
    gap = float(np.min(np.abs(np.abs(sdf) - band))) if sdf.size else float("inf")
    return same, gap


def pixel_voxels(shape, origin, s, cam, mm, T):
    """Steps 2-3 of the mask: (inside [H][W], k, j, i) of every pixel's point."""
    W, H, fx, fy, cx, cy = cam
    W, H = int(W), int(H)
    nz, ny, nx = shape
    ys, xs = np.mgrid[0:H, 0:W]
    D = mm.astype(np.float64) * 0.001
    a, b = D * ((xs.astype(np.float64) - float(cx)) / float(fx)), D * ((ys.astype(np.float64) - float(cy)) / float(fy))
    g = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            p = ((T[r, 0] * a + T[r, 1] * b) + T[r, 2] * D) + T[r, 3]
            g.append(np.floor((p - float(origin[r])) / float(s)))
        inside = (g[0] >= 0) & (g[0] <= nx - 1) & (g[1] >= 0) & (g[1] <= ny - 1) & (g[2] >= 0) & (g[2] <= nz - 1)
    i, j, k = (np.where(inside, x, 0).astype(np.intp) for x in g)
    return inside, k, j, i


def dynamic_frame(tsdf, weight, words, origin, s, trunc, cam, depth_mm, world_T_cam, max_dist=10.0, table=None, **params):
    """tests/ref_tsdf_dynamic.py's frame with the layer's term: a settled voxel is no candidate."""
    prm = {**REF.PRM, **params}
    base = REF.dynamic_frame(tsdf, weight, origin, s, trunc, cam, depth_mm, world_T_cam, max_dist=max_dist, table=table, **prm)
    if base["stats"][0] == REF.UNUSED:
        return base
    T = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    mm = REF.resample(depth_mm, cam, table)
    inside, k, j, i = pixel_voxels(np.asarray(tsdf).shape, origin, s, cam, mm, T)
    released = inside & unpack(words)[1][k, j, i]
    cand = (base["candidates"].astype(bool) & ~released).astype(np.uint8)
    ro, rd = int(prm["open_radius"]), int(prm["dilate_radius"])
    mask = REF.dilation(REF.dilation(REF.erosion(cand, ro), ro), rd)
    depth = mm.copy()
    depth[mask != 0] = 0
    stats = np.array([REF.OK, int(base["valid"].sum()), int(cand.sum()), int((base["valid"] & mask).sum())], np.int32)
    return {"mask": mask, "depth": depth, "stats": stats, "valid": base["valid"], "candidates": cand}


def dynamic(tsdf, weight, words, origin, s, trunc, cam, frames, poses, settle_frames, band_vox, max_dist=10.0, table=None,
            **params):
    """One tslam_tsdf_dynamic call with the layer on: every frame classified against ``words`` as
    they stand, then ``words`` updated with the frames in order."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    res = [dynamic_frame(tsdf, weight, words, origin, s, trunc, cam, frames[f], poses[f], max_dist=max_dist, table=table, **params)
           for f in range(len(poses))]
    out = {k: np.stack([r[k] for r in res]) for k in res[0]}
    out["words"] = update(words, origin, s, cam, frames, poses, float(max_dist), float(band_vox) * float(s), settle_frames, table)
    return out
