"""An independent restatement of thor_slam_amd/dense_align.py for the tests: the same rule written
from its text, with flat pixel arrays, a top-down tree and an explicit matrix factorisation, so that
an error in either file shows as a difference.  IEEE f64, one rounding per written operation."""

from __future__ import annotations

import math

import numpy as np

import ref_tsdf_render as RR

OK, UNUSED, NO_MODEL, DEGENERATE, REJECTED = range(5)
PRM = dict(iterations=10, min_inliers=200, max_distance=0.1, min_weight=1e-4, max_depth=10.0, step_scale=0.5,
           max_translation=0.1, max_rotation=0.1, eps_translation=1e-6, eps_rotation=1e-6, min_pivot=1e-6)


def fold(v):
    """The pairwise tree, top down: a power-of-two run is the sum of its two halves' trees."""
    n = v.shape[0]
    if n == 1:
        return v[0]
    return fold(v[:n // 2]) + fold(v[n // 2:])


def view_sums(terms, W, H):
    """terms [H*W][29] -> 29 sums in the rule's order: lanes, the four tiles, the blocks."""
    bx, by = -(-W // 16), -(-H // 16)
    size = 256
    while size < bx * by:
        size *= 2
    blocks = np.zeros((size, 29))
    img = np.zeros((by * 16, bx * 16, 29))
    img[:H, :W] = terms.reshape(H, W, 29)
    cut = img.reshape(by, 2, 8, bx, 2, 8, 29)          # [block row][tile row][y in tile][block col][tile col][x in tile]
    tiles = []
    for wy in (0, 1):
        for wx in (0, 1):                              # every block's tile (wy, wx) at once: lanes first, blocks by * bx + bx
            lanes = cut[:, wy, :, :, wx, :, :].transpose(1, 3, 0, 2, 4).reshape(64, by * bx, 29)
            tiles.append(fold(lanes))
    blocks[:by * bx] = (tiles[0] + tiles[1]) + (tiles[2] + tiles[3])
    return fold(blocks)


def frame_terms(depth_mm, cam, table, max_dist, T, T0, dm, nrm, gate):
    W, H, fx, fy, cx, cy = int(cam[0]), int(cam[1]), *[float(v) for v in cam[2:]]
    x = np.tile(np.arange(W), H)
    y = np.repeat(np.arange(H), W)
    sx, sy = x, y
    if table is not None:
        t = np.asarray(table, dtype=np.int64).reshape(-1, 2)
        sx = np.minimum(np.maximum((t[:, 0] + 16) >> 5, 0), W - 1)
        sy = np.minimum(np.maximum((t[:, 1] + 16) >> 5, 0), H - 1)
    D = np.asarray(depth_mm).reshape(-1)[sy * W + sx].astype(np.float64) * 0.001
    keep = (D > 0.0) & (D <= max_dist)
    a, b = D * ((x - cx) / fx), D * ((y - cy) / fy)
    R, C, R0, C0 = T[:3, :3], T[:3, 3], T0[:3, :3], T0[:3, 3]
    p = np.stack([((R[i, 0] * a + R[i, 1] * b) + R[i, 2] * D) + C[i] for i in range(3)], axis=1)
    h = p - C0[None, :]
    q = np.stack([(R0[0, i] * h[:, 0] + R0[1, i] * h[:, 1]) + R0[2, i] * h[:, 2] for i in range(3)], axis=1)
    keep &= q[:, 2] > 0.0
    with np.errstate(all="ignore"):
        u = np.floor(((fx * q[:, 0]) / q[:, 2] + cx) + 0.5)
        v = np.floor(((fy * q[:, 1]) / q[:, 2] + cy) + 0.5)
    keep &= (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
    m = np.where(keep, v * W + u, 0).astype(np.int64)
    z = dm.reshape(-1).astype(np.float64)[m]
    n = nrm.reshape(-1, 3).astype(np.float64)[m]
    keep &= (z > 0.0) & ((n[:, 0] != 0.0) | (n[:, 1] != 0.0) | (n[:, 2] != 0.0))
    m0, m1 = ((m % W) - cx) / fx, ((m // W) - cy) / fy
    V = np.stack([C0[i] + z * ((R0[i, 0] * m0 + R0[i, 1] * m1) + R0[i, 2]) for i in range(3)], axis=1)
    e = p - V
    keep &= (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= gate * gate
    r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    J = np.stack([n[:, 0], n[:, 1], n[:, 2], p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
    cols = [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [-(J[:, i] * r) for i in range(6)] + [r * r, np.ones_like(r)]
    return np.where(keep[:, None], np.stack(cols, axis=1), 0.0)


def factor_solve(s, min_pivot):
    """LDL^T: x, or None when a pivot is at or below min_pivot times the largest diagonal entry;
    also the smallest pivot ratio met."""
    A = np.zeros((6, 6))
    it = iter(s[:21])
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = next(it)
    big = max(A[i, i] for i in range(6))
    L, d = np.eye(6), np.zeros(6)
    worst = math.inf
    for j in range(6):
        acc = A[j, j]
        for k in range(j):
            acc = acc - L[j, k] * (L[j, k] * d[k])
        d[j] = acc
        worst = min(worst, acc / big) if big > 0 else 0.0
        if not acc > min_pivot * big:
            return None, worst
        for i in range(j + 1, 6):
            acc = A[i, j]
            for k in range(j):
                acc = acc - L[i, k] * (L[j, k] * d[k])
            L[i, j] = acc / d[j]
    y = np.zeros(6)
    for i in range(6):
        acc = s[21 + i]
        for k in range(i):
            acc = acc - L[i, k] * y[k]
        y[i] = acc
    x = np.zeros(6)
    for i in reversed(range(6)):
        acc = y[i] / d[i]
        for k in range(i + 1, 6):
            acc = acc - L[k, i] * x[k]
        x[i] = acc
    return x, worst


def step(T, x):
    t, w = x[:3], x[3:]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if th2 == 0.0:
        a, b = 1.0, 0.5
    else:
        th = math.sqrt(th2)
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    I = np.eye(3)
    Q = (I + a * K) + b * (np.outer(w, w) - I * th2)
    N = np.eye(4)
    for i in range(3):
        for j in range(4):
            N[i, j] = (Q[i, 0] * T[0, j] + Q[i, 1] * T[1, j]) + Q[i, 2] * T[2, j]
        N[i, 3] = N[i, 3] + t[i]
    return N, (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2], th2


def align_frame(tsdf, weight, origin, s, cam, depth_mm, pose, max_dist=10.0, table=None, model=None, **kw):
    prm = {**PRM, **kw}
    T0 = np.eye(4)
    T0[:3] = np.asarray(pose, dtype=np.float64).reshape(4, 4)[:3]
    res = dict(world_T_cam=T0.copy(), status=UNUSED, iterations=0, inliers=[0, 0], rms=[0.0, 0.0], normal_eq=np.zeros(28), counts=[],
               pivots=[])
    if not math.isfinite(T0[0, 0]):
        return res
    if model is None:
        model = RR.render_view(tsdf, weight, origin, s, cam, T0, min_weight=prm["min_weight"], min_depth=0.0,
                               max_depth=prm["max_depth"], step_scale=prm["step_scale"])
    T, status = T0.copy(), OK
    for it in range(prm["iterations"]):
        sums = view_sums(frame_terms(depth_mm, cam, table, float(max_dist), T, T0, model["depth_m"], model["normal"],
                                     float(prm["max_distance"])), int(cam[0]), int(cam[1]))
        n = int(sums[28])
        rms = math.sqrt(sums[27] / sums[28]) if n else 0.0
        if it == 0:
            res["inliers"][0], res["rms"][0] = n, rms
        res["inliers"][1], res["rms"][1], res["iterations"], res["normal_eq"] = n, rms, it + 1, sums[:28].copy()
        res["counts"].append(n)
        if n < prm["min_inliers"]:
            status = NO_MODEL
            break
        x, worst = factor_solve(sums, prm["min_pivot"])
        res["pivots"].append(worst)
        if x is None:
            status = DEGENERATE
            break
        T, tt, th2 = step(T, x)
        if tt < prm["eps_translation"] * prm["eps_translation"] and th2 < prm["eps_rotation"] * prm["eps_rotation"]:
            break
    if status == OK:
        c = T[:3, 3] - T0[:3, 3]
        tr = 0.0
        for i in range(3):
            for j in range(3):
                tr = tr + T[i, j] * T0[i, j]
        if not ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2] <= prm["max_translation"] * prm["max_translation"]
                and tr >= 1.0 + 2.0 * math.cos(prm["max_rotation"])):
            status = REJECTED
    res["status"] = status
    if status == OK:
        res["world_T_cam"] = T
    return res


def align(tsdf, weight, origin, s, cam, depth_mm, poses, models=None, **kw):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    out = [align_frame(tsdf, weight, origin, s, cam, depth_mm[i], poses[i], model=None if models is None else models[i], **kw)
           for i in range(len(poses))]
    return {"world_T_cam": np.stack([o["world_T_cam"] for o in out]),
            "stats": np.array([[o["status"], o["iterations"], o["inliers"][0], o["inliers"][1]] for o in out], dtype=np.int32),
            "residuals": np.array([o["rms"] for o in out]), "normal_eq": np.stack([o["normal_eq"] for o in out]),
            "counts": [o["counts"] for o in out], "pivots": [o["pivots"] for o in out]}
