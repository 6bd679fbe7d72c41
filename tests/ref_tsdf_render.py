"""An independent restatement of the ray-casting rule of thor_slam_amd/dense_render.py (rules 1-6
of its docstring) for the tests: rays in lockstep, the volume indexed as [k][j][i].  IEEE f64, one
rounding per operation, sums in the written order; NumPy's element-wise operations do that."""

from __future__ import annotations

import numpy as np


def _lerp(p, q, u):
    return p + u * (q - p)


def sample(tsdf, weight, min_weight, gx, gy, gz):
    """Rule 4: (known, value) at grid coordinates (arrays of one length)."""
    nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        bx, by, bz = np.floor(gx), np.floor(gy), np.floor(gz)
        valid = (bx >= 0) & (bx <= nx - 2) & (by >= 0) & (by <= ny - 2) & (bz >= 0) & (bz <= nz - 2)
    i = np.where(valid, bx, 0).astype(np.intp)
    j = np.where(valid, by, 0).astype(np.intp)
    k = np.where(valid, bz, 0).astype(np.intp)
    known = valid.copy()
    corner = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                known &= weight[k + dz, j + dy, i + dx].astype(np.float64) >= min_weight
                corner[dx, dy, dz] = tsdf[k + dz, j + dy, i + dx].astype(np.float64)
    ux, uy, uz = gx - bx, gy - by, gz - bz
    front = _lerp(_lerp(corner[0, 0, 0], corner[1, 0, 0], ux), _lerp(corner[0, 1, 0], corner[1, 1, 0], ux), uy)
    back = _lerp(_lerp(corner[0, 0, 1], corner[1, 0, 1], ux), _lerp(corner[0, 1, 1], corner[1, 1, 1], ux), uy)
    return known, _lerp(front, back, uz)


def render_view(tsdf, weight, origin, s, cam, T, min_weight=1e-4, min_depth=0.0, max_depth=10.0, step_scale=0.5,
                color=None, color_weight=None):
    W, H, fx, fy, cx, cy = cam
    tsdf = np.asarray(tsdf, np.float32)
    weight = np.asarray(weight, np.float32)
    nz, ny, nx = tsdf.shape
    dims = (nx, ny, nz)
    out = {"depth_m": np.zeros((H, W), np.float32), "depth_mm": np.zeros((H, W), np.uint16),
           "normal": np.zeros((H, W, 3), np.float32), "color": np.zeros((H, W, 3), np.uint8),
           "samples": np.zeros((H, W), np.int32)}
    T = np.asarray(T, np.float64).reshape(4, 4)
    if not np.isfinite(T[0, 0]):
        return out
    ys, xs = np.mgrid[0:H, 0:W]
    dc0 = ((xs.astype(np.float64) - cx) / fx).ravel()
    dc1 = ((ys.astype(np.float64) - cy) / fy).ravel()
    L = np.sqrt((dc0 * dc0 + dc1 * dc1) + 1.0)
    g0 = [(T[a, 3] - origin[a]) / s - 0.5 for a in range(3)]
    gd = [((T[a, 0] * dc0 + T[a, 1] * dc1) + T[a, 2]) / s for a in range(3)]
    # clip
    t0 = np.full(W * H, float(min_depth))
    t1 = np.full(W * H, float(max_depth))
    alive = np.ones(W * H, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            top = float(dims[a] - 1)
            par = gd[a] == 0
            if g0[a] < 0 or g0[a] > top:
                alive &= ~par
            qa, qb = (0.0 - g0[a]) / gd[a], (top - g0[a]) / gd[a]
            t0 = np.where(par, t0, np.maximum(t0, np.minimum(qa, qb)))
            t1 = np.where(par, t1, np.minimum(t1, np.maximum(qa, qb)))
    alive &= t0 <= t1
    # march: a ray's state lives at its pixel index; `alive` marks the rays still going
    t = t0.copy()
    prev_f = np.full(W * H, np.nan)          # NaN: no prev
    prev_t = np.zeros(W * H)
    t_hit = np.full(W * H, np.nan)
    count = np.zeros(W * H, np.int32)
    for _ in range(nx + ny + nz + 2):
        r = np.flatnonzero(alive)
        if r.size == 0:
            break
        known, f = sample(tsdf, weight, min_weight, g0[0] + t[r] * gd[0][r], g0[1] + t[r] * gd[1][r], g0[2] + t[r] * gd[2][r])
        count[r] += 1
        has = ~np.isnan(prev_f[r])
        hit = known & has & (f <= 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            th = prev_t[r] + (t[r] - prev_t[r]) * (prev_f[r] / (prev_f[r] - f))
        t_hit[r[hit]] = th[hit]
        alive[r[hit]] = False
        go = r[~hit]
        fg = f[~hit]
        pos = known[~hit] & (fg > 0)
        prev_f[go] = np.where(pos, fg, np.nan)
        prev_t[go] = t[go]
        step = np.where(pos, np.maximum(step_scale * fg, s), s)
        t[go] = t[go] + step / L[go]
        alive[go[t[go] > t1[go]]] = False
    out["samples"] = count.reshape(H, W)
    r = np.flatnonzero(~np.isnan(t_hit))
    if r.size == 0:
        return out
    ts = t_hit[r]
    depth_m = np.zeros(W * H, np.float32)
    depth_m[r] = ts.astype(np.float32)
    mm = np.floor(1000.0 * ts + 0.5)
    mm[(mm < 1) | (mm > 65535)] = 0
    depth_mm = np.zeros(W * H, np.uint16)
    depth_mm[r] = mm.astype(np.uint16)
    gs = [g0[a] + ts * gd[a][r] for a in range(3)]
    grad, ok = [], np.ones(r.size, bool)
    for a in range(3):
        plus = [gs[b] + 0.5 if b == a else gs[b] for b in range(3)]
        minus = [gs[b] - 0.5 if b == a else gs[b] for b in range(3)]
        kp, fp = sample(tsdf, weight, min_weight, *plus)
        km, fm = sample(tsdf, weight, min_weight, *minus)
        ok &= kp & km
        grad.append(fp - fm)
    length = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2])
    ok &= length > 0
    normal = np.zeros((W * H, 3), np.float32)
    for a in range(3):
        with np.errstate(divide="ignore", invalid="ignore"):
            normal[r, a] = np.where(ok, grad[a] / length, 0.0).astype(np.float32)
    col = np.zeros((W * H, 3), np.uint8)
    if color is not None:
        vi = [np.clip(np.floor(gs[a] + 0.5), 0, dims[a] - 1).astype(np.intp) for a in range(3)]
        rgb = np.asarray(color, np.float32)[vi[2], vi[1], vi[0]].astype(np.float64)
        cw = np.asarray(color_weight, np.float32)[vi[2], vi[1], vi[0]]
        with np.errstate(invalid="ignore"):
            q = np.clip(np.floor(rgb + 0.5), 0, 255)
        q[np.isnan(q)] = 0
        q[~(cw > 0)] = 0
        col[r] = q[:, ::-1].astype(np.uint8)
    out["depth_m"], out["depth_mm"] = depth_m.reshape(H, W), depth_mm.reshape(H, W)
    out["normal"], out["color"] = normal.reshape(H, W, 3), col.reshape(H, W, 3)
    return out


def render(tsdf, weight, origin, s, cam, poses, **kw):
    views = [render_view(tsdf, weight, origin, s, cam, T, **kw) for T in np.asarray(poses, np.float64).reshape(-1, 4, 4)]
    return {k: np.stack([v[k] for v in views]) for k in views[0]}
