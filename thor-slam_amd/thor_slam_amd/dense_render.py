"""The dense map seen from a pose: TSDF ray casting (``tslam_tsdf_render_init`` / ``tslam_tsdf_render``
/ ``tslam_tsdf_render_buffers`` / ``tslam_tsdf_render_read``; ``k_tsdf_render`` in
``k_tsdf_render.hip``; ``HipSlamEngine.get_dense_view``).  For every pixel of a pinhole camera at
``world_T_cam`` (in the volume's frame) the depth, the normal and the colour of the surface the
volume holds.  This file is the spec, a NumPy reference of every operation the device performs,
restated for the tests in ``tests/ref_tsdf_render.py``.

All arithmetic is IEEE f64, one rounding per written operation (no fused multiply-add), sums in the
written order.  Volume values are f32 [nz][ny][nx], widened on load.

* **Inputs.**  ``tsdf``, ``weight`` and optionally the colour layer, dims ``n = (nx, ny, nz)``, every
  ``n_a >= 2``; the voxel size ``s`` and the effective corner ``o`` (with a rolling window
  ``o = o0 + s * float(shift)``, thor_slam_amd/dense_follow.py); a camera ``W, H, fx, fy, cx, cy``
  without distortion; per view ``world_T_cam`` = rotation ``R``, centre ``C`` and a use flag (a pose
  whose first element is not finite, or an untracked batch frame: unused, all outputs zero);
  ``min_weight >= 0``, ``0 <= min_depth < max_depth``, ``0 < step_scale <= 1``.
* **1. Ray of pixel (x, y).**  ``dc = ((x - cx) / fx, (y - cy) / fy, 1)``,
  ``d[a] = (R[a][0] dc0 + R[a][1] dc1) + R[a][2]``.  The ray parameter ``t`` is the depth along the
  camera's z axis; one unit of ``t`` is ``L = sqrt((dc0^2 + dc1^2) + 1)`` metres.  ``L`` belongs to
  the camera: a host table f64 [H][W] (``ray_length_table``), which the device loads.
* **2. Grid coordinates** (voxel-centre index units).  ``g0[a] = (C[a] - o[a]) / s - 0.5``,
  ``gd[a] = d[a] / s``, ``g(t)[a] = g0[a] + t * gd[a]``.
* **3. Clip.**  ``[t0, t1]`` starts as ``[min_depth, max_depth]``.  Per axis: with ``gd[a] == 0``
  the ray misses if ``g0[a] < 0`` or ``g0[a] > n_a - 1`` and is otherwise unconstrained; else with
  ``qa = (0 - g0[a]) / gd[a]`` and ``qb = ((n_a - 1) - g0[a]) / gd[a]``:
  ``t0 = max(t0, min(qa, qb))``, ``t1 = min(t1, max(qa, qb))``.  The ray misses unless ``t0 <= t1``.
* **4. Sample at g.**  ``b = floor(g)``; the cell is valid when ``0 <= b[a] <= n_a - 2`` on every
  axis; the sample is *known* when the cell is valid and all eight corner weights are
  ``>= min_weight``.  Its value, with ``u = g - b`` and ``lerp(p, q, u) = p + u * (q - p)``: along x
  (four lerps), then y (two), then z.
* **5. March** from ``t = t0`` with ``prev = none``.  At each sample: if it is known, ``prev``
  exists and ``f <= 0`` the ray hits at ``t* = tp + (t - tp) * (fp / (fp - f))``.  Otherwise
  ``prev = (f, t)`` if the sample is known and ``f > 0``, else none; then
  ``t = t + max(step_scale * f, s) / L`` with a ``prev``, else ``t = t + s / L``; if ``t > t1`` the
  ray misses.  A back face (negative, then positive) is never a hit.  Every step is at least one
  voxel of metric length, so a ray inside the slabs takes at most the volume's diagonal in voxels
  plus one samples; a ray that has taken ``nx + ny + nz + 2`` samples misses (a bound exact
  arithmetic never reaches: it keeps a degenerate camera from marching without end).
* **6. Outputs at a hit**, with ``g* = g(t*)``.  ``depth_m = f32(t*)``;
  ``depth_mm = floor(1000 t* + 0.5)`` as u16, 0 when that is below 1 or above 65535 (the format
  ``tslam_tsdf_integrate`` reads).  ``normal``: central differences of the same field,
  ``grad[a] = f(g* + e_a / 2) - f(g* - e_a / 2)`` (six samples of rule 4); (0, 0, 0) if one of them
  is not known or ``|grad| = sqrt((gx^2 + gy^2) + gz^2)`` is not above zero, else ``f32(grad[a] /
  |grad|)``: in the volume's frame, pointing into free space as the mesh's faces do.  ``color``: of
  the voxel ``clamp(floor(g*[a] + 0.5), 0, n_a - 1)``; with the colour layer on and that voxel's
  colour weight above 0 the channels ``min(max(floor(c + 0.5), 0), 255)`` in the order B, G, R (the
  input images' order; the layer stores R, G, B), else 0, 0, 0.
* **A miss** gives zeros in every output, as every pixel of an unused view does.  A hit has
  ``depth_m > 0``.

``step_scale`` below 1 exists because the TSDF is projective: along a ray that is not the
integrating camera's it over-estimates the distance to the surface, and a full step can jump the
thin negative band of a surface seen at a grazing angle.
"""

from __future__ import annotations

import math

import numpy as np

OUT_DEPTH_M, OUT_DEPTH_MM, OUT_NORMAL, OUT_COLOR = 1, 2, 4, 8     # tslam_tsdf_render_params.outputs
OUT_ALL = 15
MAX_VIEWS = 256                                                    # TSDF_MAX_FRAMES
MAX_IMAGE = 16384


def check_render_params(width, height, fx, fy, cx, cy, min_weight, min_depth, max_depth, step_scale,
                        outputs=OUT_ALL, max_views=1) -> None:
    """``tslam_tsdf_render_init`` refuses the same settings."""
    for v in (width, height, outputs, max_views):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("width, height, outputs and max_views must be integers")
    if not (1 <= width <= MAX_IMAGE and 1 <= height <= MAX_IMAGE):
        raise ValueError(f"width and height must be 1..{MAX_IMAGE}")
    vals = [float(v) for v in (fx, fy, cx, cy, min_weight, min_depth, max_depth, step_scale)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("camera and render parameters must be finite")
    if not (vals[0] > 0 and vals[1] > 0):
        raise ValueError("fx and fy must be > 0")
    if not vals[4] >= 0:
        raise ValueError("min_weight must be >= 0")
    if not 0 <= vals[5] < vals[6]:
        raise ValueError("need 0 <= min_depth < max_depth")
    if not 0 < vals[7] <= 1:
        raise ValueError("step_scale must be in (0, 1]")
    if not 1 <= outputs <= OUT_ALL:
        raise ValueError("outputs must be a bit mask 1..15")
    if not 1 <= max_views <= MAX_VIEWS:
        raise ValueError(f"max_views must be 1..{MAX_VIEWS}")


def ray_length_table(W: int, H: int, fx: float, fy: float, cx: float, cy: float) -> np.ndarray:
    """``L`` of rule 1, f64 [H][W]."""
    dc0 = (np.arange(W, dtype=np.float64) - float(cx)) / float(fx)
    dc1 = (np.arange(H, dtype=np.float64) - float(cy)) / float(fy)
    return np.sqrt((dc0[None, :] * dc0[None, :] + dc1[:, None] * dc1[:, None]) + 1.0)


def scaled_intrinsics(rect_size, rect_intr, size) -> tuple:
    """The intrinsics of a camera of ``size`` = (W, H) pixels with the field of view of the camera
    ``rect_size``, ``rect_intr`` = (fx, fy, cx, cy): pixel centres at integers."""
    (w0, h0), (fx, fy, cx, cy), (w, h) = rect_size, rect_intr, size
    ax, ay = float(w) / float(w0), float(h) / float(h0)
    return (fx * ax, fy * ay, (cx + 0.5) * ax - 0.5, (cy + 0.5) * ay - 0.5)


def rigid_inverse(T: np.ndarray) -> np.ndarray:
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    for r in range(3):
        for c in range(3):
            out[r, c] = T[c, r]
        out[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return out


def view_in_volume(world_T_volume: np.ndarray, world_T_view: np.ndarray) -> np.ndarray:
    """``volume_T_view = world_T_volume^-1 world_T_view`` (rigid), sums in index order: how
    ``get_dense_view`` moves a camera pose of the published world into the volume's frame."""
    A, B = rigid_inverse(world_T_volume), np.asarray(world_T_view, dtype=np.float64)
    out = np.eye(4)
    for r in range(3):
        for c in range(4):
            out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return out


class _Volume:
    def __init__(self, tsdf, weight, min_weight):
        self.tsdf = np.ascontiguousarray(tsdf, dtype=np.float32)
        self.weight = np.ascontiguousarray(weight, dtype=np.float32)
        nz, ny, nx = self.tsdf.shape
        if min(nx, ny, nz) < 2 or self.weight.shape != self.tsdf.shape:
            raise ValueError("the volume needs dims >= 2 and a weight of the same shape")
        self.n = np.array([nx, ny, nz], dtype=np.float64)
        self.dims = (nx, ny, nz)
        self.min_weight = float(min_weight)
        self.off = [dz * ny * nx + dy * nx + dx for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]

    def sample(self, g: np.ndarray):
        """Rule 4 at grid coordinates g [m][3]: (known [m], f [m])."""
        nx, ny, _ = self.dims
        with np.errstate(invalid="ignore"):
            b = np.floor(g)
            valid = np.all((b >= 0.0) & (b <= self.n - 2.0), axis=1)
        known = np.zeros(g.shape[0], dtype=bool)
        f = np.zeros(g.shape[0], dtype=np.float64)
        idx = np.nonzero(valid)[0]
        if idx.size == 0:
            return known, f
        bi = b[idx].astype(np.int64)
        u = g[idx] - b[idx]
        base = (bi[:, 2] * ny + bi[:, 1]) * nx + bi[:, 0]
        tf, wf = self.tsdf.reshape(-1), self.weight.reshape(-1)
        ok = np.ones(idx.size, dtype=bool)
        v = []
        for o in self.off:
            ok &= wf[base + o].astype(np.float64) >= self.min_weight
            v.append(tf[base + o].astype(np.float64))
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        c00 = v[0] + ux * (v[1] - v[0])
        c10 = v[2] + ux * (v[3] - v[2])
        c01 = v[4] + ux * (v[5] - v[4])
        c11 = v[6] + ux * (v[7] - v[6])
        c0 = c00 + uy * (c10 - c00)
        c1 = c01 + uy * (c11 - c01)
        known[idx] = ok
        f[idx] = c0 + uz * (c1 - c0)
        return known, f


def render_view(tsdf, weight, origin, s, cam, world_T_cam, min_weight=1e-4, min_depth=0.0, max_depth=10.0,
                step_scale=0.5, color=None, color_weight=None) -> dict:
    """One view: ``depth_m`` f32 [H][W], ``depth_mm`` u16 [H][W], ``normal`` f32 [H][W][3], ``color``
    u8 [H][W][3] (B, G, R); for measurements also ``samples`` i32 [H][W], the samples rule 5 took
    per ray, and ``t`` f64 [H][W], the hit depth t* before the f32 cast (0 at a miss)."""
    W, H, fx, fy, cx, cy = cam
    W, H = int(W), int(H)
    check_render_params(W, H, fx, fy, cx, cy, min_weight, min_depth, max_depth, step_scale)
    vol = _Volume(tsdf, weight, min_weight)
    s = float(s)
    out = {"depth_m": np.zeros((H, W), np.float32), "depth_mm": np.zeros((H, W), np.uint16),
           "normal": np.zeros((H, W, 3), np.float32), "color": np.zeros((H, W, 3), np.uint8),
           "samples": np.zeros((H, W), np.int32), "t": np.zeros((H, W), np.float64)}
    T = np.asarray(world_T_cam, dtype=np.float64).reshape(4, 4)
    if not math.isfinite(T[0, 0]):
        return out
    m = W * H
    # 1. rays
    dc0 = np.tile((np.arange(W, dtype=np.float64) - float(cx)) / float(fx), H)
    dc1 = np.repeat((np.arange(H, dtype=np.float64) - float(cy)) / float(fy), W)
    L = ray_length_table(W, H, fx, fy, cx, cy).reshape(-1)
    # 2. grid coordinates
    g0 = np.array([(T[a, 3] - float(origin[a])) / s - 0.5 for a in range(3)])
    gd = np.stack([((T[a, 0] * dc0 + T[a, 1] * dc1) + T[a, 2]) / s for a in range(3)], axis=1)
    # 3. clip
    t0 = np.full(m, float(min_depth))
    t1 = np.full(m, float(max_depth))
    miss = np.zeros(m, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(3):
            zero = gd[:, a] == 0.0
            miss |= zero & bool(g0[a] < 0.0 or g0[a] > vol.n[a] - 1.0)
            qa = (0.0 - g0[a]) / gd[:, a]
            qb = ((vol.n[a] - 1.0) - g0[a]) / gd[:, a]
            t0 = np.where(zero, t0, np.maximum(t0, np.minimum(qa, qb)))
            t1 = np.where(zero, t1, np.minimum(t1, np.maximum(qa, qb)))
        miss |= ~(t0 <= t1)
    # 5. march
    t = t0.copy()
    has = np.zeros(m, dtype=bool)
    fp, tp = np.zeros(m), np.zeros(m)
    tstar = np.zeros(m)
    hit = np.zeros(m, dtype=bool)
    samples = np.zeros(m, dtype=np.int32)
    act = np.nonzero(~miss)[0]
    for _ in range(sum(vol.dims) + 2):
        if act.size == 0:
            break
        known, f = vol.sample(g0[None, :] + t[act, None] * gd[act])
        samples[act] += 1
        h = known & has[act] & (f <= 0.0)
        hi = act[h]
        tstar[hi] = tp[hi] + (t[hi] - tp[hi]) * (fp[hi] / (fp[hi] - f[h]))
        hit[hi] = True
        rest, f = act[~h], f[~h]
        pos = known[~h] & (f > 0.0)
        has[rest] = pos
        fp[rest] = np.where(pos, f, 0.0)
        tp[rest] = t[rest]
        t[rest] = t[rest] + np.where(pos, np.maximum(float(step_scale) * f, s), s) / L[rest]
        act = rest[~(t[rest] > t1[rest])]
    out["samples"] = samples.reshape(H, W)
    out["t"] = tstar.reshape(H, W)
    # 6. outputs
    hi = np.nonzero(hit)[0]
    if hi.size == 0:
        return out
    ts = tstar[hi]
    dm = np.zeros(m, np.float32)
    dm[hi] = ts.astype(np.float32)
    mm = np.floor(1000.0 * ts + 0.5)
    mm = np.where((mm < 1.0) | (mm > 65535.0), 0.0, mm)
    dmm = np.zeros(m, np.uint16)
    dmm[hi] = mm.astype(np.uint16)
    gs = g0[None, :] + ts[:, None] * gd[hi]
    grad = np.zeros((hi.size, 3))
    ok = np.ones(hi.size, dtype=bool)
    for a in range(3):
        e = np.zeros(3)
        e[a] = 0.5
        kp, vp = vol.sample(gs + e[None, :])
        km, vm = vol.sample(gs - e[None, :])
        ok &= kp & km
        grad[:, a] = vp - vm
    norm = np.sqrt((grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2])
    ok &= norm > 0.0
    nrm = np.zeros((m, 3), np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm[hi] = np.where(ok[:, None], grad / norm[:, None], 0.0).astype(np.float32)
    col = np.zeros((m, 3), np.uint8)
    if color is not None:
        nx, ny, nz = vol.dims
        v = np.clip(np.floor(gs + 0.5), 0.0, vol.n[None, :] - 1.0).astype(np.int64)
        flat = (v[:, 2] * ny + v[:, 1]) * nx + v[:, 0]
        c = np.ascontiguousarray(color, dtype=np.float32).reshape(-1, 3)[flat].astype(np.float64)
        cw = np.ascontiguousarray(color_weight, dtype=np.float32).reshape(-1)[flat]
        with np.errstate(invalid="ignore"):
            q = np.minimum(np.maximum(np.floor(c + 0.5), 0.0), 255.0)
        q = np.where(np.isnan(q), 0.0, q)
        col[hi] = np.where((cw > 0.0)[:, None], q[:, ::-1], 0.0).astype(np.uint8)
    out["depth_m"], out["depth_mm"] = dm.reshape(H, W), dmm.reshape(H, W)
    out["normal"], out["color"] = nrm.reshape(H, W, 3), col.reshape(H, W, 3)
    return out


def render(tsdf, weight, origin, s, cam, poses, **kw) -> dict:
    """``render_view`` of every pose of ``poses`` [n][4][4], stacked on a leading axis."""
    views = [render_view(tsdf, weight, origin, s, cam, T, **kw) for T in np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)]
    return {k: np.stack([v[k] for v in views]) for k in views[0]}
