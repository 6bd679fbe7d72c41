"""Dense frame-to-model alignment: projective point-to-plane ICP of a depth frame against the
ray-cast map (``tslam_tsdf_align_init`` / ``tslam_tsdf_align`` / ``tslam_tsdf_align_read`` /
``tslam_tsdf_align_buffers`` / ``tslam_tsdf_integrate_aligned``; ``k_tsdf_align.hip``;
``HipSlamConfig.dense_align``).  It corrects the pose a depth frame is integrated with (KinectFusion's
tracking half).  This file is the spec, a NumPy reference of every operation the device performs,
restated for the tests in ``tests/ref_tsdf_align.py``.

All arithmetic is IEEE f64, one rounding per written operation (no fused multiply-add), sums in the
written order.  Images are widened on load.

* **Inputs** per frame: the initial pose ``T0 = world_T_cam = (R0, C0)`` in the volume's frame and
  its use flag (a host pose whose first element is not finite, or an untracked batch frame: unused,
  as in ``dense_render.py``); the frame's depth image u16 [H][W] in millimetres; the pair's
  rectified camera ``W, H, fx, fy, cx, cy``; for a raw RGB-D camera its undistortion table i32
  [H][W][2] (5 fractional bits); the volume's ``max_dist``; the parameters below.
* **1. Model images.**  ``depth_m`` and ``normal`` of ``dense_render.py`` at ``T0`` with that camera
  and ``min_weight``, ``min_depth = 0``, ``max_depth``, ``step_scale``.  Model pixel (mx, my) is
  *usable* when ``dm = depth_m > 0`` and a component of its normal ``n`` is not zero.  Its vertex:
  ``Vm[a] = C0[a] + dm * d[a]``, ``d[a] = (R0[a][0] mc0 + R0[a][1] mc1) + R0[a][2]``,
  ``mc = ((mx - cx) / fx, (my - cy) / fy)``.
* **2. One iteration** at ``T = (R, C)`` (``T0`` in the first).  Pixel (x, y):
  ``(ix, iy) = (x, y)``, or through the table ``clamp((map[y][x][k] + 16) >> 5, 0, size - 1)``;
  ``D = depth[iy][ix] * 0.001``, valid when ``0 < D <= max_dist``.
  ``pc = (D dc0, D dc1, D)`` with ``dc = ((x - cx) / fx, (y - cy) / fy)``;
  ``p[a] = ((R[a][0] pc0 + R[a][1] pc1) + R[a][2] pc2) + C[a]``;
  ``h = p - C0``; ``q[a] = (R0[0][a] h0 + R0[1][a] h1) + R0[2][a] h2``; need ``q2 > 0``;
  ``mx = floor((fx q0 / q2 + cx) + 0.5)``, ``my`` alike, inside the image and usable;
  ``e = p - Vm``; need ``(e0^2 + e1^2) + e2^2 <= max_distance * max_distance``;
  ``r = (n0 e0 + n1 e1) + n2 e2``;
  ``J = (n0, n1, n2, p1 n2 - p2 n1, p2 n0 - p0 n2, p0 n1 - p1 n0)`` (translation, then rotation, of
  a left perturbation in the volume's frame).  The pixel's 29 terms: ``J[i] J[j]`` for
  ``i <= j`` (21, row-major), ``-(J[i] r)`` (6), ``r r`` and 1.  A pixel that fails a test
  contributes 29 zeros.
* **3. Reduction**, each of the 29 on its own, by *pairwise trees*: ``tree(v)`` of ``2^k`` values
  replaces them by ``v[2i] + v[2i + 1]`` until one is left (neighbours first).  The image is cut
  into 16 x 16 pixel blocks (zeros outside the image), a block into four 8 x 8 tiles
  ``w = 2 (y / 8 % 2) + (x / 8 % 2)``, a tile into lanes ``l = 8 (y % 8) + (x % 8)``.  A tile is
  ``tree`` over its 64 lanes; a block is ``(w0 + w1) + (w2 + w3)``; the view is ``tree`` over the
  blocks in the order ``by * blocks_x + bx``, padded with zeros to ``max(256, 2^ceil(log2(blocks)))``.
* **4. Solve** ``A x = b`` (A from the 21, b from the 6, ``x = (t, w)``) by LDL^T without pivoting:
  for j = 0..5 with ``g[k] = L[j][k] d[k]``: ``d[j] = A[j][j] - sum_k<j L[j][k] g[k]`` and
  ``L[i][j] = (A[i][j] - sum_k<j L[i][k] g[k]) / d[j]``, every sum subtracted term by term with k
  ascending.  DEGENERATE when a ``d[j] <= min_pivot * max_i A[i][i]`` (tested as it is formed).
  ``y[i] = b[i] - sum_k<i L[i][k] y[k]``; ``z[i] = y[i] / d[i]``; ``x[i] = z[i] - sum_k>i L[k][i] x[k]``
  for i = 5..0, k ascending.
* **5. Update.**  ``th2 = (w0^2 + w1^2) + w2^2``, ``th = sqrt(th2)``; ``a = sin(th) / th``,
  ``b = (1 - cos(th)) / th2`` (``a = 1, b = 0.5`` when ``th2 == 0``);
  ``Q[i][j] = (I[i][j] + a K[i][j]) + b (w[i] w[j] - I[i][j] th2)`` with ``K`` the cross-product
  matrix of ``w``; ``R[i][j] <- (Q[i][0] R[0][j] + Q[i][1] R[1][j]) + Q[i][2] R[2][j]``,
  ``C[i] <- ((Q[i][0] C[0] + Q[i][1] C[1]) + Q[i][2] C[2]) + t[i]``.  ``sqrt``, ``sin`` and ``cos``
  are the only operations of this rule not pinned against the host's.
* **6. Stop** after ``iterations``, or when ``(t0^2 + t1^2) + t2^2 < eps_translation^2`` and
  ``th2 < eps_rotation^2``.
* **7. Accept.**  An iteration with fewer than ``min_inliers`` terms ends the frame as NO_MODEL, a
  degenerate system as DEGENERATE.  At the stop the total correction must satisfy
  ``|C - C0|^2 <= max_translation^2`` (summed as above) and
  ``sum_ij R[i][j] R0[i][j] >= 1 + 2 cos(max_rotation)`` (the sum row-major, left to right; the
  right side computed on the host), else REJECTED.  Every outcome but OK returns ``T0`` bit for bit.
* **Status**: 0 OK, 1 UNUSED, 2 NO_MODEL, 3 DEGENERATE, 4 REJECTED.  **Stats**: status, iterations
  run, the inliers of the first and of the last executed iteration; their rms residuals
  ``sqrt(sum r^2 / inliers)`` (0 without inliers); the 28 sums (A, b, sum r^2) of the last executed
  iteration.
"""

from __future__ import annotations

import math

import numpy as np

from .dense_render import render_view

OK, UNUSED, NO_MODEL, DEGENERATE, REJECTED = 0, 1, 2, 3, 4
MAX_ITERATIONS = 64
MAX_FRAMES = 256                                                   # TSDF_MAX_FRAMES
N_TERMS = 29
DEFAULTS = dict(iterations=10, min_inliers=200, max_distance=0.1, min_weight=1e-4, max_depth=10.0, step_scale=0.5,
                max_translation=0.1, max_rotation=0.1, eps_translation=1e-6, eps_rotation=1e-6, min_pivot=1e-6)
_UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


def check_align_params(iterations, min_inliers, max_distance, min_weight, max_depth, step_scale, max_translation,
                       max_rotation, eps_translation, eps_rotation, min_pivot, max_frames=1) -> None:
    """``tslam_tsdf_align_init`` refuses the same settings."""
    for v in (iterations, min_inliers, max_frames):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("iterations, min_inliers and max_frames must be integers")
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be 1..{MAX_ITERATIONS}")
    if min_inliers < 6:
        raise ValueError("min_inliers must be >= 6")
    if not 1 <= max_frames <= MAX_FRAMES:
        raise ValueError(f"max_frames must be 1..{MAX_FRAMES}")
    vals = [float(v) for v in (max_distance, min_weight, max_depth, step_scale, max_translation, max_rotation,
                               eps_translation, eps_rotation, min_pivot)]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("align parameters must be finite")
    if not (vals[0] > 0 and vals[2] > 0 and vals[4] > 0):
        raise ValueError("max_distance, max_depth and max_translation must be > 0")
    if not vals[1] >= 0:
        raise ValueError("min_weight must be >= 0")
    if not 0 < vals[3] <= 1:
        raise ValueError("step_scale must be in (0, 1]")
    if not 0 < vals[5] <= math.pi:
        raise ValueError("max_rotation must be in (0, pi]")
    if not (vals[6] >= 0 and vals[7] >= 0):
        raise ValueError("eps_translation and eps_rotation must be >= 0")
    if not 0 < vals[8] < 1:
        raise ValueError("min_pivot must be in (0, 1)")


def tree(v: np.ndarray) -> np.ndarray:
    """Rule 3's pairwise tree over axis 0 (a power of two long)."""
    while v.shape[0] > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def reduce_view(terms: np.ndarray) -> np.ndarray:
    """Rule 3: terms f64 [H][W][29] -> the 29 sums."""
    H, W, n = terms.shape
    by, bx = (H + 15) // 16, (W + 15) // 16
    pad = np.zeros((by * 16, bx * 16, n))
    pad[:H, :W] = terms
    # [by][wy][ly][bx][wx][lx] -> [lane][wave][block]
    v = pad.reshape(by, 2, 8, bx, 2, 8, n).transpose(2, 5, 1, 4, 0, 3, 6).reshape(64, 4, by * bx, n)
    w = tree(v)
    blocks = (w[0] + w[1]) + (w[2] + w[3])
    size = 256
    while size < by * bx:
        size *= 2
    padded = np.zeros((size, n))
    padded[:by * bx] = blocks
    return tree(padded)


def model_vertices(model: dict, cam, T0: np.ndarray):
    """Rule 1: (usable [H][W], Vm [H][W][3], n [H][W][3]) of the model images at T0."""
    W, H, fx, fy, cx, cy = cam
    dm = model["depth_m"].astype(np.float64)
    n = model["normal"].astype(np.float64)
    usable = (dm > 0.0) & np.any(n != 0.0, axis=-1)
    mc0 = ((np.arange(int(W), dtype=np.float64) - float(cx)) / float(fx))[None, :]
    mc1 = ((np.arange(int(H), dtype=np.float64) - float(cy)) / float(fy))[:, None]
    Vm = np.stack([T0[a, 3] + dm * ((T0[a, 0] * mc0 + T0[a, 1] * mc1) + T0[a, 2]) for a in range(3)], axis=-1)
    return usable, Vm, n


def pixel_terms(depth_mm, cam, undistort, max_dist, T, T0, usable, Vm, nrm, max_distance) -> np.ndarray:
    """Rule 2: the 29 terms of every pixel, f64 [H][W][29]."""
    W, H, fx, fy, cx, cy = cam
    W, H, fx, fy, cx, cy = int(W), int(H), float(fx), float(fy), float(cx), float(cy)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ix, iy = xs, ys
    if undistort is not None:
        mp = np.asarray(undistort, dtype=np.int32)
        ix = np.clip((mp[..., 0] + 16) >> 5, 0, W - 1)
        iy = np.clip((mp[..., 1] + 16) >> 5, 0, H - 1)
    D = np.asarray(depth_mm, dtype=np.uint16)[iy, ix].astype(np.float64) * 0.001
    ok = (D > 0.0) & (D <= float(max_dist))
    dc0 = (xs.astype(np.float64) - cx) / fx
    dc1 = (ys.astype(np.float64) - cy) / fy
    pc = (D * dc0, D * dc1, D)
    p = [((T[a, 0] * pc[0] + T[a, 1] * pc[1]) + T[a, 2] * pc[2]) + T[a, 3] for a in range(3)]
    hh = [p[a] - T0[a, 3] for a in range(3)]
    q = [(T0[0, a] * hh[0] + T0[1, a] * hh[1]) + T0[2, a] * hh[2] for a in range(3)]
    ok &= q[2] > 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        fu = np.floor((fx * q[0] / q[2] + cx) + 0.5)
        fv = np.floor((fy * q[1] / q[2] + cy) + 0.5)
        ok &= (fu >= 0.0) & (fu < W) & (fv >= 0.0) & (fv < H)
    mx = np.where(ok, fu, 0.0).astype(np.int64)
    my = np.where(ok, fv, 0.0).astype(np.int64)
    ok &= usable[my, mx]
    V, n = Vm[my, mx], nrm[my, mx]
    e = [p[a] - V[..., a] for a in range(3)]
    ok &= (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= float(max_distance) * float(max_distance)
    r = (n[..., 0] * e[0] + n[..., 1] * e[1]) + n[..., 2] * e[2]
    J = [n[..., 0], n[..., 1], n[..., 2], p[1] * n[..., 2] - p[2] * n[..., 1], p[2] * n[..., 0] - p[0] * n[..., 2],
         p[0] * n[..., 1] - p[1] * n[..., 0]]
    out = np.zeros((H, W, N_TERMS))
    for k, (i, j) in enumerate(_UPPER):
        out[..., k] = J[i] * J[j]
    for i in range(6):
        out[..., 21 + i] = -(J[i] * r)
    out[..., 27] = r * r
    out[..., 28] = 1.0
    out[~ok] = 0.0
    return out


def solve_ldlt(sums: np.ndarray, min_pivot: float):
    """Rule 4: (x [6] or None when degenerate, the smallest d[j] / max_i A[i][i] met)."""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(_UPPER):
        A[i, j] = A[j, i] = sums[k]
    b = [float(v) for v in sums[21:27]]
    top = max(float(A[i, i]) for i in range(6))
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    ratio = math.inf
    for j in range(6):
        g = [L[j][k] * d[k] for k in range(j)]
        v = float(A[j, j])
        for k in range(j):
            v = v - L[j][k] * g[k]
        d[j] = v
        if top > 0.0:
            ratio = min(ratio, v / top)
        if not v > float(min_pivot) * top:
            return None, (ratio if top > 0.0 else 0.0)
        for i in range(j + 1, 6):
            s = float(A[i, j])
            for k in range(j):
                s = s - L[i][k] * g[k]
            L[i][j] = s / v
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i] / d[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return np.array(x), ratio


def update_pose(T: np.ndarray, x: np.ndarray):
    """Rule 5: (the new pose, |t|^2, theta^2)."""
    t, w = [float(v) for v in x[:3]], [float(v) for v in x[3:]]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    a, b = 1.0, 0.5
    if th2 != 0.0:
        th = math.sqrt(th2)
        a, b = math.sin(th) / th, (1.0 - math.cos(th)) / th2
    K = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    Q = [[((1.0 if i == j else 0.0) + a * K[i][j]) + b * (w[i] * w[j] - (th2 if i == j else 0.0)) for j in range(3)]
         for i in range(3)]
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = (Q[i][0] * T[0, j] + Q[i][1] * T[1, j]) + Q[i][2] * T[2, j]
        out[i, 3] = ((Q[i][0] * T[0, 3] + Q[i][1] * T[1, 3]) + Q[i][2] * T[2, 3]) + t[i]
    return out, (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2], th2


def within_limits(T: np.ndarray, T0: np.ndarray, max_translation: float, max_rotation: float) -> bool:
    """Rule 7's two tests."""
    c = [T[a, 3] - T0[a, 3] for a in range(3)]
    cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
    tr = 0.0
    for i in range(3):
        for j in range(3):
            tr = tr + T[i, j] * T0[i, j]
    return bool(cc <= float(max_translation) * float(max_translation) and tr >= 1.0 + 2.0 * math.cos(float(max_rotation)))


def _rms(sums) -> float:
    return math.sqrt(sums[27] / sums[28]) if sums[28] > 0 else 0.0


def align_frame(tsdf, weight, origin, s, cam, depth_mm, world_T_cam, max_dist=10.0, undistort=None, model=None,
                **params) -> dict:
    """One frame: ``world_T_cam`` [4][4] (the aligned pose, or ``T0`` as it came), ``status``,
    ``iterations``, ``inliers`` (first, last), ``rms`` (first, last), ``normal_eq`` f64 [28]; for
    measurements also ``history`` (per iteration: inliers, rms, pivot ratio).  ``model``: the model
    images (``depth_m``, ``normal``) when they were rendered elsewhere."""
    prm = {**DEFAULTS, **params}
    check_align_params(**prm)
    T0 = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    P0 = np.eye(4)                      # T0 as the device keeps it: three rows, then 0 0 0 1
    P0[:3] = T0[:3]
    out = {"world_T_cam": P0.copy(), "status": UNUSED, "iterations": 0, "inliers": (0, 0), "rms": (0.0, 0.0),
           "normal_eq": np.zeros(28), "history": []}
    if not math.isfinite(T0[0, 0]):
        return out
    if model is None:
        model = render_view(tsdf, weight, origin, s, cam, T0, min_weight=prm["min_weight"], min_depth=0.0,
                            max_depth=prm["max_depth"], step_scale=prm["step_scale"])
    usable, Vm, nrm = model_vertices(model, cam, P0)
    T = P0.copy()
    first = None
    status = OK
    for it in range(1, prm["iterations"] + 1):
        sums = reduce_view(pixel_terms(depth_mm, cam, undistort, max_dist, T, P0, usable, Vm, nrm, prm["max_distance"]))
        stat = (int(sums[28]), _rms(sums))
        first = first or stat
        out.update(iterations=it, inliers=(first[0], stat[0]), rms=(first[1], stat[1]), normal_eq=sums[:28].copy())
        if stat[0] < prm["min_inliers"]:
            out["history"].append(stat + (None,))
            status = NO_MODEL
            break
        x, ratio = solve_ldlt(sums, prm["min_pivot"])
        out["history"].append(stat + (ratio,))
        if x is None:
            status = DEGENERATE
            break
        T, tt, th2 = update_pose(T, x)
        if tt < prm["eps_translation"] * prm["eps_translation"] and th2 < prm["eps_rotation"] * prm["eps_rotation"]:
            break
    if status == OK and not within_limits(T, P0, prm["max_translation"], prm["max_rotation"]):
        status = REJECTED
    out["status"] = status
    if status == OK:
        out["world_T_cam"] = T
    return out


def align(tsdf, weight, origin, s, cam, depth_mm, poses, models=None, **kw) -> dict:
    """``align_frame`` of every frame, stacked: ``depth_mm`` [n][H][W], ``poses`` [n][4][4]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    res = [align_frame(tsdf, weight, origin, s, cam, depth_mm[i], poses[i], model=None if models is None else models[i], **kw)
           for i in range(poses.shape[0])]
    return {"world_T_cam": np.stack([r["world_T_cam"] for r in res]),
            "stats": np.array([[r["status"], r["iterations"], r["inliers"][0], r["inliers"][1]] for r in res], dtype=np.int32),
            "residuals": np.array([r["rms"] for r in res]), "normal_eq": np.stack([r["normal_eq"] for r in res]),
            "history": [r["history"] for r in res]}
