"""The dense map's rolling window, restated for the tests (``thor_slam_amd/dense_follow.py`` is the
product's spec; ``k_tsdf_follow`` / ``k_tsdf_shift`` / ``k_tsdf_move`` the device code).  Written on
its own: nothing of the rule is imported from the product.

* state: a cumulative shift (3 ints, voxels), zero at the start;
* effective origin ``o0 + s * float(shift)`` per axis, recomputed from the shift every time;
* a move by delta: ``new[k, j, i] = old[k + dz, j + dy, i + dx]`` inside the volume, 0 elsewhere,
  for every layer; then ``shift += delta``;
* the decision of a call: the first view (at most 256 looked at) whose use flag is set; its camera
  centre ``C[a] = -((R[0, a] t0 + R[1, a] t1) + R[2, a] t2)`` of ``cam_T_world = [R | t]``;
  ``e = floor((C - o_eff) / s) - anchor``; ``delta = step * trunc(e / step)`` where ``|e| > margin``;
  nothing moves without a used view, with a centre that is not finite, or at 2^30 voxels.
"""

from __future__ import annotations

import math

import numpy as np

from oracle.numpy_tsdf import integrate

TWO30 = 2 ** 30


def cam_T_world(T: np.ndarray) -> np.ndarray:
    """[R^T | -R^T t] of world_T_cam in k_tsdf_poses' expression order."""
    out = np.eye(4)
    for r in range(3):
        for k in range(3):
            out[r, k] = T[k, r]
        out[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return out


def centre(cTw: np.ndarray) -> list:
    """The camera centre in the volume's frame from cam_T_world."""
    R, t = cTw[:3, :3], cTw[:3, 3]
    with np.errstate(invalid="ignore"):
        return [float(-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2])) for a in range(3)]


def origin_of(o0, s, shift) -> tuple:
    return tuple(float(o0[a]) + float(s) * float(int(shift[a])) for a in range(3))


def trunc_div(e: int, step: int) -> int:
    q = abs(e) // step
    return q if e >= 0 else -q


def decide(views, o0, s, shift, anchor, margin, step) -> tuple:
    """``views``: (cam_T_world, used) of the call's views in order.  -> delta."""
    first = next((cTw for cTw, used in list(views)[:256] if used), None)
    if first is None:
        return (0, 0, 0)
    C = centre(np.asarray(first, dtype=np.float64))
    if not all(math.isfinite(c) for c in C):
        return (0, 0, 0)
    o = origin_of(o0, s, shift)
    delta = [0, 0, 0]
    for a in range(3):
        c = math.floor((C[a] - o[a]) / s)
        if abs(c) >= TWO30:
            return (0, 0, 0)
        e = int(c) - int(anchor[a])
        if abs(e) > margin:
            delta[a] = step * trunc_div(e, step)
        if abs(int(shift[a]) + delta[a]) >= TWO30:
            return (0, 0, 0)
    return tuple(delta)


def move(layer: np.ndarray, delta) -> np.ndarray:
    """One layer [nz][ny][nx](+[3]) moved by delta = (dx, dy, dz)."""
    nz, ny, nx = layer.shape[:3]
    dx, dy, dz = (int(d) for d in delta)
    k, j, i = np.meshgrid(np.arange(nz) + dz, np.arange(ny) + dy, np.arange(nx) + dx, indexing="ij")
    ok = (k >= 0) & (k < nz) & (j >= 0) & (j < ny) & (i >= 0) & (i < nx)
    out = np.zeros_like(layer)
    out[ok] = layer[k[ok], j[ok], i[ok]]
    return out


class Window:
    """A following (or hand-moved) volume: a sequence of calls through ``oracle.numpy_tsdf.integrate``
    at the effective origin."""

    def __init__(self, o0, dims, s, trunc, max_dist, max_weight, anchor=None, margin=None, step=None):
        shape = tuple(dims)[::-1]
        self.o0, self.s, self.trunc, self.max_dist, self.max_weight = tuple(o0), s, trunc, max_dist, max_weight
        self.vol = {"tsdf": np.zeros(shape, np.float32), "weight": np.zeros(shape, np.float32),
                    "color": np.zeros(shape + (3,), np.float32), "color_weight": np.zeros(shape, np.float32)}
        self.shift = [0, 0, 0]
        self.anchor = tuple(math.floor(-o / s) for o in o0) if anchor is None else tuple(anchor)
        self.margin, self.step = margin, step           # margin None: not following
        self.moves = []                                 # delta of every call

    @property
    def origin(self) -> tuple:
        return origin_of(self.o0, self.s, self.shift)

    def shift_by(self, delta) -> None:
        if any(abs(self.shift[a] + int(delta[a])) >= TWO30 for a in range(3)):
            delta = (0, 0, 0)
        if any(delta):
            for key in self.vol:
                self.vol[key] = move(self.vol[key], delta)
        self.shift = [self.shift[a] + int(delta[a]) for a in range(3)]

    def call(self, views) -> tuple:
        """One integrate call.  ``views``: dicts with ``cTw`` (cam_T_world), ``used``, ``depth``,
        ``intr`` and optionally ``map`` and ``bgr``, in integration order."""
        delta = (0, 0, 0)
        if self.margin is not None:
            delta = decide([(v["cTw"], v["used"]) for v in views], self.o0, self.s, self.shift, self.anchor,
                           self.margin, self.step)
            self.shift_by(delta)
        self.moves.append(delta)
        o = self.origin
        for v in views:
            if v["used"]:
                integrate(self.vol["tsdf"], self.vol["weight"], v["depth"], v["cTw"], v["intr"], o, self.s, self.trunc,
                          self.max_dist, self.max_weight, v.get("map"), bgr=v.get("bgr"), color=self.vol["color"],
                          color_w=self.vol["color_weight"])
        return delta
