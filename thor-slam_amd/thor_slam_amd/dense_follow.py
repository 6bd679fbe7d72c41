"""The dense map's rolling window (``HipSlamConfig.dense_follow``; ``tslam_tsdf_follow``,
``tslam_tsdf_shift``, ``tslam_tsdf_window``; ``k_tsdf_follow`` / ``k_tsdf_shift`` / ``k_tsdf_move``
in ``k_tsdf.hip``): a volume of fixed size that moves with the camera in whole voxels.  Everything
the window still covers is kept, what leaves is dropped, what enters is unobserved.  The per-voxel
update stays the one of ``oracle/numpy_tsdf.py``; this file is the spec of everything around it,
restated for the tests in ``tests/ref_tsdf_follow.py``.

* **State.**  A cumulative integer shift ``shift[3]`` in voxels: zero after ``tslam_tsdf_init`` and
  after ``tslam_reset``.
* **Effective origin.**  Always recomputed from the shift, never accumulated:
  ``o_eff[a] = o0[a] + s * float(shift[a])``, one multiply and one add in f64 (no fused
  multiply-add on the device, so host and device agree).  Voxel (i, j, k) is centred at
  ``o_eff + s * (i + 0.5)`` as before, and the brick cull uses the same ``o_eff``.
* **A move by** ``delta[3]``.  For every layer (tsdf, weight, colour, colour weight)
  ``new(i, j, k) = old(i + dx, j + dy, k + dz)`` where that index lies inside the volume, and 0
  everywhere else; then ``shift += delta``.  ``|delta| >= dim`` on an axis empties the volume.
* **The decision.**  One per integrate call, before the call's first voxel update, from the FIRST
  USED VIEW of the call's FIRST CHUNK (at most 256 views): the first entry of the pose table with a
  non-zero use flag (``q[12]``).  Host poses and device poses, one camera and a rig go through that
  one table; for a rig it is the first selected camera of the first used frame.  With
  ``q = [R (9, row-major), t (3), use]`` of ``cam_T_world``, the camera centre in the volume's frame
  is ``C[a] = -((q[a] q[9] + q[3 + a] q[10]) + q[6 + a] q[11])``, in that order.  Per axis
  ``c = floor((C[a] - o_eff[a]) / s)``, ``e = int(c) - anchor[a]``, and
  ``delta[a] = step * trunc(e / step)`` (C integer division, toward zero) if ``|e| > margin``, else 0.
  The whole decision is "no move" when the chunk has no used view, when ``C`` is not finite, or
  when ``|c|`` or the new ``|shift|`` would reach 2^30 on any axis.
* **Parameters.**  ``1 <= step <= margin < 2^30`` and ``|anchor| < 2^30``: after a move
  ``|e| < step <= margin``, which is the hysteresis.  The default anchor is the voxel that holds the
  tracking world's origin in the unshifted window, ``floor(-o0[a] / s)``, so the configured layout
  of the room around the camera is kept.
* **Grouping matters.**  There is one decision per call, because ``k_tsdf_integrate`` reads and
  writes every voxel once per call; the same frames grouped into other calls can give another
  sequence of moves, and so another volume.  An explicit move (``tslam_tsdf_shift``, also refused
  beyond 2^30) writes the same ``delta`` and ``shift`` and shares everything downstream.
"""

from __future__ import annotations

import math

import numpy as np

LIMIT = 1 << 30        # TSDF_SHIFT_LIMIT
CHUNK = 256            # TSDF_MAX_FRAMES: views of a call's first chunk


def check_follow_params(margin, step, anchor=None) -> None:
    """``HipSlamConfig.validate`` and the library refuse the same settings."""
    for v in (margin, step):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("dense_follow_margin and dense_follow_step must be integers")
    if not 1 <= step <= margin < LIMIT:
        raise ValueError("dense_follow needs 1 <= dense_follow_step <= dense_follow_margin < 2^30")
    if anchor is not None:
        ok = not isinstance(anchor, (str, bytes)) and hasattr(anchor, "__len__") and len(anchor) == 3 and all(
            isinstance(a, (int, np.integer)) and not isinstance(a, bool) and abs(int(a)) < LIMIT for a in anchor)
        if not ok:
            raise ValueError("dense_follow_anchor must be None or three integers (voxels) below 2^30")


def default_anchor(origin, s: float) -> tuple:
    """The voxel of the unshifted window that holds the tracking world's origin."""
    return tuple(int(math.floor(-float(o) / float(s))) for o in origin)


def effective_origin(origin, s: float, shift) -> np.ndarray:
    return np.array([float(o) + float(s) * float(int(k)) for o, k in zip(origin, shift)], dtype=np.float64)


def camera_centre(q) -> list:
    """Of one pose-table entry ``q`` (13 doubles), in the device's expression order."""
    return [-((q[a] * q[9] + q[3 + a] * q[10]) + q[6 + a] * q[11]) for a in range(3)]


def decide(table, origin, s: float, shift, anchor, margin: int, step: int) -> tuple:
    """``delta`` of one integrate call from its first chunk's pose table [n][13]."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, 13)[:CHUNK]
    used = np.nonzero(table[:, 12] != 0.0)[0]
    if used.size == 0:
        return (0, 0, 0)
    C = camera_centre([float(v) for v in table[used[0]]])
    o = effective_origin(origin, s, shift)
    delta = []
    for a in range(3):
        if not math.isfinite(C[a]):
            return (0, 0, 0)
        c = math.floor((C[a] - float(o[a])) / float(s))
        if not abs(c) < LIMIT:
            return (0, 0, 0)
        e = int(c) - int(anchor[a])
        d = (1 if e > 0 else -1) * step * (abs(e) // step) if abs(e) > margin else 0      # toward zero
        if not abs(int(shift[a]) + d) < LIMIT:
            return (0, 0, 0)
        delta.append(d)
    return tuple(delta)


def move_layer(layer: np.ndarray, delta) -> np.ndarray:
    """A layer [nz][ny][nx] (or [nz][ny][nx][3]) moved by ``delta`` = (dx, dy, dz) voxels."""
    out = np.zeros_like(layer)
    nz, ny, nx = layer.shape[:3]
    dx, dy, dz = (int(d) for d in delta)
    src, dst = [], []
    for n, d in ((nz, dz), (ny, dy), (nx, dx)):
        lo, hi = max(0, -d), min(n, n - d)       # destination indices whose source lo + d .. exists
        if lo >= hi:
            return out
        dst.append(slice(lo, hi))
        src.append(slice(lo + d, hi + d))
    out[tuple(dst)] = layer[tuple(src)]
    return out
