"""The dense map from several cameras of a rig, restated for the tests
(``thor_slam_amd/dense_rig.py`` is the product's spec; ``k_tsdf.hip`` the device code).

Nothing here but ``oracle.numpy_tsdf.integrate`` (one view into the volume),
``oracle.numpy_rig.mul4`` and ``oracle.numpy_rig.inv_rigid`` (the device's summation orders):

* view ``v = f * n_cams + ci`` in ascending v (frame-major, camera-minor);
* ``world_T_cam = mul4(mul4(inv_rigid(E[0]), T_abs(f)), E[pair])`` with ``E[p] = base_T_rect[p]``
  and ``T_abs`` the body's world_T_base (base at frame 0); the volume's frame is pair 0's rectified
  left camera at frame 0;
* ``cam_T_world = [R^T | -((r0 t0 + r1 t1) + r2 t2)]``;
* a frame's views are all used or all skipped: device poses, the rig's status is 0, or the frame
  is the global first one with status 2 (what ``k_rig_pose`` writes there); host poses, a NaN in
  ``world_T_base[f][0][0]`` skips it;
* camera ci: pair's intrinsics, and the raw camera's undistortion table unless the depth lives in
  the rectified camera already.
"""

from __future__ import annotations

import numpy as np

from oracle.numpy_rig import inv_rigid, mul4
from oracle.numpy_tsdf import integrate


def new_volume(dims) -> dict:
    """Empty volume and colour layer, [nz][ny][nx]."""
    shape = tuple(dims)[::-1]
    return {"tsdf": np.zeros(shape, np.float32), "weight": np.zeros(shape, np.float32),
            "color": np.zeros(shape + (3,), np.float32), "color_weight": np.zeros(shape, np.float32)}


def cam_T_world(T: np.ndarray) -> np.ndarray:
    out = np.eye(4)
    for r in range(3):
        for k in range(3):
            out[r, k] = T[k, r]
        out[r, 3] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return out


def world_T_cam(E: list, T_abs: np.ndarray, pair: int) -> np.ndarray:
    return mul4(mul4(inv_rigid(np.asarray(E[0], float)), np.asarray(T_abs, float)), np.asarray(E[pair], float))


def used_device(stats, g0: int = 0) -> list:
    """Use flags of a batch from the rig's status per frame (``read_rig_poses()["stats"][:, 0]``)."""
    return [int(s) == 0 or (int(s) == 2 and g0 + f == 0) for f, s in enumerate(stats)]


def used_host(world_T_base) -> list:
    return [bool(np.isfinite(np.asarray(T)[0, 0])) for T in world_T_base]


def integrate_rig(vol: dict, pairs, depth, world_T_base, used, E, rects, origin, s, trunc, max_dist, max_weight,
                  bgr=None, rect: bool = False, order: str = "frame") -> dict:
    """``depth[f][ci]`` u16 mm of camera ci = pair ``pairs[ci]`` (``bgr[f][ci]`` its colour, or None)
    into ``vol`` in place.  ``order``: "frame" is the rule; "camera" (camera-major) is what one
    launch per camera would do, for the test that tells the two apart."""
    n_frames, n_cams = len(depth), len(pairs)
    assert list(pairs) == sorted(set(pairs))
    views = [(f, ci) for f in range(n_frames) for ci in range(n_cams)]
    if order == "camera":
        views = [(f, ci) for ci in range(n_cams) for f in range(n_frames)]
    for f, ci in views:
        if not used[f]:
            continue
        p = pairs[ci]
        r = rects[p]
        mp = None if (rect or r.is_identity) else r.map_left
        integrate(vol["tsdf"], vol["weight"], depth[f][ci], cam_T_world(world_T_cam(E, world_T_base[f], p)),
                  (r.fx, r.fy, r.cx, r.cy), origin, s, trunc, max_dist, max_weight, mp,
                  bgr=None if bgr is None else bgr[f][ci], color=vol["color"], color_w=vol["color_weight"])
    return vol
