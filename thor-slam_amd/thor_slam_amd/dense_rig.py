"""The dense map from several cameras of a rig (``HipSlamConfig.dense_cameras``;
``tslam_tsdf_integrate_rig``, ``k_tsdf.hip``): which views are integrated, in which order, and on
which pose.  The per-voxel update of a view is the one of ``oracle/numpy_tsdf.py``; this file is the
spec of everything around it, restated for the tests in ``tests/ref_tsdf_rig.py``.

The reference's dense-map interface is a list of cameras (``config/slam_config.yaml:61-68``
``nvblox_cameras``, ``scripts/run_pipeline.py:371-392`` one topic set per listed camera,
``launch/thor_nvblox.launch.py:23`` ``num_cameras``); ``dense_cameras`` is that list.

* **Views and their order.**  A call names ``n_cams`` cameras (pairs of the handle, strictly
  ascending) and ``n_frames`` frames.  View ``v = f * n_cams + ci``; views are integrated in
  ascending ``v``: frame-major, camera-minor.  A batch therefore equals one call per frame, and the
  volume does not depend on the batch size, also once a weight has reached ``max_weight``.
* **Volume frame.**  Pair 0's rectified left camera at frame 0 (RDF), as with one camera.
* **Pose of a view.**  With ``E_p = base_T_rect[p]``, ``E_p^-1 = [R^T | -((r0 t0 + r1 t1) + r2 t2)]``
  and ``T = world_T_base(f)`` (the body's ``T_abs``, base at frame 0):
  ``world_T_cam = (E_0^-1 T) E_p``, every element of a product summed as
  ``((a0 b0 + a1 b1) + a2 b2) + a3 b3``; then ``cam_T_world = [R^T | -((r0 t0 + r1 t1) + r2 t2)]``.
  No fused multiply-add anywhere, so NumPy reproduces the device bit for bit.
* **Use flag.**  A frame's views are all used or all skipped.  Device poses: the rig's status is 0
  (tracked), or the frame is the global first frame (status 2 there: ``k_rig_pose`` writes the
  identity and ``TS_INIT``).  Host poses: a NaN in ``world_T_base[f][0][0]`` skips the frame.
* **Per camera.**  The pair's intrinsics; the raw camera's undistortion table for depth of the raw
  camera (RGB-D records) and none for depth of the rectified camera (dense stereo depth); its own
  depth (and optionally BGR colour) base pointer and frame stride.
* **Chunks.**  The kernel's pose table holds 256 views; more go in chunks of ``256 // n_cams`` whole
  frames, in order.
"""

from __future__ import annotations

import numpy as np

MAX_VIEWS = 256   # TSDF_MAX_FRAMES: views per launch
MAX_CAMS = 8      # TS_RIG_MAXP


class DenseCamerasError(ValueError):
    """A ``dense_cameras`` setting that cannot be honoured (``HipSlamConfig.validate`` and
    ``HipSlamEngine.initialize`` raise it as it is, a ValueError)."""


def mul4(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """4x4 product in the device's summation order (``mul4_fixed``)."""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            out[i, j] = ((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j]
    return out


def inv_rigid(e: np.ndarray) -> np.ndarray:
    """[R^T | -R^T t] in the device's expression order (``set_rig_E``, ``k_tsdf_rig_poses``)."""
    out = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = e[j, i]
        out[i, 3] = -((e[0, i] * e[0, 3] + e[1, i] * e[1, 3]) + e[2, i] * e[2, 3])
    out[3, 3] = 1.0
    return out


def rig_world_T_cam(base_T_rect: list, world_T_base: np.ndarray, pair: int) -> np.ndarray:
    """Pose of pair ``pair``'s rectified left camera in the volume's frame, from the body pose."""
    return mul4(mul4(inv_rigid(np.asarray(base_T_rect[0], dtype=np.float64)), np.asarray(world_T_base, dtype=np.float64)),
                np.asarray(base_T_rect[pair], dtype=np.float64))


def frame_used(status: int, global_frame: int) -> bool:
    """Device poses: the rig's stats record of the frame decides for all of its views."""
    return status == 0 or (status == 2 and global_frame == 0)


def chunk_frames(n_cams: int) -> int:
    """Whole frames per launch."""
    return MAX_VIEWS // n_cams


def view_order(n_cams: int, n_frames: int) -> list[tuple[int, int]]:
    """(frame, camera index) of every view in integration order."""
    return [(f, ci) for f in range(n_frames) for ci in range(n_cams)]


def resolve_dense_cameras(spec, source_names: list) -> tuple:
    """``HipSlamConfig.dense_cameras`` -> ascending pair indices.  ``source_names[p]``: the source
    name of pair p's left (RGB-D: colour) camera.  () stays (): pair 0 on its own pose."""
    n = len(source_names)
    if isinstance(spec, str):
        if spec != "all":
            raise DenseCamerasError("dense_cameras must be (), 'all' or a tuple of pair indices / source names")
        entries = list(range(n))
    else:
        entries = list(spec)
    if not entries:
        return ()
    if n < 2:
        raise DenseCamerasError("dense_cameras needs a rig of several pairs (a single pair is the default dense map)")
    pairs = []
    for e in entries:
        if isinstance(e, str):
            if e not in source_names:
                raise DenseCamerasError(f"dense_cameras: unknown camera source {e!r} (have {sorted(set(source_names))})")
            p = source_names.index(e)
        elif isinstance(e, (int, np.integer)) and not isinstance(e, bool):
            p = int(e)
            if not 0 <= p < n:
                raise DenseCamerasError(f"dense_cameras: pair {p} out of range 0..{n - 1}")
        else:
            raise DenseCamerasError(f"dense_cameras entries are pair indices or source names, not {e!r}")
        if p in pairs:
            raise DenseCamerasError(f"dense_cameras names pair {p} twice")
        pairs.append(p)
    if len(pairs) > MAX_CAMS:
        raise DenseCamerasError(f"dense_cameras: at most {MAX_CAMS} cameras")
    return tuple(sorted(pairs))
