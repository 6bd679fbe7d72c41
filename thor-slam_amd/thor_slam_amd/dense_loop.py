"""The dense map kept consistent with poses that change after integration: archived depth frames
moved to their corrected poses (``tslam_tsdf_archive_init`` / ``tslam_tsdf_archive_integrate`` /
``tslam_tsdf_archive_move`` / ``tslam_tsdf_archive_read`` / ``tslam_tsdf_archive_read_depth``;
``k_tsdf_move_frames.hip``; ``HipSlamConfig.dense_loop``).  A loop closure or a relocalisation
corrects the keyframe poses after their depth went into the volume; BundleFusion's remedy is to keep
the depth frames, take a frame whose pose changed out of the volume at its old pose and integrate it
again at the new one.  This file is the spec and holds the host helpers; its restatement for the
tests is ``tests/ref_tsdf_move.py``.

All arithmetic is IEEE f64, one rounding per written operation (no fused multiply-add), sums in the
written order; ``tsdf`` and ``weight`` are stored as f32 after every update.

* **Pose entries.**  The integrator works on a 13-double entry ``q`` per frame: ``cam_T_world`` as
  ``q[3 r + k] = T[k][r]`` (R transposed), ``q[9 + r] = -((T[0][r] T[0][3] + T[1][r] T[1][3]) +
  T[2][r] T[2][3])`` from ``T = world_T_cam``, and a use flag.  The camera centre of an entry:
  ``C[a] = -((q[a] q[9] + q[3 + a] q[10]) + q[6 + a] q[11])``.
* **Observation** of a voxel centre ``c`` by a frame (the integrator's test, operation for
  operation): ``p = R c + t`` row-wise; need ``p_z > 0``; ``ix = floor(fx p_x / p_z + cx + 1/2)``,
  ``iy`` alike, inside the image; through the undistortion table when the camera has one;
  ``d = mm * 0.001``, need ``0 < d <= max_dist``; ``sdf = d - p_z``, need ``sdf >= -trunc``;
  ``obs = min(sdf, trunc)``.
* **Integration**: ``w' = w + 1``; ``tsdf' = (tsdf w + obs) / w'``; ``w' = min(w', max_weight)``.
* **De-integration**, its inverse: ``w' = w - 1``; if ``w' > 0``: ``tsdf' = (tsdf w - obs) / w'``
  and the weight is ``w'``; else ``tsdf' = 0`` and the weight 0 (the voxel is unobserved again).
  The test is deterministic, so a de-integration on the very entry a frame was integrated with meets
  exactly the voxels the integration met.  The archive therefore stores that entry, copied on the
  device, never recomputed.
* **The archive** is a ring of ``capacity`` frames.  An integrate call takes the frames
  ``first_frame + i`` with ``(first_frame + i) % interval == 0`` whose pose is used (a host pose
  whose first element is finite; a tracked batch frame, on ``world_T_corr * T_abs`` with the product
  in ``mul4``'s order) and only those; they are integrated, and the r-th of them takes slot
  ``(count + r) % capacity`` with its depth image, its entry and ``world_T_cam``; ``count`` grows by
  their number.  *Archive order* is oldest first: numbers ``count - min(count, capacity) .. count - 1``.
  A frame that left the ring stays in the volume as it is.
* **Selection.**  A move names frames and new poses ``world_T_cam``; the last entry that names a
  frame counts, frames not in the ring and poses whose first element is not finite are ignored.
  With ``qo`` the stored entry and ``qn`` the new pose's: ``d = C(qn) - C(qo)``,
  ``dd = (d0 d0 + d1 d1) + d2 d2``, ``tr = (((0 + qo[0] qn[0]) + qo[1] qn[1]) + ...) + qo[8] qn[8]``
  (= trace(R_old^T R_new)); the frame moves when ``dd > min_translation^2`` or
  ``tr < 1 + 2 cos(min_rotation)``, the right sides computed on the host.
* **The move.**  The selected frames in archive order; each is de-integrated on its stored entry and
  then integrated on the new one (per voxel this is the order of the updates; a voxel is loaded once
  and stored once per call).  Afterwards the stored entry and pose of a moved frame are the new ones.
* **Saturation.**  Where a voxel's weight had reached ``max_weight`` history is lost: the removal
  then treats the frame as one of the last ``max_weight`` observations, and a voxel whose weight is
  driven to 0 that way restarts from the re-inserted frames alone.  That is approximate, as it is in
  BundleFusion; the move equals a rebuild from scratch, up to f32 rounding, only where no weight
  saturated.  ``dense_loop`` therefore wants ``tsdf_max_weight`` above the number of frames that see
  a voxel.
* **Not moved**: the colour layer, rig cameras (``dense_cameras``), a following window.
"""

from __future__ import annotations

import math

import numpy as np

MOVE_CHUNK = 128   # TSDF_MOVE_CHUNK: selected frames whose pose tables sit in LDS at a time


def check_loop_params(capacity, min_translation, min_rotation) -> None:
    """``tslam_tsdf_archive_init`` / ``tslam_tsdf_archive_move`` refuse the same settings."""
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 1:
        raise ValueError("dense_loop_capacity must be an integer >= 1")
    if min_translation is not None and not (isinstance(min_translation, (int, float)) and 0 <= min_translation < math.inf):
        raise ValueError("dense_loop_min_translation_m must be None or a finite distance >= 0")
    if not (isinstance(min_rotation, (int, float)) and 0 <= min_rotation <= math.pi):
        raise ValueError("dense_loop_min_rotation_rad must be in [0, pi]")


def pose_entry(world_T_cam: np.ndarray) -> np.ndarray:
    """The 12 pose doubles of the integrator's entry for ``world_T_cam`` [4][4] (rule "Pose entries")."""
    T = np.asarray(world_T_cam, dtype=np.float64).reshape(4, 4)
    q = np.zeros(12)
    for r in range(3):
        for k in range(3):
            q[3 * r + k] = T[k, r]
        q[9 + r] = -((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3])
    return q


def entry_centre(q: np.ndarray) -> np.ndarray:
    return np.array([-((q[a] * q[9] + q[3 + a] * q[10]) + q[6 + a] * q[11]) for a in range(3)])


def moves(q_old: np.ndarray, q_new: np.ndarray, min_translation: float, min_rotation: float) -> bool:
    """Rule "Selection" for one frame that is in the ring and has a finite new pose."""
    d = entry_centre(q_new) - entry_centre(q_old)
    dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    tr = 0.0
    for k in range(9):
        tr = tr + q_old[k] * q_new[k]
    return bool(dd > float(min_translation) * float(min_translation) or tr < 1.0 + 2.0 * math.cos(float(min_rotation)))
