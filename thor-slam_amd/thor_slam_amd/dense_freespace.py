"""Masked objects that come to rest enter the map: the free-space layer (``tslam_tsdf_freespace_init``
/ ``tslam_tsdf_freespace_read`` / ``tslam_tsdf_freespace_write``; ``k_tsdf_freespace.hip``;
``HipSlamConfig.dense_dynamic_settle_frames``).  The free-space mask of ``dense_dynamic.py`` has no
memory: a chair that is moved, a door that is closed or a pallet that is set down in known free space
would be masked for ever, and masked depth is never integrated, so the map there would never stop
saying "free".  This layer counts, per voxel, the consecutive frames that saw a surface in it, and
releases the voxel to the map after ``settle_frames`` of them (the job of nvblox's free-space layer).
This file is the spec, a NumPy reference of every operation the device performs, restated for the
tests in ``tests/ref_tsdf_freespace.py``.

All arithmetic is IEEE f64, one rounding per written operation (no fused multiply-add), sums in the
written order, as in ``dense_dynamic.py``.

* **The layer**: one ``uint32`` word per voxel, ``[nz][ny][nx]``.  Bits 0..15 are ``run``, the
  consecutive occupied observations, saturating at 65535; bit 16 is ``settled``; higher bits are 0.
  A new layer is all zero.
* **Parameters**: ``settle_frames`` 1..65535; ``occupied_band_vox`` finite with
  ``0 < occupied_band_vox <= trunc_vox`` of the volume (the upper bound keeps the integrator's brick
  cull conservative for this walk too).  ``band = occupied_band_vox * s``, computed once.
* **Observation** of voxel (i, j, k) by a used frame (``k_tsdf_integrate``'s steps, expression for
  expression):

  1. the centre ``c[a] = o[a] + s * (index[a] + 0.5)`` from the *effective* origin ``o`` (under a
     rolling window ``o[a] = origin[a] + s * float(shift[a])``);
  2. ``cam_T_world = (Q, t)`` from ``world_T_cam = T``: ``Q[r][k] = T[k][r]``,
     ``t[r] = -((T[0][r] T[0][3] + T[1][r] T[1][3]) + T[2][r] T[2][3])``;
     ``p[r] = ((Q[r][0] c0 + Q[r][1] c1) + Q[r][2] c2) + t[r]``;
  3. ``p2 > 0``;
  4. ``ix = floor((fx p0 / p2 + cx) + 0.5)``, ``iy = floor((fy p1 / p2 + cy) + 0.5)``, inside the image;
  5. for a raw camera, the table lookup ``clamp((map[iy][ix][k] + 16) >> 5, 0, size - 1)``;
  6. ``d = mm * 0.001`` with ``0 < d <= max_dist``;
  7. ``sdf = d - p2``.

  If a step fails there is no observation.  Otherwise ``sdf < -band``: none (occluded), the word is
  unchanged; ``-band <= sdf <= band``: *occupied*, ``run = min(run + 1, 65535)`` and ``settled`` is
  set once ``run >= settle_frames``; ``sdf > band``: *free*, ``run = 0`` and ``settled`` is cleared.
  The depth is the call's **raw** input depth, not the mask's filtered copy.
* **Use in the mask**: step 4 of ``dense_dynamic.py`` gains one term while the layer exists: a pixel
  is a candidate only if its voxel's word has ``settled == 0``.
* **Order within a ``tslam_tsdf_dynamic`` call**: all frames of the call are classified against the
  volume and the layer as the stream finds them; after the mask outputs are written, the layer is
  updated with the call's used frames in frame order (a frame on a NaN pose, or an untracked batch
  frame, observes nothing).  A release therefore takes effect from the next call; with the engine that
  is the next batch.

Known limits.  The occupied test is voxel-projective (the voxel's centre against the pixel it
projects to) while the candidate test is pixel-lands-in-voxel: after a release a thin rim of
candidates can remain on an object's silhouette; the opening removes it at ``open_radius >= 1``.
``run`` counts observing frames, not time.

Out of scope: time-based durations, TSDF decay, rigs, aligned and archived integration, sharded
engines, a dynamic occupancy layer for the masked points.
"""

from __future__ import annotations

import math

import numpy as np

from . import dense_dynamic as DD

RUN_MASK, SETTLED, RUN_MAX = 0xFFFF, 0x10000, 65535
DEFAULT_BAND_VOX = 1.5


def check_freespace_params(settle_frames, occupied_band_vox, trunc_vox=None) -> None:
    """``tslam_tsdf_freespace_init`` refuses the same settings (``trunc_vox``: the volume's, when known)."""
    if isinstance(settle_frames, bool) or not isinstance(settle_frames, (int, np.integer)):
        raise ValueError("settle_frames must be an integer")
    b = occupied_band_vox
    if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)) or not math.isfinite(float(b)):
        raise ValueError("occupied_band_vox must be a finite number")
    if not 1 <= settle_frames <= RUN_MAX:
        raise ValueError(f"settle_frames must be 1..{RUN_MAX}")
    if not float(b) > 0:
        raise ValueError("occupied_band_vox must be > 0")
    if trunc_vox is not None and not float(b) <= float(trunc_vox):
        raise ValueError("occupied_band_vox must be <= trunc_vox (the truncation distance in voxels)")


def check_words(words) -> None:
    """``tslam_tsdf_freespace_write`` refuses a word with a bit above 16."""
    if (np.asarray(words, dtype=np.uint32) & ~np.uint32(RUN_MASK | SETTLED)).any():
        raise ValueError("bits above 16 must be 0")


def split(words) -> tuple[np.ndarray, np.ndarray]:
    """(``run`` u16, ``settled`` bool) of a layer."""
    w = np.asarray(words, dtype=np.uint32)
    return (w & np.uint32(RUN_MASK)).astype(np.uint16), (w & np.uint32(SETTLED)) != 0


def cam_T_world(world_T_cam) -> tuple[np.ndarray, np.ndarray]:
    """Step 2's table entry: (Q [3][3], t [3]) as ``k_tsdf_poses`` writes them."""
    T = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    Q = T[:3, :3].T.copy()
    t = np.array([-((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3]) for r in range(3)])
    return Q, t


def observe(dims, origin, s, cam, depth_mm, world_T_cam, max_dist, band, undistort=None):
    """Steps 1-7 for every voxel: (occupied, free), booleans [nz][ny][nx]."""
    W, H, fx, fy, cx, cy = int(cam[0]), int(cam[1]), *[float(v) for v in cam[2:]]
    nx, ny, nz = (int(n) for n in dims)
    s = float(s)
    d_img = np.asarray(depth_mm, dtype=np.uint16).reshape(H, W)
    T = np.array(world_T_cam, dtype=np.float64).reshape(4, 4)
    none = np.zeros((nz, ny, nx), dtype=bool)
    if not math.isfinite(T[0, 0]):
        return none, none.copy()
    Q, t = cam_T_world(T)
    X = (float(origin[0]) + s * (np.arange(nx, dtype=np.float64) + 0.5))[None, None, :]
    Y = (float(origin[1]) + s * (np.arange(ny, dtype=np.float64) + 0.5))[None, :, None]
    Z = (float(origin[2]) + s * (np.arange(nz, dtype=np.float64) + 0.5))[:, None, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = [((Q[r, 0] * X + Q[r, 1] * Y) + Q[r, 2] * Z) + t[r] for r in range(3)]
        ok = p[2] > 0.0
        fu = np.floor((fx * p[0] / p[2] + cx) + 0.5)
        fv = np.floor((fy * p[1] / p[2] + cy) + 0.5)
        ok &= (fu >= 0.0) & (fu < W) & (fv >= 0.0) & (fv < H)
    ix = np.where(ok, fu, 0.0).astype(np.int64)
    iy = np.where(ok, fv, 0.0).astype(np.int64)
    if undistort is not None:
        mp = np.asarray(undistort, dtype=np.int32).reshape(H, W, 2)[iy, ix].astype(np.int64)
        ix = np.clip((mp[..., 0] + 16) >> 5, 0, W - 1)
        iy = np.clip((mp[..., 1] + 16) >> 5, 0, H - 1)
    d = d_img[iy, ix].astype(np.float64) * 0.001
    ok &= (d > 0.0) & (d <= float(max_dist))
    with np.errstate(invalid="ignore"):
        sdf = d - p[2]
        return ok & (sdf >= -band) & (sdf <= band), ok & (sdf > band)


def update_frame(words, origin, s, cam, depth_mm, world_T_cam, max_dist, band, settle_frames, undistort=None) -> np.ndarray:
    """The layer after one frame (a new array)."""
    w = np.array(words, dtype=np.uint32)
    occ, free = observe(w.shape[::-1], origin, s, cam, depth_mm, world_T_cam, max_dist, band, undistort)
    run = np.minimum((w & np.uint32(RUN_MASK)) + np.uint32(1), np.uint32(RUN_MAX))
    settled = (w & np.uint32(SETTLED)) | np.where(run >= np.uint32(settle_frames), np.uint32(SETTLED), np.uint32(0))
    w = np.where(occ, settled | run, w)
    return np.where(free, np.uint32(0), w).astype(np.uint32)


def update(words, origin, s, cam, depth_mm, poses, max_dist, band, settle_frames, undistort=None) -> np.ndarray:
    """The layer after the frames of a call, in frame order: ``depth_mm`` [n][H][W], ``poses`` [n][4][4]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    w = np.array(words, dtype=np.uint32)
    for f in range(poses.shape[0]):
        w = update_frame(w, origin, s, cam, depth_mm[f], poses[f], max_dist, band, settle_frames, undistort)
    return w


def dynamic(tsdf, weight, words, origin, s, trunc, cam, depth_mm, poses, settle_frames, occupied_band_vox, max_dist=10.0,
            undistort=None, **params) -> dict:
    """One ``tslam_tsdf_dynamic`` call with the layer on: ``dense_dynamic.dynamic``'s outputs, every
    frame classified against ``words`` as they stand, and ``words``: the layer after the call."""
    check_freespace_params(settle_frames, occupied_band_vox)
    check_words(words)
    out = DD.dynamic(tsdf, weight, origin, s, trunc, cam, depth_mm, poses, max_dist=max_dist, undistort=undistort,
                     layer=np.asarray(words, dtype=np.uint32), **params)
    band = float(occupied_band_vox) * float(s)
    out["words"] = update(words, origin, s, cam, depth_mm, poses, max_dist, band, settle_frames, undistort)
    return out
