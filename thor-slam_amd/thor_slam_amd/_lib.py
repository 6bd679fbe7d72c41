"""ctypes binding of ``libtslam_hip.so`` (C-ABI in ``include/tslam.h``).

The library is built in-tree (``make -C thor-slam_amd/csrc`` or ``__graft_entry__.build()``) and
loaded from this package directory.  There is deliberately no fallback: if the HIP library is
missing or fails to load, every engine constructor raises.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

from .dense_follow import default_anchor
from .params import HipSlamConfig

LIB_NAME = "libtslam_hip.so"
LIB_PATH = Path(__file__).resolve().parent / LIB_NAME

# enum tslam_buffer
BUF = {
    "pyramid": 0, "smooth": 1, "keypoints": 2, "kcount": 3, "desc": 4, "stereo": 5, "disp": 6,
    "temporal": 7, "temporal_uv": 8, "corr": 9, "pose": 10, "stats": 11, "qbest": 12,
    "qsecond": 13, "tbest": 14, "ysorted": 15, "rowstart": 16, "desc_ys": 17, "det_thr": 18, "det_fail": 19,
    "hyp": 20, "ypos": 21, "qtpos": 22,
}
STAGE = {"rectify": 0, "detect": 1, "describe": 2, "match": 3, "pose": 4, "all": 5, "ba": 6}
# single kernels, in pipeline order (bench.py times each with HIP events)
KERNELS = {
    "rectify_pyramid": 10, "detect": 11, "select": 12, "describe": 13,
    "match": 14, "match_refine": 15, "pose": 16, "chain": 17,
}
INE_RECORD = 80   # TSLAM_BA_INE_RECORD: doubles of an inertial factor record
RIG_KERNEL = 18   # rig pose (+ chain; sharded: the range's rig pose only)
POSE_SOLVE_KERNEL = 19   # P3P + RANSAC + refine on injected correspondences (parity tests)
TRANSPORT = {"rccl": 0, "copy": 1}   # tslam_group_create
DET_COUNTERS, DET_COUNTER_BLOCKS = 12, 9   # tslam_detect_counters: words per level (TS_DCNT), index of the block count
SHARD_GATHER, SHARD_RESULTS, SHARD_PROFILE, SHARD_SERIAL, SHARD_PIPELINE, SHARD_SOLO, SHARD_PAIRS = 1, 2, 4, 8, 16, 32, 64   # tslam_shard_options
# tslam_shard_timing segments (enum tslam_segment), in order
SHARD_SEGMENTS = ("rectify_pyramid", "detect", "select", "describe", "pack", "exchange_wait", "import", "match",
                  "match_refine", "pose", "rig", "state", "pose_gather", "chain", "local_ba", "pair_blocks")
POSE_OK, POSE_LOST, POSE_INIT = 0, 1, 2


class StereoDesc(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double),
        ("baseline", ctypes.c_double),
        ("map_left", ctypes.POINTER(ctypes.c_int32)), ("map_right", ctypes.POINTER(ctypes.c_int32)),
    ]


class Params(ctypes.Structure):
    _fields_ = [
        ("n_features", ctypes.c_int32), ("n_levels", ctypes.c_int32), ("fast_threshold", ctypes.c_int32),
        ("edge_margin", ctypes.c_int32), ("max_hamming", ctypes.c_int32), ("ratio_pct", ctypes.c_int32),
        ("stereo_row_tol", ctypes.c_int32), ("max_disparity", ctypes.c_int32), ("temporal_window", ctypes.c_int32),
        ("ransac_hypotheses", ctypes.c_int32), ("refine_iters", ctypes.c_int32), ("min_inliers", ctypes.c_int32),
        ("ransac_thr_px", ctypes.c_double), ("ransac_seed", ctypes.c_uint64),
        ("max_batch", ctypes.c_int32), ("n_pairs", ctypes.c_int32), ("ransac_splits", ctypes.c_int32),
        ("ba_window", ctypes.c_int32), ("ba_kf_interval", ctypes.c_int32), ("ba_iters", ctypes.c_int32),
        ("ba_pad", ctypes.c_int32), ("ba_lambda", ctypes.c_double), ("ba_outlier_px", ctypes.c_double),
        ("rgbd", ctypes.c_int32), ("ransac_mode", ctypes.c_int32),
        ("refine_block", ctypes.c_int32), ("match_refine", ctypes.c_int32),
    ]


class CameraDesc(ctypes.Structure):
    """tslam_camera_desc: one raw camera (camera_info K/D + world extrinsics, isaac_ros.py:364-411)."""
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("K", ctypes.c_double * 9), ("D", ctypes.c_double * 14),
        ("n_coeffs", ctypes.c_int32), ("cam_idx", ctypes.c_int32), ("world_T_cam", ctypes.c_double * 16),
        ("source", ctypes.c_char_p),
    ]


class ImuState(ctypes.Structure):
    """tslam_imu_state: the IMU filter's state (orientation, velocity, biases, variances)."""
    _fields_ = [
        ("R", ctypes.c_double * 9), ("v", ctypes.c_double * 3), ("ba", ctypes.c_double * 3), ("var_v", ctypes.c_double),
        ("var_b", ctypes.c_double), ("bg", ctypes.c_double * 3), ("var_g", ctypes.c_double),
        ("w_prev", ctypes.c_double * 3), ("has_w_prev", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class ImuStep(ctypes.Structure):
    """tslam_imu_step: one frame interval's IMU prediction."""
    _fields_ = [
        ("dt", ctypes.c_double), ("gyro", ctypes.c_double * 3), ("w", ctypes.c_double * 3), ("R_rel", ctypes.c_double * 9),
        ("t_rel", ctypes.c_double * 3), ("w_rot", ctypes.c_double), ("w_trans", ctypes.c_double),
        ("v1", ctypes.c_double * 3), ("var_v1", ctypes.c_double), ("has_v1", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class StereoDepthSgmParams(ctypes.Structure):
    """tslam_stereo_depth_sgm_params: semi-global aggregation of the dense stereo matcher."""
    _fields_ = [
        ("enable", ctypes.c_int32), ("p1", ctypes.c_int32), ("p2", ctypes.c_int32), ("paths", ctypes.c_int32),
        ("chunk_frames", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3),
    ]


class StereoDepthFilterParams(ctypes.Structure):
    """tslam_stereo_depth_filter_params: median and speckle filters of the dense stereo matcher."""
    _fields_ = [
        ("enable", ctypes.c_int32), ("median", ctypes.c_int32), ("speckle_size", ctypes.c_int32),
        ("speckle_range", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4),
    ]


class TsdfRigCamera(ctypes.Structure):
    """tslam_tsdf_rig_camera: one camera of ``Handle.tsdf_integrate_rig``."""
    _fields_ = [
        ("pair", ctypes.c_int32), ("rect", ctypes.c_int32), ("depth", ctypes.c_void_p), ("color", ctypes.c_void_p),
        ("stride_bytes", ctypes.c_int64),
    ]


class TsdfFollowParams(ctypes.Structure):
    """tslam_tsdf_follow_params: the rolling window's rule (thor_slam_amd/dense_follow.py)."""
    _fields_ = [("anchor", ctypes.c_int32 * 3), ("margin", ctypes.c_int32), ("step", ctypes.c_int32)]


class TsdfRenderParams(ctypes.Structure):
    """tslam_tsdf_render_params: the camera and the marching rule of ``Handle.tsdf_render``
    (thor_slam_amd/dense_render.py)."""
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fx", ctypes.c_double), ("fy", ctypes.c_double),
        ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("min_weight", ctypes.c_double), ("min_depth", ctypes.c_double),
        ("max_depth", ctypes.c_double), ("step_scale", ctypes.c_double), ("outputs", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class DepthRegisterParams(ctypes.Structure):
    """tslam_depth_register_params: the rule of ``Handle.depth_register`` (thor_slam_amd/depth_register.py)."""
    _fields_ = [
        ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("color_width", ctypes.c_int32),
        ("color_height", ctypes.c_int32), ("f_c", ctypes.c_double), ("cxc", ctypes.c_double), ("cyc", ctypes.c_double),
        ("map", ctypes.c_void_p), ("color_T_rect", ctypes.c_double * 12), ("max_depth_mm", ctypes.c_int32),
        ("tol_mm", ctypes.c_int32), ("max_splat", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class TsdfRigColor(ctypes.Structure):
    """tslam_tsdf_rig_color: one camera's colour and mask of ``Handle.tsdf_integrate_rig_color``."""
    _fields_ = [
        ("color", ctypes.c_void_p), ("color_stride", ctypes.c_int64), ("mask", ctypes.c_void_p),
        ("mask_stride", ctypes.c_int64),
    ]


class TsdfAlignParams(ctypes.Structure):
    """tslam_tsdf_align_params: the rule of ``Handle.tsdf_align`` (thor_slam_amd/dense_align.py)."""
    _fields_ = [
        ("iterations", ctypes.c_int32), ("min_inliers", ctypes.c_int32), ("max_distance", ctypes.c_double),
        ("min_weight", ctypes.c_double), ("max_depth", ctypes.c_double), ("step_scale", ctypes.c_double),
        ("max_translation", ctypes.c_double), ("max_rotation", ctypes.c_double), ("eps_translation", ctypes.c_double),
        ("eps_rotation", ctypes.c_double), ("min_pivot", ctypes.c_double), ("reserved", ctypes.c_int32 * 4),
    ]


class TsdfDynamicParams(ctypes.Structure):
    """tslam_tsdf_dynamic_params: the rule of ``Handle.tsdf_dynamic`` (thor_slam_amd/dense_dynamic.py)."""
    _fields_ = [
        ("min_free_weight", ctypes.c_double), ("free_fraction", ctypes.c_double), ("open_radius", ctypes.c_int32),
        ("dilate_radius", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4),
    ]


class TsdfFreespaceParams(ctypes.Structure):
    """tslam_tsdf_freespace_params: the free-space layer's rule (thor_slam_amd/dense_freespace.py)."""
    _fields_ = [("occupied_band_vox", ctypes.c_double), ("settle_frames", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


def camera_desc(cam) -> CameraDesc:
    """A ``CameraConfig`` (intrinsics + world extrinsics) as a ``tslam_camera_desc``."""
    d = CameraDesc()
    intr = cam.intrinsics
    d.width, d.height = int(intr.width), int(intr.height)
    d.K[:] = [float(v) for v in np.asarray(intr.matrix, dtype=np.float64).reshape(9)]
    coeffs = np.asarray(intr.coeffs, dtype=np.float64).flatten()[:14]
    d.D[:len(coeffs)] = [float(v) for v in coeffs]
    d.n_coeffs = len(coeffs)
    d.cam_idx = int(cam.cam_idx)
    d.world_T_cam[:] = [float(v) for v in cam.extrinsics.to_4x4_matrix().reshape(16)]
    d.source = str(cam.source_name).encode()
    return d


_lib: ctypes.CDLL | None = None

# name -> (restype, argtypes); every symbol include/tslam.h declares
_P = ctypes.c_void_p
_SIGNATURES = {
    "tslam_imu_create": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "tslam_imu_destroy": (None, [_P]),
    "tslam_imu_reset": (ctypes.c_int, [_P]),
    "tslam_imu_begin": (ctypes.c_int, [_P, _P]),
    "tslam_imu_ready": (ctypes.c_int, [_P]),
    "tslam_imu_get_state": (ctypes.c_int, [_P, _P]),
    "tslam_imu_set_state": (ctypes.c_int, [_P, _P]),
    "tslam_imu_predict": (ctypes.c_int, [_P, _P, ctypes.c_double, _P, _P, _P]),
    "tslam_imu_coast": (ctypes.c_int, [_P, _P, _P, _P]),
    "tslam_imu_correct": (ctypes.c_int, [_P, _P, _P, _P, _P, _P]),
    "tslam_imu_batch_priors": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, _P, _P]),
    "tslam_imu_absorb": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, _P, _P, _P]),
    "tslam_imu_vision_only": (ctypes.c_int, [_P, _P, ctypes.c_double, _P, _P, _P]),
    "tslam_imu_gravity": (ctypes.c_int, [_P, _P]),
    "tslam_imu_preintegrate": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_double,
                                              ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _P]),
    "tslam_last_error": (ctypes.c_char_p, []),
    "tslam_abi_version": (ctypes.c_int, []),
    "tslam_create": (ctypes.c_int, [ctypes.POINTER(StereoDesc), ctypes.POINTER(Params), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "tslam_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "tslam_comm_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "tslam_comm_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "tslam_submit_sharded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tslam_shard_options": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_perturb_temporal": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]),
    "tslam_shard_timing": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "tslam_create_rig": (ctypes.c_int, [ctypes.POINTER(CameraDesc), ctypes.c_int, ctypes.POINTER(Params), ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_void_p)]),
    "tslam_rig_pairs": (ctypes.c_int, [ctypes.POINTER(CameraDesc), ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "tslam_rectify_pair": (ctypes.c_int, [ctypes.POINTER(CameraDesc), ctypes.POINTER(CameraDesc), ctypes.POINTER(StereoDesc),
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_rgbd_undistort": (ctypes.c_int, [ctypes.POINTER(CameraDesc), ctypes.POINTER(StereoDesc), ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "tslam_submit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tslam_begin_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "tslam_run_stage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tslam_end_batch": (ctypes.c_int, [ctypes.c_void_p]),
    "tslam_detect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_describe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_match": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_pose": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "tslam_read_poses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4),
    "tslam_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "tslam_frames_done": (ctypes.c_int64, [ctypes.c_void_p]),
    "tslam_buffer_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                         ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "tslam_copy_out": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]),
    "tslam_copy_in": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]),
    "tslam_ring_slot": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "tslam_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_set_rig": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_set_motion_prior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "tslam_read_rig_poses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4),
    "tslam_host_stage": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]),
    "tslam_submit_host": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "tslam_poll_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 9
                         + [ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]),
    "tslam_poll_pose": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_void_p] * 5),
    "tslam_set_shard": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "tslam_exchange_sizes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "tslam_pack_streams": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_unpack_streams": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_import_raw": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p]),
    "tslam_stage_raw_peers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_pack_streams_peers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_import_peers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_pair_block_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]),
    "tslam_pack_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_unpack_pairs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_group_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "tslam_group_submit": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tslam_group_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "tslam_pack_poses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_unpack_poses": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_ba_read_map": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_map_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "tslam_relocalize": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64] + [ctypes.c_void_p] * 3),
    "tslam_relocalize_rig": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "tslam_reloc_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_int)]),
    "tslam_ba_read":(ctypes.c_int, [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 6),
    "tslam_ba_replay_schur": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "tslam_ba_split_solve": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_ba_defer": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_select_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "tslam_match_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "tslam_match_layout": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_describe_mode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_match_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)]),
    "tslam_detect_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_int]),
    "tslam_ba_inertial": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                         ctypes.c_void_p, ctypes.c_double]),
    "tslam_ba_inertial_factor": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "tslam_ba_read_inertial": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_ba_profile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
    "tslam_loop_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]),
    "tslam_loop_add_keyframe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "tslam_loop_read_keyframe": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.POINTER(ctypes.c_int)]),
    "tslam_loop_query": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "tslam_loop_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 3),
    "tslam_tsdf_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_double, ctypes.c_double]),
    "tslam_tsdf_integrate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_write": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_ba_imu_factor": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double]),
    "tslam_tsdf_color": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_tsdf_integrate_rgbd": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "tslam_tsdf_read_color": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_write_color": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_mesh_read_colors": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "tslam_mesh_extract": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "tslam_mesh_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "tslam_mesh_extract_whole": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64),
                                                ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]),
    "tslam_esdf_compute": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    "tslam_esdf_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_esdf_slice": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_void_p]),
    "tslam_pose_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]),
    "tslam_test_potrf_delay": (ctypes.c_int, [ctypes.c_int]),
    "tslam_ba_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_loop_auto": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "tslam_loop_job_vote": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_int64)]),
    "tslam_loop_job_verify": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int64)]),
    "tslam_loop_job_pose_graph": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_int64)]),
    "tslam_loop_job_poll": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_double)]),
    "tslam_stereo_depth_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "tslam_stereo_depth": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]),
    "tslam_stereo_depth_images": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                 ctypes.c_void_p]),
    "tslam_stereo_depth_buffers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                  ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)]),
    "tslam_stereo_depth_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_stereo_depth_sgm": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_stereo_depth_filter": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_stereo_depth_filter_apply": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                       ctypes.c_double, ctypes.c_int, ctypes.c_void_p]),
    "tslam_tsdf_integrate_rect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                 ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_integrate_rig": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                                ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_stereo_depth_slots": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                                ctypes.c_void_p]),
    "tslam_tsdf_follow": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_shift": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_window": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_render_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]),
    "tslam_tsdf_render": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                                         ctypes.c_void_p]),
    "tslam_tsdf_render_buffers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p]),
    "tslam_tsdf_render_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_align_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "tslam_tsdf_align": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_align_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_align_buffers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                ctypes.POINTER(ctypes.c_void_p)]),
    "tslam_tsdf_integrate_aligned": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                                    ctypes.c_int, ctypes.c_void_p]),
    "tslam_tsdf_dynamic_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "tslam_tsdf_dynamic": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_dynamic_buffers": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p),
                                                  ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                  ctypes.c_void_p]),
    "tslam_tsdf_dynamic_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p]),
    "tslam_tsdf_freespace_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_freespace_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_freespace_write": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_depth_register_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]),
    "tslam_depth_register": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                            ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "tslam_depth_register_blank": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "tslam_depth_register_buffers": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                    ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                                    ctypes.c_void_p]),
    "tslam_depth_register_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "tslam_depth_register_profile": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tslam_tsdf_integrate_rect_color": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64,
                                                       ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_integrate_rig_color": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                      ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_archive_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "tslam_tsdf_archive_integrate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                    ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_archive_move": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_double, ctypes.c_double, ctypes.c_void_p]),
    "tslam_tsdf_archive_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_int64)]),
    "tslam_tsdf_archive_read_depth": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "tslam_tsdf_store_init": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64]),
    "tslam_tsdf_store_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "tslam_tsdf_store_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
}


def load_library(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """Load (once) and type the HIP library.  Raises ``RuntimeError`` when it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is None and os.environ.get("TSLAM_LIBRARY"):
        path = os.environ["TSLAM_LIBRARY"]  # e.g. an experiment build; still cached as the one library
        p = Path(path)
        lib_is_default = True
    else:
        p = Path(path) if path is not None else LIB_PATH
        lib_is_default = path is None
    # torch ships its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Whichever loads first
    # is the one HIP runtime of the process; load torch's first so tensors and our kernels share
    # it (loading ours first leaves torch's HSA runtime unable to see the device).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not p.exists():
        raise RuntimeError(
            f"{p} is missing: the MI355X hot path has no CPU fallback. "
            "Build it with `make -C thor-slam_amd/csrc` (or __graft_entry__.build())."
        )
    lib = ctypes.CDLL(str(p))
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib_is_default:
        _lib = lib
    return lib


def exported_symbols() -> list[str]:
    return list(_SIGNATURES)


TSLAM_ESINGULAR = -5


class SingularSystemError(RuntimeError):
    """A pose-graph solve whose normal matrix was not positive definite (TSLAM_ESINGULAR)."""


def _check(rc: int) -> None:
    if rc != 0:
        msg = load_library().tslam_last_error()
        text = f"tslam error {rc}: {msg.decode() if msg else ''}"
        raise SingularSystemError(text) if rc == TSLAM_ESINGULAR else RuntimeError(text)


RANSAC_MODE = {"auto": 0, "exhaustive": 1, "bounded": 2}   # tslam_params.ransac_mode
MATCH_REFINE = {"auto": 0, "split": 1}   # tslam_params.match_refine
SELECT_MODE = {"auto": 0, "generic": 1, "resident": 2}   # tslam_select_mode
MATCH_MODE = {"auto": 0, "direct": 1, "merged": 2}   # tslam_match_mode
MATCH_LAYOUT = {"fused": 0, "split": 1}              # tslam_match_layout


def make_params(cfg: HipSlamConfig, max_batch: int, n_pairs: int, ransac_splits: int = 0,
                ransac_mode: str = "auto", refine_block: int = 0, match_refine: str = "auto") -> Params:
    return Params(
        cfg.n_features, cfg.n_levels, cfg.fast_threshold, cfg.edge_margin, cfg.max_hamming, cfg.ratio_pct,
        cfg.stereo_row_tol, cfg.max_disparity, cfg.temporal_window, cfg.ransac_hypotheses, cfg.refine_iters,
        cfg.min_inliers, float(cfg.ransac_thr_px), int(cfg.ransac_seed) & ((1 << 64) - 1), int(max_batch), int(n_pairs),
        int(ransac_splits), int(cfg.ba_window), int(cfg.ba_kf_interval), int(cfg.ba_iters), 0, float(cfg.ba_lambda),
        float(cfg.ba_outlier_px), int(bool(cfg.rgbd)), RANSAC_MODE[ransac_mode], int(refine_block),
        MATCH_REFINE[match_refine],
    )


def native_rectify_pair(left, right=None, rgbd: bool = False) -> dict:
    """``tslam_rectify_pair`` (``tslam_rgbd_undistort`` with ``rgbd``) on two ``CameraConfig``:
    the library's C++ restatement of ``calib.stereo_rectify`` / ``calib.rgbd_undistort``."""
    lib = load_library()
    dl = camera_desc(left)
    h, w = int(dl.height), int(dl.width)
    desc = StereoDesc()
    ml = np.zeros((h, w, 2), np.int32)
    mr = np.zeros((h, w, 2), np.int32)
    base = np.zeros((4, 4))
    rot = np.zeros((2, 3, 3))
    if rgbd:
        _check(lib.tslam_rgbd_undistort(ctypes.byref(dl), ctypes.byref(desc), ml.ctypes.data, base.ctypes.data))
        mr[...] = ml
        rot[:] = np.eye(3)
    else:
        dr = camera_desc(right)
        _check(lib.tslam_rectify_pair(ctypes.byref(dl), ctypes.byref(dr), ctypes.byref(desc), ml.ctypes.data,
                                      mr.ctypes.data, base.ctypes.data, rot.ctypes.data))
    return {"width": desc.width, "height": desc.height, "fx": desc.fx, "fy": desc.fy, "cx": desc.cx, "cy": desc.cy,
            "baseline": desc.baseline, "map_left": ml, "map_right": mr, "base_T_rect": base,
            "rect_left": rot[0], "rect_right": rot[1]}


def comm_unique_id() -> bytes:
    """``tslam_comm_unique_id``: a fresh RCCL unique id (128 bytes) for ``Handle.comm_init``."""
    buf = (ctypes.c_uint8 * 128)()
    _check(load_library().tslam_comm_unique_id(buf))
    return bytes(buf)


class Handle:
    """Owns one ``tslam_handle`` (one device, ``n_pairs`` stereo pairs, batches <= ``max_batch``)."""

    def __init__(self, rects: list, cfg: HipSlamConfig, max_batch: int = 1, device: int = 0, ransac_splits: int = 0,
                 ransac_mode: str = "auto", refine_block: int = 0, match_refine: str = "auto"):
        self.lib = load_library()
        cfg.validate()
        self.cfg = cfg
        self.n_pairs = len(rects)
        self.cams_per_pair = 1 if cfg.rgbd else 2   # RGB-D: one colour camera (+ aligned depth) per "pair"
        self.n_cams = self.cams_per_pair * self.n_pairs
        self.max_batch = int(max_batch)
        self._maps = []  # keep host maps alive during create
        descs = (StereoDesc * self.n_pairs)()
        for i, r in enumerate(rects):
            ml = None if r.is_identity else np.ascontiguousarray(r.map_left, dtype=np.int32)
            mr = None if r.is_identity else np.ascontiguousarray(r.map_right, dtype=np.int32)
            self._maps += [ml, mr]
            descs[i] = StereoDesc(
                r.width, r.height, r.fx, r.fy, r.cx, r.cy, r.baseline,
                None if ml is None else ml.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                None if mr is None else mr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            )
        params = make_params(cfg, max_batch, self.n_pairs, ransac_splits, ransac_mode, refine_block, match_refine)
        h = ctypes.c_void_p()
        _check(self.lib.tslam_create(descs, ctypes.byref(params), int(device), ctypes.byref(h)))
        self.h = h
        self._maps = []
        self._read_layout()

    @classmethod
    def from_cameras(cls, cams: list, cfg: HipSlamConfig, max_batch: int = 1, device: int = 0,
                     ransac_splits: int = 0) -> "Handle":
        """``tslam_create_rig``: the handle from raw per-camera calibration (``CameraConfig`` list),
        rectified and paired by the library's C++ host code; multi-pair rigs get ``tslam_set_rig``."""
        self = cls.__new__(cls)
        self.lib = load_library()
        cfg.validate()
        self.cfg = cfg
        descs = (CameraDesc * len(cams))(*[camera_desc(c) for c in cams])
        n_pairs = self.lib.tslam_rig_pairs(descs, len(cams), None, 0)
        _check(min(n_pairs, 0))
        self.n_pairs = n_pairs
        self.cams_per_pair = 1 if cfg.rgbd else 2
        self.n_cams = self.cams_per_pair * n_pairs
        self.max_batch = int(max_batch)
        params = make_params(cfg, max_batch, 0, ransac_splits)
        h = ctypes.c_void_p()
        _check(self.lib.tslam_create_rig(descs, len(cams), ctypes.byref(params), int(device), ctypes.byref(h)))
        self.h = h
        self._read_layout()
        return self

    def _read_layout(self) -> None:
        lay = (ctypes.c_int64 * 16)()
        lev = (ctypes.c_int32 * 18)()
        _check(self.lib.tslam_layout(self.h, lay, lev))
        self.width, self.height = int(lay[0]), int(lay[1])
        self.n_levels, self.K, self.ring, self.batch = int(lay[2]), int(lay[3]), int(lay[4]), int(lay[5])
        self.pyr_bytes = int(lay[7])
        self.pyr_off = [int(lay[8 + l]) for l in range(self.n_levels)]
        self.level_wh = [(int(lev[3 * l]), int(lev[3 * l + 1])) for l in range(self.n_levels)]
        self.quotas = [int(lev[3 * l + 2]) for l in range(self.n_levels)]
        self.koff = [sum(self.quotas[:l]) for l in range(self.n_levels)]

    # -- lifecycle -------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.tslam_destroy(self.h)
            self.h = None

    def __del__(self):  # noqa: D105
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        _check(self.lib.tslam_reset(self.h))

    @property
    def frames_done(self) -> int:
        return int(self.lib.tslam_frames_done(self.h))

    # -- execution -------------------------------------------------------------------------
    def submit(self, images_dev_ptr: int, n_frames: int, stream: int = 0) -> None:
        _check(self.lib.tslam_submit(self.h, ctypes.c_void_p(images_dev_ptr), int(n_frames), ctypes.c_void_p(stream)))

    def begin_batch(self, images_dev_ptr: int, n_frames: int) -> None:
        _check(self.lib.tslam_begin_batch(self.h, ctypes.c_void_p(images_dev_ptr), int(n_frames)))

    def run_stage(self, stage: str, stream: int = 0) -> None:
        _check(self.lib.tslam_run_stage(self.h, STAGE[stage], ctypes.c_void_p(stream)))

    def run_kernel(self, name: str, stream: int = 0) -> None:
        _check(self.lib.tslam_run_stage(self.h, KERNELS[name], ctypes.c_void_p(stream)))

    def run_pose_solve(self, stream: int = 0) -> None:
        """``TSLAM_KERNEL_POSE_SOLVE`` (parity tests): P3P + RANSAC + refinement on the
        correspondences and counts already in the ``corr`` / ``stats`` buffers."""
        _check(self.lib.tslam_run_stage(self.h, POSE_SOLVE_KERNEL, ctypes.c_void_p(stream)))

    def perturb_temporal(self, percent: int, seed: int = 11, stream: int = 0) -> None:
        """``tslam_perturb_temporal`` (benchmark hook): outliers into the batch's refined temporal
        positions, between the match_refine and pose kernels."""
        _check(self.lib.tslam_perturb_temporal(self.h, int(percent), int(seed) & ((1 << 64) - 1), ctypes.c_void_p(stream)))

    def run_rig(self, stream: int = 0) -> None:
        _check(self.lib.tslam_run_stage(self.h, RIG_KERNEL, ctypes.c_void_p(stream)))

    def end_batch(self) -> None:
        _check(self.lib.tslam_end_batch(self.h))

    def sync(self) -> None:
        _check(self.lib.tslam_sync(self.h))

    def read_poses(self, n_frames: int) -> dict:
        n = n_frames * self.n_pairs
        t_rel = np.zeros((n, 4, 4))
        t_abs = np.zeros((n, 4, 4))
        cov = np.zeros((n, 6, 6))
        stats = np.zeros((n, 8), dtype=np.int32)
        _check(self.lib.tslam_read_poses(self.h, int(n_frames), t_rel.ctypes.data, t_abs.ctypes.data, cov.ctypes.data,
                                         stats.ctypes.data))
        shape = (n_frames, self.n_pairs)
        return {
            "T_rel": t_rel.reshape(shape + (4, 4)), "T_abs": t_abs.reshape(shape + (4, 4)),
            "cov": cov.reshape(shape + (6, 6)), "stats": stats.reshape(shape + (8,)),
        }

    def set_motion_prior(self, rot: np.ndarray, weight: np.ndarray, trans: np.ndarray | None = None,
                         trans_weight: np.ndarray | None = None) -> None:
        """Motion prior for the next batch: rot [n][P][3][3] (predicted T_rel rotations), weight
        [n][P]; optionally trans [n][P][3] (predicted T_rel translations) and trans_weight [n][P]."""
        rot = np.asarray(rot, dtype=np.float64)
        n = rot.shape[0]
        buf = np.zeros((n, self.n_pairs, 16))
        buf[..., :9] = rot.reshape(n, self.n_pairs, 9)
        buf[..., 9] = np.asarray(weight, dtype=np.float64).reshape(n, self.n_pairs)
        if trans is not None:
            buf[..., 10:13] = np.asarray(trans, dtype=np.float64).reshape(n, self.n_pairs, 3)
            buf[..., 13] = np.asarray(trans_weight, dtype=np.float64).reshape(n, self.n_pairs)
        _check(self.lib.tslam_set_motion_prior(self.h, np.ascontiguousarray(buf).ctypes.data, int(n)))

    def set_rig(self, base_T_rect: list) -> None:
        """Enable the rig pose: base_T_rect-left (4x4) of every pair, in pair order."""
        e = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.float64) for m in base_T_rect]))
        if e.shape != (self.n_pairs, 4, 4):
            raise ValueError(f"need {self.n_pairs} 4x4 matrices")
        _check(self.lib.tslam_set_rig(self.h, e.ctypes.data))

    def read_rig_poses(self, n_frames: int) -> dict:
        """Body-frame rig motion of the last batch (synchronises)."""
        t_rel = np.zeros((n_frames, 4, 4))
        t_abs = np.zeros((n_frames, 4, 4))
        cov = np.zeros((n_frames, 6, 6))
        stats = np.zeros((n_frames, 8), dtype=np.int32)
        _check(self.lib.tslam_read_rig_poses(self.h, int(n_frames), t_rel.ctypes.data, t_abs.ctypes.data, cov.ctypes.data,
                                             stats.ctypes.data))
        return {"T_rel": t_rel, "T_abs": t_abs, "cov": cov, "stats": stats}

    # -- asynchronous host boundary ------------------------------------------------------------
    def submit_host(self, images: np.ndarray, timestamps=None) -> None:
        """Host frames [n][...] (contiguous u8: [n][2P][H][W] gray or [n][P][5HW] RGB-D) -> the
        device, asynchronously (tslam_submit_host)."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        n = int(images.shape[0])
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.float64)
        _check(self.lib.tslam_submit_host(self.h, images.ctypes.data, None if ts is None else ts.ctypes.data, n))

    def host_stage(self) -> np.ndarray:
        """The pinned staging buffer of the next submit_host as a [max_batch][frame_bytes] u8 view
        (tslam_host_stage: waits until its previous DMA finished); frames written there and passed
        back to submit_host skip the staging copy."""
        p, fb = ctypes.c_void_p(), ctypes.c_int64()
        _check(self.lib.tslam_host_stage(self.h, ctypes.byref(p), ctypes.byref(fb)))
        key = (p.value, fb.value)
        views = getattr(self, "_stage_views", None)
        if views is None:
            views = self._stage_views = {}
        if key not in views:
            buf = (ctypes.c_uint8 * (self.max_batch * fb.value)).from_address(p.value)
            views[key] = np.frombuffer(buf, dtype=np.uint8).reshape(self.max_batch, fb.value)
        return views[key]

    def _poll_buffers(self) -> tuple:
        """Result arrays of tslam_poll_batch, allocated once with their pointers (a non-blocking poll
        that finds nothing ready costs one C call, no allocation)."""
        if getattr(self, "_pb", None) is None:
            B, P = self.max_batch, self.n_pairs
            arrs = (np.zeros((B, P, 4, 4)), np.zeros((B, P, 4, 4)), np.zeros((B, P, 6, 6)),
                    np.zeros((B, P, 8), dtype=np.int32), np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), np.zeros((B, 6, 6)),
                    np.zeros((B, 8), dtype=np.int32), np.zeros(B))
            g0, n = ctypes.c_int64(), ctypes.c_int()
            self._pb = (arrs, tuple(ctypes.c_void_p(a.ctypes.data) for a in arrs), g0, n, ctypes.byref(g0),
                        ctypes.byref(n))
        return self._pb

    def poll_batch(self, block: bool = False) -> dict | None:
        """Results of the oldest unread submitted batch (copies), or None when none is ready."""
        arrs, ptrs, g0, n, g0_ref, n_ref = self._poll_buffers()
        rc = self.lib.tslam_poll_batch(self.h, int(block), self.max_batch, *ptrs, g0_ref, n_ref)
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        k = n.value
        t_rel, t_abs, cov, stats, r_rel, r_abs, r_cov, r_st, ts = (a[:k].copy() for a in arrs)
        out = {"T_rel": t_rel, "T_abs": t_abs, "cov": cov, "stats": stats, "timestamps": ts,
               "first_frame": int(g0.value), "n": k}
        out["rig"] = {"T_rel": r_rel, "T_abs": r_abs, "cov": r_cov, "stats": r_st}
        return out

    def poll_pose(self) -> dict | None:
        """Newest completed pose not returned before (non-blocking), or None."""
        T, cov = np.zeros((4, 4)), np.zeros((6, 6))
        ts, st, conf = ctypes.c_double(), ctypes.c_int32(), ctypes.c_float()
        rc = self.lib.tslam_poll_pose(self.h, T.ctypes.data, cov.ctypes.data, ctypes.addressof(ts), ctypes.addressof(st),
                                      ctypes.addressof(conf))
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        return {"T": T, "cov": cov, "timestamp": ts.value, "state": st.value, "confidence": conf.value}

    # -- sharded rig (thor_slam_amd/shard.py drives these) --------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """``tslam_comm_init``: join an RCCL communicator and own this rank's shard of the rig."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(self.lib.tslam_comm_init(self.h, buf, int(rank), int(world)))

    def submit_sharded(self, images_dev_ptr: int, n_frames: int | None = None, stream: int = 0) -> None:
        """``tslam_submit_sharded``: one batch (default max_batch frames) of this rank's cameras,
        exchanges over RCCL."""
        n = self.max_batch if n_frames is None else int(n_frames)
        _check(self.lib.tslam_submit_sharded(self.h, ctypes.c_void_p(images_dev_ptr), n, ctypes.c_void_p(stream)))

    def shard_options(self, gather: bool = False, results: bool = False, profile: bool = False,
                      serial: bool = False, pipeline: bool = False, solo: bool = False, pairs: bool = False) -> None:
        """``tslam_shard_options`` of the driver behind this (sharded) handle (``pairs``:
        TSLAM_SHARD_PAIRS, the pair split of a one-camera-per-rank stereo rig)."""
        flags = ((SHARD_GATHER if gather else 0) | (SHARD_RESULTS if results else 0) | (SHARD_PROFILE if profile else 0)
                 | (SHARD_SERIAL if serial else 0) | (SHARD_PIPELINE if pipeline else 0) | (SHARD_SOLO if solo else 0)
                 | (SHARD_PAIRS if pairs else 0))
        _check(self.lib.tslam_shard_options(self.h, flags))

    def shard_timing(self) -> tuple[dict, int]:
        """``tslam_shard_timing``: average µs per batch of every segment of this rank (since the
        last call; synchronises) and the number of batches."""
        out = (ctypes.c_double * len(SHARD_SEGMENTS))()
        nb = self.lib.tslam_shard_timing(self.h, out, len(SHARD_SEGMENTS))
        _check(min(nb, 0))
        return {k: float(v) for k, v in zip(SHARD_SEGMENTS, out)}, int(nb)

    def set_shard(self, cam_lo: int, cam_hi: int, rank: int, world: int) -> None:
        _check(self.lib.tslam_set_shard(self.h, int(cam_lo), int(cam_hi), int(rank), int(world)))

    def exchange_sizes(self) -> tuple[int, int]:
        """(bytes of one stream block, bytes of one pose record)."""
        sb, pr = ctypes.c_int64(), ctypes.c_int64()
        _check(self.lib.tslam_exchange_sizes(self.h, ctypes.byref(sb), ctypes.byref(pr)))
        return int(sb.value), int(pr.value)

    def pack_streams(self, first_frame: int, n_frames: int, cam_lo: int, cam_hi: int, dst_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_pack_streams(self.h, int(first_frame), int(n_frames), int(cam_lo), int(cam_hi),
                                           ctypes.c_void_p(dst_ptr), ctypes.c_void_p(stream)))

    def unpack_streams(self, first_frame: int, n_frames: int, cam_lo: int, cam_hi: int, src_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_unpack_streams(self.h, int(first_frame), int(n_frames), int(cam_lo), int(cam_hi),
                                             ctypes.c_void_p(src_ptr), ctypes.c_void_p(stream)))

    def import_raw(self, images_ptr: int, first_frame: int, n_frames: int, cam_lo: int, cam_hi: int, stream: int = 0) -> None:
        _check(self.lib.tslam_import_raw(self.h, ctypes.c_void_p(images_ptr), int(first_frame), int(n_frames), int(cam_lo),
                                         int(cam_hi), ctypes.c_void_p(stream)))

    def stage_raw_peers(self, prev_raw_ptr: int, dst_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_stage_raw_peers(self.h, ctypes.c_void_p(prev_raw_ptr), ctypes.c_void_p(dst_ptr),
                                              ctypes.c_void_p(stream)))

    def pack_streams_peers(self, dst_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_pack_streams_peers(self.h, ctypes.c_void_p(dst_ptr), ctypes.c_void_p(stream)))

    def import_peers(self, raw_ptr: int, streams_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_import_peers(self.h, ctypes.c_void_p(raw_ptr), ctypes.c_void_p(streams_ptr),
                                           ctypes.c_void_p(stream)))

    def pair_block_bytes(self) -> int:
        """Bytes of one RGB-D pair block (pose, stats, correspondences of one frame and camera)."""
        n = ctypes.c_int64()
        _check(self.lib.tslam_pair_block_bytes(self.h, ctypes.byref(n)))
        return int(n.value)

    def pack_pairs(self, f0: int, n_frames: int, pair_lo: int, pair_hi: int, dst_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_pack_pairs(self.h, int(f0), int(n_frames), int(pair_lo), int(pair_hi),
                                         ctypes.c_void_p(dst_ptr), ctypes.c_void_p(stream)))

    def unpack_pairs(self, f0: int, n_frames: int, pair_lo: int, pair_hi: int, src_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_unpack_pairs(self.h, int(f0), int(n_frames), int(pair_lo), int(pair_hi),
                                           ctypes.c_void_p(src_ptr), ctypes.c_void_p(stream)))

    def pack_poses(self, dst_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_pack_poses(self.h, ctypes.c_void_p(dst_ptr), ctypes.c_void_p(stream)))

    def unpack_poses(self, src_ptr: int, stream: int = 0) -> None:
        _check(self.lib.tslam_unpack_poses(self.h, ctypes.c_void_p(src_ptr), ctypes.c_void_p(stream)))

    # -- buffer access (tests) -------------------------------------------------------------
    def buffer_info(self, which: str) -> tuple[int, int, int]:
        ptr = ctypes.c_void_p()
        tot = ctypes.c_int64()
        per = ctypes.c_int64()
        _check(self.lib.tslam_buffer_info(self.h, BUF[which], ctypes.byref(ptr), ctypes.byref(tot), ctypes.byref(per)))
        return int(ptr.value or 0), int(tot.value), int(per.value)

    def copy_out(self, which: str, offset: int, nbytes: int, dtype) -> np.ndarray:
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(self.lib.tslam_copy_out(self.h, BUF[which], int(offset), out.ctypes.data, int(nbytes)))
        return out

    def copy_in(self, which: str, offset: int, data: np.ndarray) -> None:
        data = np.ascontiguousarray(data)
        _check(self.lib.tslam_copy_in(self.h, BUF[which], int(offset), data.ctypes.data, int(data.nbytes)))

    def ring_slot(self, global_frame: int) -> int:
        return int(self.lib.tslam_ring_slot(self.h, int(global_frame)))

    def frame_block(self, which: str, slot: int, dtype) -> np.ndarray:
        """All bytes of one frame slot of a buffer (ring slot or batch slot, per the layout)."""
        _, _, per = self.buffer_info(which)
        return self.copy_out(which, slot * per, per, dtype)

    def ba_read(self, pair: int = 0) -> dict:
        """A8 keyframe window of one pair (synchronises): slot-indexed frames, cam_T_world,
        landmark ids, landmark positions (by id), observations and the last solve's counts.
        On a rig (``set_rig``, several pairs) ``pair = n_pairs`` reads the body window of the
        rig-level solve: ``T_cw`` is body_T_world per slot, counts are the joint ones."""
        W, K = self.cfg.ba_window, self.K
        frames = np.zeros(W, dtype=np.int64)
        T = np.zeros((W, 4, 4))
        lm = np.zeros((W, K), dtype=np.int32)
        X = np.zeros((W * K, 3))
        uvd = np.zeros((3, W, K))
        cnt = np.zeros(4, dtype=np.int32)
        _check(self.lib.tslam_ba_read(self.h, int(pair), *(a.ctypes.data for a in (frames, T, lm, X, uvd, cnt))))
        return {"frames": frames, "T_cw": T, "lm": lm.astype(np.int64), "X": X, "u": uvd[0], "v": uvd[1],
                "d": uvd[2], "n_obs": int(cnt[0]), "n_lm": int(cnt[1]), "ok": bool(cnt[2])}

    def ba_read_map(self, pair: int = 0) -> dict:
        """Global landmark ids and keyframe-keypoint descriptors of the window (by landmark id)."""
        WK = self.cfg.ba_window * self.K
        gid = np.zeros(WK, dtype=np.int64)
        desc = np.zeros((WK, 8), dtype=np.uint32)
        _check(self.lib.tslam_ba_read_map(self.h, int(pair), gid.ctypes.data, desc.ctypes.data))
        return {"gid": gid, "desc": desc}

    def map_upload(self, xyz: np.ndarray, desc: np.ndarray) -> None:
        """Upload a relocalisation map: world points [n][3] f64 and rBRIEF descriptors [n][8] u32."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        desc = np.ascontiguousarray(desc, dtype=np.uint32).reshape(-1, 8)
        if xyz.shape[0] != desc.shape[0]:
            raise ValueError("xyz and desc must have the same number of points")
        _check(self.lib.tslam_map_upload(self.h, xyz.ctypes.data, desc.ctypes.data, int(xyz.shape[0])))

    def relocalize(self, frame: int, pair: int = 0) -> dict:
        """cam_T_world of a resident frame's left camera in the uploaded map (synchronises)."""
        T = np.zeros((4, 4))
        cov = np.zeros((6, 6))
        st = np.zeros(8, dtype=np.int32)
        _check(self.lib.tslam_relocalize(self.h, int(pair), int(frame), T.ctypes.data, cov.ctypes.data, st.ctypes.data))
        return {"T": T, "cov": cov, "stats": st}

    def relocalize_rig(self, frame: int) -> dict:
        """body_T_world of a resident frame of the rig (``set_rig``) in the uploaded map (base-frame
        world points), from every pair's view (synchronises): T, cov, stats (the rig's), and
        pair_stats [P][8]."""
        T, cov = np.zeros((4, 4)), np.zeros((6, 6))
        st, pst = np.zeros(8, dtype=np.int32), np.zeros((self.n_pairs, 8), dtype=np.int32)
        _check(self.lib.tslam_relocalize_rig(self.h, int(frame), T.ctypes.data, cov.ctypes.data, st.ctypes.data,
                                             pst.ctypes.data))
        return {"T": T, "cov": cov, "stats": st, "pair_stats": pst}

    def reloc_read(self, pair: int = 0) -> dict:
        """What the last ``relocalize`` / ``loop_verify`` / ``relocalize_rig`` left for ``pair``
        (synchronises): match [K] i32 (map index or -1 per keypoint) and corr [n_corr][8] f64 (X Y Z du
        dv bx by bz, keypoint order)."""
        match = np.full(self.K, -1, dtype=np.int32)
        corr = np.zeros((self.K, 8))
        n = ctypes.c_int()
        _check(self.lib.tslam_reloc_read(self.h, int(pair), match.ctypes.data, corr.ctypes.data, ctypes.byref(n)))
        return {"match": match, "corr": corr[:n.value]}

    # -- loop closure + pose graph --------------------------------
    def loop_init(self, max_keyframes: int = 1024, signature: int = 256) -> None:
        _check(self.lib.tslam_loop_init(self.h, int(max_keyframes), int(signature)))

    def loop_add_keyframe(self, frame: int, pair: int = 0) -> tuple[int, int]:
        """Store a resident frame's stereo landmarks in the keyframe database -> (entry, landmarks)."""
        slot, n = ctypes.c_int(), ctypes.c_int()
        _check(self.lib.tslam_loop_add_keyframe(self.h, int(pair), int(frame), ctypes.byref(slot), ctypes.byref(n)))
        return int(slot.value), int(n.value)

    def loop_read_keyframe(self, slot: int) -> dict:
        n = ctypes.c_int()
        _check(self.lib.tslam_loop_read_keyframe(self.h, int(slot), None, None, ctypes.byref(n)))
        xyz = np.zeros((max(n.value, 1), 3))
        desc = np.zeros((max(n.value, 1), 8), dtype=np.uint32)
        _check(self.lib.tslam_loop_read_keyframe(self.h, int(slot), xyz.ctypes.data, desc.ctypes.data, ctypes.byref(n)))
        return {"xyz": xyz[:n.value], "desc": desc[:n.value]}

    def loop_query(self, slot: int, n_candidates: int) -> np.ndarray:
        """Place-recognition votes of entry ``slot`` against entries [0, n_candidates)."""
        votes = np.zeros(max(int(n_candidates), 1), dtype=np.int32)
        _check(self.lib.tslam_loop_query(self.h, int(slot), int(n_candidates), votes.ctypes.data))
        return votes[:int(n_candidates)]

    def loop_verify(self, frame: int, slot: int, pair: int = 0) -> dict:
        """cam_q_T_cam_c of a resident frame against a database entry (synchronises)."""
        T = np.zeros((4, 4))
        cov = np.zeros((6, 6))
        st = np.zeros(8, dtype=np.int32)
        _check(self.lib.tslam_loop_verify(self.h, int(pair), int(frame), int(slot), T.ctypes.data, cov.ctypes.data,
                                          st.ctypes.data))
        return {"T": T, "cov": cov, "stats": st}

    # -- asynchronous loop closure (tslam_loop_auto / tslam_loop_job_*) -----------------------
    def loop_auto(self, interval: int) -> None:
        """Keyframes (g % interval == 0) stored by the submit path itself; 0 turns it off."""
        _check(self.lib.tslam_loop_auto(self.h, int(interval)))

    def loop_job_vote(self, query: int, k0: int, n_kf: int) -> "LoopJob":
        job = ctypes.c_int64()
        _check(self.lib.tslam_loop_job_vote(self.h, int(query), int(k0), int(n_kf), ctypes.byref(job)))
        return LoopJob(self, job.value, "vote", n=int(n_kf) * self.n_pairs)

    def loop_job_verify(self, frame: int, query: int, cand: int, pair: int = 0) -> "LoopJob":
        job = ctypes.c_int64()
        _check(self.lib.tslam_loop_job_verify(self.h, int(pair), int(frame), int(query), int(cand), ctypes.byref(job)))
        return LoopJob(self, job.value, "verify")

    def loop_job_pose_graph(self, T: np.ndarray, edges: np.ndarray, meas: np.ndarray, info: np.ndarray,
                            iters: int) -> "LoopJob":
        T = np.ascontiguousarray(np.array(T, dtype=np.float64).reshape(-1, 4, 4))
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
        meas = np.ascontiguousarray(np.asarray(meas, dtype=np.float64).reshape(-1, 4, 4))
        info = np.ascontiguousarray(np.asarray(info, dtype=np.float64).reshape(-1, 6, 6))
        job = ctypes.c_int64()
        _check(self.lib.tslam_loop_job_pose_graph(self.h, int(T.shape[0]), T.ctypes.data, int(edges.shape[0]),
                                                  edges.ctypes.data, meas.ctypes.data, info.ctypes.data, int(iters),
                                                  ctypes.byref(job)))
        return LoopJob(self, job.value, "pose_graph", n=int(T.shape[0]))

    def pose_graph(self, T: np.ndarray, edges: np.ndarray, meas: np.ndarray, info: np.ndarray, iters: int) -> dict:
        """Gauss-Newton on a keyframe pose graph (node 0 fixed) on the device -> poses, cost."""
        T = np.ascontiguousarray(np.array(T, dtype=np.float64).reshape(-1, 4, 4))
        edges = np.ascontiguousarray(np.asarray(edges, dtype=np.int32).reshape(-1, 2))
        meas = np.ascontiguousarray(np.asarray(meas, dtype=np.float64).reshape(-1, 4, 4))
        info = np.ascontiguousarray(np.asarray(info, dtype=np.float64).reshape(-1, 6, 6))
        cost = ctypes.c_double()
        _check(self.lib.tslam_pose_graph(self.h, int(T.shape[0]), T.ctypes.data, int(edges.shape[0]), edges.ctypes.data,
                                         meas.ctypes.data, info.ctypes.data, int(iters), ctypes.byref(cost)))
        return {"T": T, "cost": cost.value}

    # -- RGB-D dense mapping ------------------------------------------
    def tsdf_init(self, origin, dims, voxel_size: float = 0.05, trunc_vox: float = 4.0, max_dist: float = 10.0,
                  max_weight: float = 100.0) -> None:
        o = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        d = np.ascontiguousarray(dims, dtype=np.int32).reshape(3)
        self._tsdf_dims = tuple(int(x) for x in d)
        self._tsdf_anchor = default_anchor(o, float(voxel_size))
        _check(self.lib.tslam_tsdf_init(self.h, o.ctypes.data, d.ctypes.data, float(voxel_size), float(trunc_vox),
                                        float(max_dist), float(max_weight)))

    def tsdf_color(self, enable: bool = True) -> None:
        """The colour layer (call before tsdf_init)."""
        _check(self.lib.tslam_tsdf_color(self.h, int(bool(enable))))
        self._tsdf_color = bool(enable)

    def tsdf_integrate_rgbd(self, color_dev_ptr: int, depth_dev_ptr: int, stride_bytes: int, n_frames: int,
                            first_frame: int = 0, world_T_cam: np.ndarray | None = None, pair: int = 0,
                            stream: int = 0) -> None:
        """Depth + BGR colour of n frames (device, both ``stride_bytes`` apart) into the volume and
        its colour layer, with host poses or the last batch's tracked device poses."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        _check(self.lib.tslam_tsdf_integrate_rgbd(self.h, int(pair), ctypes.c_void_p(color_dev_ptr),
                                                  ctypes.c_void_p(depth_dev_ptr), int(stride_bytes), int(n_frames),
                                                  int(first_frame), None if poses is None else poses.ctypes.data,
                                                  ctypes.c_void_p(stream)))

    def tsdf_read_color(self) -> tuple[np.ndarray, np.ndarray]:
        """(colour [nz][ny][nx][3] R, G, B f32, weight [nz][ny][nx] f32) of the colour layer."""
        nx, ny, nz = self._tsdf_dims
        c = np.zeros((nz, ny, nx, 3), dtype=np.float32)
        w = np.zeros((nz, ny, nx), dtype=np.float32)
        _check(self.lib.tslam_tsdf_read_color(self.h, c.ctypes.data, w.ctypes.data))
        return c, w

    def tsdf_write_color(self, color: np.ndarray, weight: np.ndarray) -> None:
        nx, ny, nz = self._tsdf_dims
        c = np.ascontiguousarray(color, dtype=np.float32)
        w = np.ascontiguousarray(weight, dtype=np.float32)
        if c.shape != (nz, ny, nx, 3) or w.shape != (nz, ny, nx):
            raise ValueError(f"colour layer must be {(nz, ny, nx, 3)} / {(nz, ny, nx)}")
        _check(self.lib.tslam_tsdf_write_color(self.h, c.ctypes.data, w.ctypes.data))

    def tsdf_integrate(self, depth_dev_ptr: int, stride_bytes: int, n_frames: int, first_frame: int = 0,
                       world_T_cam: np.ndarray | None = None, pair: int = 0, stream: int = 0) -> None:
        """Integrate n depth frames (device u16 mm, ``stride_bytes`` apart) with host poses
        world_T_cam [n][4][4], or the last batch's tracked device poses when None."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        _check(self.lib.tslam_tsdf_integrate(self.h, int(pair), ctypes.c_void_p(depth_dev_ptr), int(stride_bytes),
                                             int(n_frames), int(first_frame),
                                             None if poses is None else poses.ctypes.data, ctypes.c_void_p(stream)))

    def tsdf_integrate_rect(self, depth_dev_ptr: int, stride_bytes: int, n_frames: int, first_frame: int = 0,
                            world_T_cam: np.ndarray | None = None, pair: int = 0, stream: int = 0) -> None:
        """``tsdf_integrate`` for depth images of the pair's RECTIFIED left camera (``stereo_depth``'s
        output): no lookup through the raw camera's undistortion table."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        _check(self.lib.tslam_tsdf_integrate_rect(self.h, int(pair), ctypes.c_void_p(depth_dev_ptr), int(stride_bytes),
                                                  int(n_frames), int(first_frame),
                                                  None if poses is None else poses.ctypes.data, ctypes.c_void_p(stream)))

    def tsdf_archive_init(self, capacity: int, interval: int = 1, pair: int = 0, rect: bool = False) -> None:
        """The depth archive (thor_slam_amd/dense_loop.py): a ring of ``capacity`` depth frames of the
        pair's camera (``rect``: its rectified camera, as ``tsdf_integrate_rect``) that keeps every
        frame whose number is a multiple of ``interval``.  After ``tsdf_init``."""
        _check(self.lib.tslam_tsdf_archive_init(self.h, int(pair), int(bool(rect)), int(capacity), int(interval)))

    def tsdf_archive_integrate(self, depth_dev_ptr: int, stride_bytes: int, n_frames: int, first_frame: int = 0,
                               world_T_corr: np.ndarray | None = None, world_T_cam: np.ndarray | None = None,
                               stream: int = 0) -> None:
        """``tsdf_integrate`` of the frames ``first_frame + i`` that are multiples of the archive's
        interval, which are archived with the poses they went in with: host poses ``world_T_cam``
        [n][4][4], or the last batch's tracked device poses premultiplied by ``world_T_corr`` [4][4]."""
        poses = corr = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        if world_T_corr is not None:
            corr = np.ascontiguousarray(np.asarray(world_T_corr, dtype=np.float64).reshape(4, 4))
        _check(self.lib.tslam_tsdf_archive_integrate(self.h, ctypes.c_void_p(depth_dev_ptr), int(stride_bytes), int(n_frames),
                                                     int(first_frame), None if corr is None else corr.ctypes.data,
                                                     None if poses is None else poses.ctypes.data, ctypes.c_void_p(stream)))

    def tsdf_archive_move(self, frames, world_T_cam_new: np.ndarray, min_translation: float, min_rotation: float,
                          stream: int = 0) -> None:
        """The archived frames among ``frames`` [n] whose pose ``world_T_cam_new`` [n][4][4] differs
        from the stored one by more than the thresholds are taken out of the volume and integrated
        again at the new pose (queued on ``stream``; ``tsdf_archive_read`` tells how many moved)."""
        f = np.ascontiguousarray(np.asarray(frames, dtype=np.int64).reshape(-1))
        T = np.ascontiguousarray(np.asarray(world_T_cam_new, dtype=np.float64).reshape(-1, 4, 4))
        if T.shape[0] != f.shape[0]:
            raise ValueError("one pose per frame")
        _check(self.lib.tslam_tsdf_archive_move(self.h, int(f.shape[0]), f.ctypes.data, T.ctypes.data, float(min_translation),
                                                float(min_rotation), ctypes.c_void_p(stream)))

    def tsdf_archive_read(self, max_frames: int | None = None) -> dict:
        """The archive, oldest frame first (synchronises): ``frames`` i64 [n], ``world_T_cam`` f64
        [n][4][4] (the pose each frame is in the volume with), ``count`` (frames in the ring; n is at
        most ``max_frames``), ``moved_last`` and ``moved_total``."""
        cnt, last, total = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int64(0)
        _check(self.lib.tslam_tsdf_archive_read(self.h, 0, None, None, ctypes.byref(cnt), ctypes.byref(last), ctypes.byref(total)))
        n = cnt.value if max_frames is None else min(cnt.value, int(max_frames))
        f = np.zeros(n, dtype=np.int64)
        T = np.zeros((n, 4, 4), dtype=np.float64)
        if n:
            _check(self.lib.tslam_tsdf_archive_read(self.h, n, f.ctypes.data, T.ctypes.data, None, None, None))
        return {"frames": f, "world_T_cam": T, "count": cnt.value, "moved_last": last.value, "moved_total": total.value}

    def tsdf_archive_read_depth(self, index: int) -> np.ndarray:
        """The depth image u16 [H][W] of entry ``index`` of ``tsdf_archive_read``'s order (synchronises)."""
        out = np.zeros((self.height, self.width), dtype=np.uint16)
        _check(self.lib.tslam_tsdf_archive_read_depth(self.h, int(index), out.ctypes.data))
        return out

    def tsdf_integrate_rig(self, cams, n_frames: int, first_frame: int = 0, world_T_base: np.ndarray | None = None,
                           stream: int = 0) -> None:
        """Depth of several cameras of the rig (``set_rig``) into the volume in one launch, on the
        rig's body pose (thor_slam_amd/dense.py ``rig_world_T_cam``).  ``cams``: per camera a dict
        ``pair``, ``depth`` (device pointer, u16 mm), ``stride_bytes``, and optionally ``rect``
        (depth of the rectified camera) and ``color`` (device pointer, BGR), pairs strictly
        ascending.  ``world_T_base`` [n_frames][4][4] on the host, or None: the last batch's
        device-resident body poses of frames first_frame.. ."""
        arr = (TsdfRigCamera * max(len(cams), 1))()
        for i, c in enumerate(cams):
            arr[i] = TsdfRigCamera(int(c["pair"]), int(bool(c.get("rect", False))), int(c["depth"]) or None,
                                   int(c.get("color") or 0) or None, int(c["stride_bytes"]))
        poses = None
        if world_T_base is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_base, dtype=np.float64).reshape(-1, 4, 4))
        _check(self.lib.tslam_tsdf_integrate_rig(self.h, ctypes.addressof(arr), len(cams), int(n_frames), int(first_frame),
                                                 None if poses is None else poses.ctypes.data, ctypes.c_void_p(stream)))

    # -- the rolling window of the dense map (thor_slam_amd/dense_follow.py) ---------------------
    def tsdf_follow(self, anchor=None, margin: int = 32, step: int = 16, enable: bool = True) -> None:
        """The window follows the camera from the next integrate call on (``anchor`` None: the
        voxel of the tracking world's origin in the unshifted window); ``enable`` False turns it
        off and leaves the window where it is.  After ``tsdf_init``, which turns it off again."""
        if not enable:
            _check(self.lib.tslam_tsdf_follow(self.h, None))
            return
        if anchor is None:
            anchor = getattr(self, "_tsdf_anchor", (0, 0, 0))   # without tsdf_init the library refuses the call
        prm = TsdfFollowParams((ctypes.c_int32 * 3)(*[int(a) for a in anchor]), int(margin), int(step))
        _check(self.lib.tslam_tsdf_follow(self.h, ctypes.addressof(prm)))

    def tsdf_shift(self, delta, stream: int = 0) -> None:
        """Move the window by ``delta`` voxels (x, y, z) on the stream; what leaves is dropped, what
        enters is unobserved."""
        d = np.ascontiguousarray(delta, dtype=np.int32).reshape(3)
        _check(self.lib.tslam_tsdf_shift(self.h, d.ctypes.data, ctypes.c_void_p(stream)))

    def tsdf_window(self) -> tuple[np.ndarray, np.ndarray]:
        """(cumulative shift i32 [3] in voxels, effective origin f64 [3] in metres); synchronises."""
        sh = np.zeros(3, dtype=np.int32)
        o = np.zeros(3, dtype=np.float64)
        _check(self.lib.tslam_tsdf_window(self.h, sh.ctypes.data, o.ctypes.data))
        return sh, o

    # -- the brick store behind the window (thor_slam_amd/dense_store.py) --------------------------
    def tsdf_store_init(self, capacity_bricks: int) -> None:
        """A new, empty store of ``capacity_bricks`` 8 x 8 x 8 bricks for what leaves the window, sized
        for the layers the volume has now (after ``tsdf_color`` / ``tsdf_freespace_init``); 0 frees it."""
        _check(self.lib.tslam_tsdf_store_init(self.h, int(capacity_bricks)))

    def tsdf_store_stats(self) -> dict:
        """The store's counters (synchronises)."""
        out = np.zeros(8, dtype=np.int64)
        _check(self.lib.tslam_tsdf_store_stats(self.h, out.ctypes.data))
        keys = ("capacity", "bricks_allocated", "bricks", "voxels_stored", "voxels_dropped", "moves", "words_per_voxel")
        return {k: int(v) for k, v in zip(keys, out)}

    def tsdf_store_read(self) -> tuple[np.ndarray, np.ndarray]:
        """(bricks i32 [n][3] (bx, by, bz), words u32 [n][C][8][8][8]) of the bricks that hold a voxel,
        in ascending (bz, by, bx); C and the components' order as the move's layers (synchronises)."""
        n = ctypes.c_int64(0)
        _check(self.lib.tslam_tsdf_store_read(self.h, 0, None, None, ctypes.addressof(n)))
        c = self.tsdf_store_stats()["words_per_voxel"]
        xyz = np.zeros((n.value, 3), dtype=np.int32)
        words = np.zeros((n.value, c, 8, 8, 8), dtype=np.uint32)
        if n.value:
            _check(self.lib.tslam_tsdf_store_read(self.h, n.value, xyz.ctypes.data, words.ctypes.data, ctypes.addressof(n)))
        return xyz, words

    # -- the volume seen from a pose (thor_slam_amd/dense_render.py) -----------------------------
    def tsdf_render_init(self, width: int, height: int, fx: float, fy: float, cx: float, cy: float,
                         min_weight: float = 1e-4, min_depth: float = 0.0, max_depth: float = 10.0,
                         step_scale: float = 0.5, max_views: int = 1, outputs: int = 15) -> None:
        """The camera, the marching parameters, the outputs (bit mask: 1 depth_m, 2 depth_mm,
        4 normal, 8 color) and the most views of one ``tsdf_render`` call; after ``tsdf_init``."""
        prm = TsdfRenderParams(int(width), int(height), float(fx), float(fy), float(cx), float(cy), float(min_weight),
                               float(min_depth), float(max_depth), float(step_scale), int(outputs), 0)
        _check(self.lib.tslam_tsdf_render_init(self.h, ctypes.addressof(prm), int(max_views)))
        self._render = (int(height), int(width), int(outputs))

    def tsdf_render(self, world_T_cam: np.ndarray | None = None, n_views: int | None = None, first_frame: int = 0,
                    pair: int = 0, stream: int = 0) -> None:
        """Views 0.. of the volume on the stream (asynchronous): at the host poses ``world_T_cam``
        [n][4][4] (volume frame; a NaN pose gives a zero image), or with None at ``pair``'s tracked
        device poses of frames first_frame.. of the last batch (``n_views`` of them)."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
            n_views = poses.shape[0] if n_views is None else n_views
        elif n_views is None:
            raise ValueError("n_views is needed with device poses")
        self._render_poses = poses   # stays alive behind the asynchronous call
        _check(self.lib.tslam_tsdf_render(self.h, int(pair), None if poses is None else poses.ctypes.data, int(n_views),
                                          int(first_frame), ctypes.c_void_p(stream)))

    def tsdf_render_buffers(self) -> tuple[dict, dict]:
        """(device pointers, bytes of one view) per output name; 0 for an output not asked for."""
        names = ("depth_m", "depth_mm", "normal", "color")
        ptrs = [ctypes.c_void_p() for _ in names]
        nbytes = (ctypes.c_int64 * 4)()
        _check(self.lib.tslam_tsdf_render_buffers(self.h, *[ctypes.byref(p) for p in ptrs], ctypes.addressof(nbytes)))
        return {k: int(p.value or 0) for k, p in zip(names, ptrs)}, {k: int(b) for k, b in zip(names, nbytes)}

    def tsdf_render_read(self, view: int = 0) -> dict:
        """The outputs asked for of one view (synchronises): ``depth_m`` f32 [H][W], ``depth_mm`` u16
        [H][W], ``normal`` f32 [H][W][3], ``color`` u8 [H][W][3] (B, G, R)."""
        if getattr(self, "_render", None) is None:   # no tsdf_render_init yet: the library says so
            _check(self.lib.tslam_tsdf_render_read(self.h, int(view), None, None, None, None))
        H, W, outputs = self._render
        spec = (("depth_m", 1, (H, W), np.float32), ("depth_mm", 2, (H, W), np.uint16),
                ("normal", 4, (H, W, 3), np.float32), ("color", 8, (H, W, 3), np.uint8))
        out = {k: np.zeros(shape, dtype=dt) for k, bit, shape, dt in spec if outputs & bit}
        _check(self.lib.tslam_tsdf_render_read(self.h, int(view), *[out[k].ctypes.data if k in out else None
                                                                    for k, _, _, _ in spec]))
        return out

    # -- dense frame-to-model alignment (thor_slam_amd/dense_align.py) ---------------------------
    def tsdf_align_init(self, pair: int = 0, rect: bool = False, max_frames: int = 1, enable: bool = True, **params) -> None:
        """The camera (``pair``; ``rect``: the depth is the rectified camera's), the most frames of
        one ``tsdf_align`` call and the rule's parameters (``dense_align.DEFAULTS``); after
        ``tsdf_init``.  ``enable`` False frees the state."""
        from .dense_align import DEFAULTS

        if not enable:
            _check(self.lib.tslam_tsdf_align_init(self.h, 0, 0, None, 0))
            return
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown align parameters {sorted(unknown)}")
        p = {**DEFAULTS, **params}
        prm = TsdfAlignParams(int(p["iterations"]), int(p["min_inliers"]), float(p["max_distance"]), float(p["min_weight"]),
                              float(p["max_depth"]), float(p["step_scale"]), float(p["max_translation"]),
                              float(p["max_rotation"]), float(p["eps_translation"]), float(p["eps_rotation"]),
                              float(p["min_pivot"]), (ctypes.c_int32 * 4)())
        _check(self.lib.tslam_tsdf_align_init(self.h, int(pair), int(bool(rect)), ctypes.addressof(prm), int(max_frames)))

    def tsdf_align(self, depth_dev_ptr: int, stride_bytes: int, n_frames: int, first_frame: int = 0,
                   world_T_cam: np.ndarray | None = None, stream: int = 0) -> None:
        """Align n depth frames (device u16 mm, ``stride_bytes`` apart) to the map on the stream
        (asynchronous), from the host poses world_T_cam [n][4][4] (volume frame) or, with None, from
        the last batch's tracked device poses of frames first_frame.. ."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        self._align_poses = poses   # stays alive behind the asynchronous call
        _check(self.lib.tslam_tsdf_align(self.h, ctypes.c_void_p(depth_dev_ptr), int(stride_bytes), int(n_frames),
                                         int(first_frame), None if poses is None else poses.ctypes.data,
                                         ctypes.c_void_p(stream)))
        self._align_n = int(n_frames)

    def tsdf_align_read(self, n_frames: int | None = None) -> dict:
        """The last ``tsdf_align`` call's results (synchronises): ``world_T_cam`` f64 [n][4][4] (the
        aligned pose where the status is 0, else the initial pose), ``stats`` i32 [n][4] (status,
        iterations run, inliers of the first and of the last iteration), ``residuals`` f64 [n][2]
        (their rms residuals, metres), ``normal_eq`` f64 [n][28]."""
        n = getattr(self, "_align_n", 0) if n_frames is None else int(n_frames)
        out = {"world_T_cam": np.zeros((n, 4, 4)), "stats": np.zeros((n, 4), np.int32), "residuals": np.zeros((n, 2)),
               "normal_eq": np.zeros((n, 28))}
        _check(self.lib.tslam_tsdf_align_read(self.h, n, *[out[k].ctypes.data for k in ("world_T_cam", "stats", "residuals",
                                                                                         "normal_eq")]))
        return out

    def tsdf_align_buffers(self) -> dict:
        """Device pointers of ``world_T_cam`` (f64 [max_frames][16]) and ``stats`` (i32 [max_frames][4])."""
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        _check(self.lib.tslam_tsdf_align_buffers(self.h, ctypes.byref(a), ctypes.byref(b)))
        return {"world_T_cam": int(a.value or 0), "stats": int(b.value or 0)}

    def tsdf_integrate_aligned(self, depth_dev_ptr: int, stride_bytes: int, n_frames: int, color_dev_ptr: int | None = None,
                               stream: int = 0) -> None:
        """``tsdf_integrate`` (with ``color_dev_ptr``: ``tsdf_integrate_rgbd``) of n frames on the
        poses of the last ``tsdf_align`` call, which stay on the device."""
        _check(self.lib.tslam_tsdf_integrate_aligned(self.h, ctypes.c_void_p(color_dev_ptr) if color_dev_ptr else None,
                                                     ctypes.c_void_p(depth_dev_ptr), int(stride_bytes), int(n_frames),
                                                     ctypes.c_void_p(stream)))

    # -- the free-space depth mask (thor_slam_amd/dense_dynamic.py) -------------------------------
    def tsdf_dynamic_init(self, pair: int = 0, rect: bool = False, max_frames: int = 1, enable: bool = True, **params) -> None:
        """The camera (``pair``; ``rect``: the depth is the rectified camera's), the most frames of
        one ``tsdf_dynamic`` call and the rule's parameters (``dense_dynamic.DEFAULTS``); after
        ``tsdf_init``.  ``enable`` False frees the state."""
        from .dense_dynamic import DEFAULTS

        if not enable:
            _check(self.lib.tslam_tsdf_dynamic_init(self.h, 0, 0, None, 0))
            return
        unknown = set(params) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown dynamic-mask parameters {sorted(unknown)}")
        p = {**DEFAULTS, **params}
        prm = TsdfDynamicParams(float(p["min_free_weight"]), float(p["free_fraction"]), int(p["open_radius"]),
                                int(p["dilate_radius"]), (ctypes.c_int32 * 4)())
        _check(self.lib.tslam_tsdf_dynamic_init(self.h, int(pair), int(bool(rect)), ctypes.addressof(prm), int(max_frames)))

    def tsdf_dynamic(self, depth_dev_ptr: int, stride_bytes: int, n_frames: int, first_frame: int = 0,
                     world_T_cam: np.ndarray | None = None, stream: int = 0) -> None:
        """The mask and the filtered depth of n depth frames (device u16 mm, ``stride_bytes`` apart)
        into slots 0.. on the stream (asynchronous), at the host poses world_T_cam [n][4][4] (volume
        frame) or, with None, at the last batch's tracked device poses of frames first_frame.. ."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        self._dynamic_poses = poses   # stays alive behind the asynchronous call
        _check(self.lib.tslam_tsdf_dynamic(self.h, ctypes.c_void_p(depth_dev_ptr), int(stride_bytes), int(n_frames),
                                           int(first_frame), None if poses is None else poses.ctypes.data,
                                           ctypes.c_void_p(stream)))

    def tsdf_dynamic_buffers(self) -> tuple[dict, dict]:
        """(device pointers of ``depth`` u16 [max_frames][H][W], ``mask`` u8 [max_frames][H][W] and
        ``stats`` i32 [max_frames][4]; bytes of one frame's ``depth`` and ``mask``)."""
        names = ("depth", "mask", "stats")
        ptrs = [ctypes.c_void_p() for _ in names]
        nbytes = (ctypes.c_int64 * 2)()
        _check(self.lib.tslam_tsdf_dynamic_buffers(self.h, *[ctypes.byref(p) for p in ptrs], ctypes.addressof(nbytes)))
        return {k: int(p.value or 0) for k, p in zip(names, ptrs)}, {"depth": int(nbytes[0]), "mask": int(nbytes[1])}

    def tsdf_dynamic_read(self, frame: int = 0) -> dict:
        """One slot (synchronises): ``mask`` u8 [H][W] (0 or 1), ``depth`` u16 [H][W] (the looked-up
        depth, 0 under the mask), ``stats`` i32 [4] (status, valid pixels, candidates, valid pixels
        under the mask)."""
        out = {"depth": np.zeros((self.height, self.width), np.uint16), "mask": np.zeros((self.height, self.width), np.uint8),
               "stats": np.zeros(4, np.int32)}
        _check(self.lib.tslam_tsdf_dynamic_read(self.h, int(frame), *[out[k].ctypes.data for k in ("depth", "mask", "stats")]))
        return out

    # -- the free-space layer (thor_slam_amd/dense_freespace.py) -----------------------------------
    def tsdf_freespace_init(self, settle_frames: int = 0, occupied_band_vox: float = 1.5, enable: bool = True) -> None:
        """A new, all-zero layer: a voxel seen occupied (within ``occupied_band_vox`` voxels of a
        surface) by ``settle_frames`` consecutive frames of ``tsdf_dynamic`` calls is no longer
        masked; after ``tsdf_init``.  ``enable`` False frees the layer."""
        if not enable:
            _check(self.lib.tslam_tsdf_freespace_init(self.h, None))
            return
        prm = TsdfFreespaceParams(float(occupied_band_vox), int(settle_frames), (ctypes.c_int32 * 5)())
        _check(self.lib.tslam_tsdf_freespace_init(self.h, ctypes.addressof(prm)))

    def tsdf_freespace_read(self) -> np.ndarray:
        """The layer's words u32 [nz][ny][nx] (bits 0..15 ``run``, bit 16 ``settled``); synchronises."""
        if getattr(self, "_tsdf_dims", None) is None:   # no volume yet: the library says so
            _check(self.lib.tslam_tsdf_freespace_read(self.h, None))
        nx, ny, nz = self._tsdf_dims
        w = np.zeros((nz, ny, nx), dtype=np.uint32)
        _check(self.lib.tslam_tsdf_freespace_read(self.h, w.ctypes.data))
        return w

    def tsdf_freespace_write(self, words: np.ndarray) -> None:
        """Replace the layer's words (u32 [nz][ny][nx], no bit above 16; synchronises)."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        if getattr(self, "_tsdf_dims", None) is None:   # no volume yet: the library says so
            _check(self.lib.tslam_tsdf_freespace_write(self.h, w.ctypes.data))
        nx, ny, nz = self._tsdf_dims
        if w.shape != (nz, ny, nx):
            raise ValueError(f"layer must be {(nz, ny, nx)}")
        _check(self.lib.tslam_tsdf_freespace_write(self.h, w.ctypes.data))

    # -- depth registration (thor_slam_amd/depth_register.py) ------------------------------------
    def depth_register_init(self, color_width: int, color_height: int, f_c: float, cxc: float, cyc: float, color_T_rect,
                            map: np.ndarray | None = None, width: int | None = None, height: int | None = None,
                            max_depth_mm: int = 65535, tol_mm: int = 50, max_splat: int = 4, max_frames: int = 1,
                            pair: int = 0) -> None:
        """The colour camera of ``pair`` (undistorted pinhole ``f_c, cxc, cyc``, the table ``map`` i32
        [Hc][Wc][2] or None, ``color_T_rect`` 12 values), the depth image's size (default: the
        handle's), the rule's parameters and the output slots of ``depth_register``."""
        T = np.ascontiguousarray(color_T_rect, dtype=np.float64).reshape(-1)
        if T.size != 12:
            raise ValueError("color_T_rect must hold 12 values (3 x 4, row-major)")
        width = self.width if width is None else int(width)
        height = self.height if height is None else int(height)
        mp = None
        if map is not None:
            mp = np.ascontiguousarray(map, dtype=np.int32)
            if mp.shape != (int(color_height), int(color_width), 2):
                raise ValueError(f"map must be {(int(color_height), int(color_width), 2)}")
        prm = DepthRegisterParams(width, height, int(color_width), int(color_height), float(f_c), float(cxc), float(cyc),
                                  None if mp is None else mp.ctypes.data, (ctypes.c_double * 12)(*[float(v) for v in T]),
                                  int(max_depth_mm), int(tol_mm), int(max_splat), 0)
        _check(self.lib.tslam_depth_register_init(self.h, int(pair), ctypes.addressof(prm), int(max_frames)))
        if not hasattr(self, "_dr_shape"):
            self._dr_shape = {}
        self._dr_shape[int(pair)] = (height, width, int(color_height), int(color_width))

    def depth_register(self, depth_dev_ptr: int, depth_stride: int, color_dev_ptr: int, color_stride: int, n_frames: int,
                       first_slot: int = 0, pair: int = 0, stream: int = 0) -> None:
        """n frames of device depth (u16 mm) and raw BGR colour planes into slots first_slot .. on the
        stream (asynchronous); the other slots keep their contents."""
        _check(self.lib.tslam_depth_register(self.h, int(pair), ctypes.c_void_p(depth_dev_ptr), int(depth_stride),
                                             ctypes.c_void_p(color_dev_ptr), int(color_stride), int(n_frames),
                                             int(first_slot), ctypes.c_void_p(stream)))

    def depth_register_blank(self, n_frames: int, first_slot: int = 0, pair: int = 0, stream: int = 0) -> None:
        """Zero ``bgr`` and ``mask`` of slots first_slot .. on the stream (frames without a colour
        image); their registered depth keeps its contents."""
        _check(self.lib.tslam_depth_register_blank(self.h, int(pair), int(n_frames), int(first_slot), ctypes.c_void_p(stream)))

    def depth_register_buffers(self, pair: int = 0) -> tuple[dict, dict]:
        """(device pointers, bytes of one slot) of ``depth`` (registered), ``bgr`` and ``mask``."""
        names = ("depth", "bgr", "mask")
        ptrs = [ctypes.c_void_p() for _ in names]
        nbytes = (ctypes.c_int64 * 3)()
        _check(self.lib.tslam_depth_register_buffers(self.h, int(pair), *[ctypes.byref(p) for p in ptrs],
                                                     ctypes.addressof(nbytes)))
        return {k: int(p.value or 0) for k, p in zip(names, ptrs)}, {k: int(b) for k, b in zip(names, nbytes)}

    def depth_register_read(self, slot: int = 0, pair: int = 0) -> dict:
        """One slot (synchronises): ``depth`` u16 [Hc][Wc] (mm, in the undistorted colour camera),
        ``bgr`` u8 [H][W][3] and ``mask`` u8 [H][W] (registered to the depth)."""
        shape = getattr(self, "_dr_shape", {}).get(int(pair))
        if shape is None:   # no depth_register_init for the pair yet: the library says so
            _check(self.lib.tslam_depth_register_read(self.h, int(pair), int(slot), None, None, None))
            raise RuntimeError("depth_register_read without depth_register_init through this Handle")
        H, W, Hc, Wc = shape
        out = {"depth": np.zeros((Hc, Wc), np.uint16), "bgr": np.zeros((H, W, 3), np.uint8), "mask": np.zeros((H, W), np.uint8)}
        _check(self.lib.tslam_depth_register_read(self.h, int(pair), int(slot), out["depth"].ctypes.data, out["bgr"].ctypes.data,
                                                  out["mask"].ctypes.data))
        return out

    def depth_register_profile(self, enable: bool = True, read: bool = False) -> dict | None:
        """Time the three passes of every later ``depth_register`` call; ``read``: the newest timed
        call's times in ms first (waits for it)."""
        ms = (ctypes.c_double * 3)()
        _check(self.lib.tslam_depth_register_profile(self.h, int(bool(enable)), ctypes.addressof(ms) if read else None))
        return dict(zip(("clear", "splat", "gather"), ms)) if read else None

    def tsdf_integrate_rect_color(self, color_dev_ptr: int, color_stride: int, mask_dev_ptr: int | None, mask_stride: int,
                                  depth_dev_ptr: int, stride_bytes: int, n_frames: int, first_frame: int = 0,
                                  world_T_cam: np.ndarray | None = None, pair: int = 0, stream: int = 0) -> None:
        """``tsdf_integrate_rect`` with BGR colour [H][W][3] (frames ``color_stride`` apart) and a
        visibility mask u8 [H][W] (``mask_stride`` apart; None: every pixel): what ``depth_register``
        writes.  The colour layer is updated only where the mask is non-zero."""
        poses = None
        if world_T_cam is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_cam, dtype=np.float64).reshape(-1, 4, 4))
        _check(self.lib.tslam_tsdf_integrate_rect_color(
            self.h, int(pair), ctypes.c_void_p(color_dev_ptr) if color_dev_ptr else None, int(color_stride),
            ctypes.c_void_p(mask_dev_ptr) if mask_dev_ptr else None, int(mask_stride), ctypes.c_void_p(depth_dev_ptr),
            int(stride_bytes), int(n_frames), int(first_frame), None if poses is None else poses.ctypes.data,
            ctypes.c_void_p(stream)))

    def tsdf_integrate_rig_color(self, cams, n_frames: int, first_frame: int = 0, world_T_base: np.ndarray | None = None,
                                 stream: int = 0) -> None:
        """``tsdf_integrate_rig`` where every camera's dict also has ``color`` (device pointer, BGR
        [H][W][3]), ``color_stride``, and optionally ``mask`` (device pointer, u8 [H][W]) with
        ``mask_stride``: colour with strides of its own, updated only where the mask is non-zero."""
        arr = (TsdfRigCamera * max(len(cams), 1))()
        col = (TsdfRigColor * max(len(cams), 1))()
        for i, c in enumerate(cams):
            arr[i] = TsdfRigCamera(int(c["pair"]), int(bool(c.get("rect", False))), int(c["depth"]) or None, None,
                                   int(c["stride_bytes"]))
            col[i] = TsdfRigColor(int(c.get("color") or 0) or None, int(c.get("color_stride", 0)),
                                  int(c.get("mask") or 0) or None, int(c.get("mask_stride", 0)))
        poses = None
        if world_T_base is not None:
            poses = np.ascontiguousarray(np.asarray(world_T_base, dtype=np.float64).reshape(-1, 4, 4))
        _check(self.lib.tslam_tsdf_integrate_rig_color(self.h, ctypes.addressof(arr), ctypes.addressof(col), len(cams),
                                                       int(n_frames), int(first_frame),
                                                       None if poses is None else poses.ctypes.data, ctypes.c_void_p(stream)))

    # -- dense stereo depth (thor_slam_amd/stereo_depth.py) ------------------------------------
    def stereo_depth_init(self, max_frames: int = 1, n_disp: int = 0, uniqueness: int = 10, lr_tol: int = 1) -> None:
        """Parameters and output slots of the dense stereo matcher (n_disp 0 = the handle's
        max_disparity)."""
        prm = (ctypes.c_int32 * 4)(int(n_disp), int(uniqueness), int(lr_tol), 0)
        _check(self.lib.tslam_stereo_depth_init(self.h, ctypes.addressof(prm), int(max_frames)))
        self._sd_shape = (self.height, self.width)

    def stereo_depth_sgm(self, p1: int = 100, p2: int = 1200, paths: int = 15, enable: bool = True,
                         chunk_frames: int = 0) -> None:
        """Semi-global aggregation (rule 3a) on or off, after ``stereo_depth_init`` (which turns it
        off again); ``chunk_frames`` 0 lets the library size its scratch."""
        prm = StereoDepthSgmParams(int(bool(enable)), int(p1), int(p2), int(paths), int(chunk_frames), (ctypes.c_int32 * 3)())
        _check(self.lib.tslam_stereo_depth_sgm(self.h, ctypes.addressof(prm)))

    def stereo_depth_filter(self, median: int = 5, speckle_size: int = 50, speckle_range: int = 32, enable: bool = True) -> None:
        """The median (rule 9) and speckle (rule 10) filters on or off, after ``stereo_depth_init``
        (which turns them off again); independent of ``stereo_depth_sgm``."""
        prm = StereoDepthFilterParams(int(bool(enable)), int(median), int(speckle_size), int(speckle_range),
                                      (ctypes.c_int32 * 4)())
        _check(self.lib.tslam_stereo_depth_filter(self.h, ctypes.addressof(prm)))

    def stereo_depth_filter_apply(self, disp32_dev_ptr: int, width: int, height: int, fxb: float, n_frames: int,
                                  stream: int = 0) -> None:
        """The enabled filters and the depth on caller-supplied dense device planes of disp32 (u16
        [n_frames][height][width]) into slots 0..n_frames-1."""
        _check(self.lib.tslam_stereo_depth_filter_apply(self.h, ctypes.c_void_p(disp32_dev_ptr), int(width), int(height),
                                                        float(fxb), int(n_frames), ctypes.c_void_p(stream)))
        self._sd_shape = (int(height), int(width))

    def stereo_depth(self, first_frame: int, n_frames: int, pair: int = 0, stream: int = 0, first_slot: int = 0) -> None:
        """Depth of ``pair``'s frames first_frame.. of the last batch into slots first_slot ..
        first_slot + n_frames - 1 (the other slots keep their depth and disp32)."""
        _check(self.lib.tslam_stereo_depth_slots(self.h, int(pair), int(first_frame), int(n_frames), int(first_slot),
                                                 ctypes.c_void_p(stream)))
        self._sd_shape = (self.height, self.width)

    def stereo_depth_images(self, left_dev_ptr: int, right_dev_ptr: int, frame_stride: int, width: int, height: int,
                            fxb: float, n_frames: int, stream: int = 0) -> None:
        """The matcher on caller-supplied rectified device images (u8, dense rows, frames
        ``frame_stride`` bytes apart); outputs dense [n_frames][height][width]."""
        _check(self.lib.tslam_stereo_depth_images(self.h, ctypes.c_void_p(left_dev_ptr), ctypes.c_void_p(right_dev_ptr),
                                                  int(frame_stride), int(width), int(height), float(fxb), int(n_frames),
                                                  ctypes.c_void_p(stream)))
        self._sd_shape = (int(height), int(width))

    def stereo_depth_buffers(self) -> tuple[int, int, int]:
        """(depth device pointer, disp32 device pointer, bytes of one full-size slot)."""
        d, q, b = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        _check(self.lib.tslam_stereo_depth_buffers(self.h, ctypes.byref(d), ctypes.byref(q), ctypes.byref(b)))
        return int(d.value or 0), int(q.value or 0), int(b.value)

    def stereo_depth_read(self, slot: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(depth u16 mm, disp32 u16 in 1/32 px) of one slot of the last call (synchronises)."""
        depth = np.zeros(self._sd_shape, dtype=np.uint16)
        disp = np.zeros(self._sd_shape, dtype=np.uint16)
        _check(self.lib.tslam_stereo_depth_read(self.h, int(slot), depth.ctypes.data, disp.ctypes.data))
        return depth, disp

    def tsdf_read(self) -> tuple[np.ndarray, np.ndarray]:
        """(tsdf, weight) as f32 [nz][ny][nx] (synchronises)."""
        nx, ny, nz = self._tsdf_dims
        t = np.zeros((nz, ny, nx), dtype=np.float32)
        w = np.zeros((nz, ny, nx), dtype=np.float32)
        _check(self.lib.tslam_tsdf_read(self.h, t.ctypes.data, w.ctypes.data))
        return t, w

    def tsdf_write(self, tsdf: np.ndarray, weight: np.ndarray) -> None:
        """Replace the volume (f32 [nz][ny][nx] each; synchronises)."""
        nx, ny, nz = self._tsdf_dims
        t = np.ascontiguousarray(tsdf, dtype=np.float32)
        w = np.ascontiguousarray(weight, dtype=np.float32)
        if t.shape != (nz, ny, nx) or w.shape != (nz, ny, nx):
            raise ValueError(f"volume must be {(nz, ny, nx)}")
        _check(self.lib.tslam_tsdf_write(self.h, t.ctypes.data, w.ctypes.data))

    # -- dense-map outputs (nvblox's mesh / ESDF / distance slice; thor_slam_amd/dense.py) -------
    def mesh(self, min_weight: float = 1e-4, stream: int = 0, colors: bool = False):
        """Marching-cubes triangle soup [n][3][3] f32 (metres), cube order (synchronises); with
        ``colors`` (colour layer) also the vertex colours [n][3][3] f32: (triangles, colours)."""
        n = ctypes.c_int64()
        _check(self.lib.tslam_mesh_extract(self.h, float(min_weight), ctypes.byref(n), ctypes.c_void_p(stream)))
        out = np.zeros((n.value, 3, 3), dtype=np.float32)
        _check(self.lib.tslam_mesh_read(self.h, out.ctypes.data, int(n.value)))
        if not colors:
            return out
        col = np.zeros((n.value, 3, 3), dtype=np.float32)
        if n.value:
            _check(self.lib.tslam_mesh_read_colors(self.h, col.ctypes.data, int(n.value)))
        return out, col

    def mesh_whole(self, min_weight: float = 1e-4, stream: int = 0, colors: bool = False):
        """The mesh of the whole map, window and brick store together (thor_slam_amd/dense_store.py):
        what ``mesh`` returns, brick by brick in ascending (bz, by, bx), vertices from absolute voxel
        coordinates and the configured origin.  ``mesh_whole_bricks`` is the number of bricks visited.
        The two extracts share the handle's buffer (synchronises)."""
        n, nb = ctypes.c_int64(), ctypes.c_int64()
        _check(self.lib.tslam_mesh_extract_whole(self.h, float(min_weight), ctypes.byref(n), ctypes.byref(nb),
                                                 ctypes.c_void_p(stream)))
        self.mesh_whole_bricks = int(nb.value)
        out = np.zeros((n.value, 3, 3), dtype=np.float32)
        _check(self.lib.tslam_mesh_read(self.h, out.ctypes.data, int(n.value)))
        if not colors:
            return out
        col = np.zeros((n.value, 3, 3), dtype=np.float32)
        if n.value:
            _check(self.lib.tslam_mesh_read_colors(self.h, col.ctypes.data, int(n.value)))
        return out, col

    def esdf(self, max_dist: float = 2.0, site_vox: float = 1.0, min_weight: float = 1e-4, stream: int = 0) -> np.ndarray:
        """Signed distance field f32 [nz][ny][nx] (NaN = unobserved; synchronises)."""
        nx, ny, nz = self._tsdf_dims
        _check(self.lib.tslam_esdf_compute(self.h, float(max_dist), float(site_vox), float(min_weight),
                                           ctypes.c_void_p(stream)))
        out = np.zeros((nz, ny, nx), dtype=np.float32)
        _check(self.lib.tslam_esdf_read(self.h, out.ctypes.data))
        return out

    def esdf_slice(self, y0: int, y1: int, max_dist: float = 2.0, site_vox: float = 1.0,
                   min_weight: float = 1e-4) -> np.ndarray:
        """2-D distance map f32 [nz][nx] over the height band y0 <= j < y1 (NaN = unobserved column)."""
        nx, ny, nz = self._tsdf_dims
        out = np.zeros((nz, nx), dtype=np.float32)
        _check(self.lib.tslam_esdf_slice(self.h, int(y0), int(y1), float(max_dist), float(site_vox), float(min_weight),
                                         out.ctypes.data))
        return out

    def ba_imu_factor(self, frame: int, M: np.ndarray, weight: float, pair: int = 0) -> None:
        """IMU rotation factor of keyframe ``frame`` (the rotation from the previous keyframe's
        camera, 3x3, and its weight) for the local BA window."""
        m = np.ascontiguousarray(M, dtype=np.float64).reshape(9)
        _check(self.lib.tslam_ba_imu_factor(self.h, int(pair), int(frame), m.ctypes.data, float(weight)))

    def ba_replay_schur(self, pair: int = 0, reps: int = 50, stream: int = 0) -> dict:
        """Average k_ba_schur duration (HIP events around ``reps`` replays) and flops per launch."""
        us, fl = ctypes.c_double(), ctypes.c_double()
        _check(self.lib.tslam_ba_replay_schur(self.h, int(pair), int(reps), ctypes.c_void_p(stream), ctypes.byref(us),
                                              ctypes.byref(fl)))
        return {"us": us.value, "flops": fl.value, "reps": int(reps)}

    def ba_inertial(self, gravity, ba_prior, ba_weight: float, bg_prior=None, bg_weight: float = 0.0,
                    pair: int = 0) -> None:
        """World gravity and the priors (value, weight) on the oldest window keyframe's
        accelerometer and gyroscope biases for pair's window (tslam.h)."""
        g = np.ascontiguousarray(gravity, dtype=np.float64).reshape(3)
        b = np.ascontiguousarray(ba_prior, dtype=np.float64).reshape(3)
        bg = np.ascontiguousarray(np.zeros(3) if bg_prior is None else bg_prior, dtype=np.float64).reshape(3)
        _check(self.lib.tslam_ba_inertial(self.h, int(pair), g.ctypes.data, b.ctypes.data, float(ba_weight),
                                          bg.ctypes.data, float(bg_weight)))

    def ba_inertial_factor(self, frame: int, record, v0, pair: int = 0) -> None:
        """Keyframe ``frame``'s inertial factor record (INE_RECORD doubles, oracle INE_N layout) and
        initial velocity, before its batch is submitted."""
        r = np.zeros(INE_RECORD)
        src = np.asarray(record, dtype=np.float64).reshape(-1)[:INE_RECORD]
        r[:src.size] = src
        v = np.ascontiguousarray(v0, dtype=np.float64).reshape(3)
        _check(self.lib.tslam_ba_inertial_factor(self.h, int(pair), int(frame), r.ctypes.data, v.ctypes.data))

    def ba_read_inertial(self, pair: int = 0) -> dict:
        """Velocities [W][3] and accelerometer / gyroscope biases [W][6] by slot (synchronises)."""
        vel = np.zeros((self.cfg.ba_window, 3))
        bias = np.zeros((self.cfg.ba_window, 6))
        _check(self.lib.tslam_ba_read_inertial(self.h, int(pair), vel.ctypes.data, bias.ctypes.data))
        return {"vel": vel, "bias": bias}

    def ba_defer(self, defer: bool) -> None:
        """``tslam_ba_defer``: a BA stage on its own stream is enqueued at the next flush point
        (the next batch's first back stage, or any state read) instead of inside the stage call."""
        _check(self.lib.tslam_ba_defer(self.h, int(bool(defer))))

    def select_mode(self, mode: str = "auto", resident_cap: int = 0) -> None:
        """``tslam_select_mode`` (test hook): the top-K selection's path, ``auto`` / ``generic`` (global
        sweeps) / ``resident`` (LDS wherever it fits), and a cap on the resident candidates (0: built in)."""
        _check(self.lib.tslam_select_mode(self.h, SELECT_MODE[mode], int(resident_cap)))

    def match_mode(self, mode: str = "auto", merge_cap: int = 0) -> None:
        """``tslam_match_mode`` (test hook): k_match's train-side flush, ``auto`` / ``direct`` (every wave's
        own atomics) / ``merged`` (per block in LDS), and a cap on the merged window positions (0: built in)."""
        _check(self.lib.tslam_match_mode(self.h, MATCH_MODE[mode], int(merge_cap)))

    def match_layout(self, layout: str = "fused") -> None:
        """``tslam_match_layout`` (test hook): ``fused``, a k_match block matches both sides of its
        tile (default), or ``split``, one block per side (the tests' reference)."""
        _check(self.lib.tslam_match_layout(self.h, MATCH_LAYOUT[layout]))

    def describe_mode(self, list_cap: int = 0) -> None:
        """``tslam_describe_mode`` (test hook): a cap on the y-sorted positions a k_describe tile lists at
        a time (0: built in); a tile whose rows hold more is served in chunks."""
        _check(self.lib.tslam_describe_mode(self.h, int(list_cap)))

    def match_counters(self) -> dict:
        """``tslam_match_counters``: the matcher's path counts since the last call (the first call switches
        counting on), per mode ``merged`` / ``direct`` / ``flushed`` / ``empty_blocks`` / ``walked_blocks``, and ``blocks_per_cu``."""
        cnt = (ctypes.c_uint32 * 16)()
        bpc = ctypes.c_int(0)
        _check(self.lib.tslam_match_counters(self.h, cnt, ctypes.byref(bpc)))
        names = ("merged", "direct", "flushed", "empty_blocks", "walked_blocks")
        out = {m: {k: int(cnt[8 * i + j]) for j, k in enumerate(names)} for i, m in enumerate(("stereo", "temporal"))}
        out["blocks_per_cu"] = bpc.value
        return out

    def detect_counters(self) -> list:
        """``tslam_detect_counters``: the detector's flush rounds since the last call (the first call
        switches counting on).  Per level a dict: for ``bright`` / ``dark`` (phase B) the ``inloop``
        rounds, the ``pooled`` tail rounds and the ``lanes`` filled in them; for ``nms`` the ``inloop``
        rounds, the waves' own ``partial`` tail rounds and their ``lanes``; and the ``blocks`` run."""
        L = self.cfg.n_levels
        cnt = (ctypes.c_uint32 * (DET_COUNTERS * L))()
        _check(self.lib.tslam_detect_counters(self.h, cnt, L))
        out = []
        for l in range(L):
            lev = {s: {k: int(cnt[DET_COUNTERS * l + 3 * i + j]) for j, k in enumerate(("inloop", "partial" if s == "nms" else "pooled", "lanes"))}
                   for i, s in enumerate(("bright", "dark", "nms"))}
            lev["blocks"] = int(cnt[DET_COUNTERS * l + DET_COUNTER_BLOCKS])
            out.append(lev)
        return out

    def ba_graph(self, enable: bool) -> None:
        """Pair windows' keyframe chains by direct launches (default) or, opt-in, from captured hipGraphs (tslam.h)."""
        _check(self.lib.tslam_ba_graph(self.h, int(bool(enable))))

    def ba_split_solve(self, split: bool) -> None:
        """k_ba_reduce + k_ba_solve (kernel boundary) instead of k_ba_reduce_solve (tslam.h)."""
        _check(self.lib.tslam_ba_split_solve(self.h, int(bool(split))))

    def ba_profile(self, max_launches: int = 0) -> dict:
        """Schur-kernel HIP-event time / launches / algorithmic flops since the last call; re-arms
        timing for up to ``max_launches`` launches (0 = off).  Synchronises."""
        ms, n, fl = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        _check(self.lib.tslam_ba_profile(self.h, int(max_launches), ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl)))
        return {"ms": ms.value, "launches": int(n.value), "flops": fl.value}

    # -- decoding helpers (tests / map export) ---------------------------------------------
    def keypoints(self, global_frame: int, cam: int) -> dict:
        """Decoded keypoints of one camera at a global frame (must still be in the ring)."""
        slot = self.ring_slot(global_frame)
        C = self.n_cams
        kp = self.frame_block("keypoints", slot, np.uint32).reshape(C, self.K, 2)[cam]
        cnt = self.frame_block("kcount", slot, np.int32).reshape(C, self.n_levels)[cam]
        desc = self.frame_block("desc", slot, np.uint32).reshape(C, self.K, 8)[cam]
        return {
            "x": (kp[:, 0] & 0xFFFF).astype(np.int64), "y": (kp[:, 0] >> 16).astype(np.int64),
            "level": (kp[:, 1] & 0xFF).astype(np.int64), "angle": ((kp[:, 1] >> 8) & 0xFF).astype(np.int64),
            "score": (kp[:, 1] >> 16).astype(np.int64), "counts": cnt.astype(np.int64), "desc": desc,
        }


class LoopJob:
    """One ``tslam_loop_job_*`` on the handle's loop stream; ``result(block)`` returns its outputs
    once (None while it runs and ``block`` is False)."""

    def __init__(self, handle: Handle, job_id: int, kind: str, n: int = 0):
        self.handle, self.id, self.kind, self.n = handle, int(job_id), kind, int(n)
        self._res = None

    def result(self, block: bool = False):
        if self._res is not None:
            return self._res
        h = self.handle
        if self.kind == "vote":
            votes = np.zeros(max(self.n, 1), dtype=np.int32)
            rc = h.lib.tslam_loop_job_poll(h.h, self.id, int(block), votes.ctypes.data, None, None, None, None, None)
            out = votes[:self.n]
        elif self.kind == "verify":
            T, cov, st = np.zeros((4, 4)), np.zeros((6, 6)), np.zeros(8, dtype=np.int32)
            rc = h.lib.tslam_loop_job_poll(h.h, self.id, int(block), None, T.ctypes.data, cov.ctypes.data, st.ctypes.data,
                                           None, None)
            out = {"T": T, "cov": cov, "stats": st}
        else:
            T, cost = np.zeros((self.n, 4, 4)), ctypes.c_double()
            rc = h.lib.tslam_loop_job_poll(h.h, self.id, int(block), None, None, None, None, T.ctypes.data,
                                           ctypes.byref(cost))
            out = {"T": T, "cost": cost.value}
        if rc < 0:
            _check(rc)
        if rc == 0:
            return None
        self._res = out
        return out


class HandleGroup:
    """``tslam_group_create``: the handles (one per rank, the same rig) driven as one sharded rig
    by the library from this process — an RCCL clique over their devices (``transport="rccl"``,
    one device per handle) or device copies (``"copy"``, ranks may share a device)."""

    def __init__(self, handles: list, transport: str = "rccl"):
        self.lib = load_library()
        self.handles = list(handles)
        arr = (ctypes.c_void_p * len(handles))(*[h.h.value for h in handles])
        g = ctypes.c_void_p()
        _check(self.lib.tslam_group_create(arr, len(handles), TRANSPORT[transport], ctypes.byref(g)))
        self.g = g

    def submit(self, image_ptrs: list[int], n_frames: int | None = None, streams: list[int] | None = None) -> None:
        """One batch of ``n_frames`` (default max_batch; a multiple of the rank count): rank r's
        cameras at device pointer image_ptrs[r] (layout of tslam_submit_sharded)."""
        imgs = (ctypes.c_void_p * len(image_ptrs))(*[int(p) for p in image_ptrs])
        sts = None if streams is None else (ctypes.c_void_p * len(streams))(*[int(s) for s in streams])
        n = self.handles[0].max_batch if n_frames is None else int(n_frames)
        _check(self.lib.tslam_group_submit(self.g, imgs, n, sts))

    def close(self) -> None:
        if getattr(self, "g", None):
            self.lib.tslam_group_destroy(self.g)
            self.g = None

    def __del__(self):  # noqa: D105
        try:
            self.close()
        except Exception:
            pass
