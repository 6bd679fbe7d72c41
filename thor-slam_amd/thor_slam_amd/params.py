"""Engine configuration for the MI355X back end.

``HipSlamConfig`` extends the reference ``SlamConfig`` (interface.py:141-165) with the knobs of
the per-frame hot path (SURVEY.md §5 "Config / flags").  Every field has the same meaning in the
NumPy oracle and in the HIP kernels; ``to_c_params`` packs them for the C-ABI
(``include/tslam.h``: ``tslam_params``).
"""

from __future__ import annotations

from dataclasses import dataclass

from .dense_align import DEFAULTS as ALIGN_DEFAULTS, check_align_params
from .dense_dynamic import check_dynamic_params
from .dense_freespace import check_freespace_params
from .dense_follow import check_follow_params
from .dense_store import check_store_params
from .dense_loop import check_loop_params
from .dense_rig import DenseCamerasError
from .slam.interface import SlamConfig
from .stereo_depth import check_params as check_stereo_depth_params
from .stereo_depth import check_filter_params as check_stereo_depth_filter_params
from .stereo_depth import check_sgm_params as check_stereo_depth_sgm_params

# Upper bounds baked into the kernels (checked on the host before any launch).
MAX_WIDTH = 2047
MAX_HEIGHT = 2047
MAX_LEVELS = 6
MAX_FEATURES = 8192
MAX_HYPOTHESES = 1024


@dataclass
class HipSlamConfig(SlamConfig):
    # A4 detect
    n_features: int = 2000          # K keypoints per image, split over pyramid levels by area
    n_levels: int = 4               # integer 2x2 box pyramid levels
    fast_threshold: int = 20        # FAST-9: corner iff score > threshold
    edge_margin: int = 19           # keypoints keep this distance from every level border
    # A6 match
    max_hamming: int = 64           # accept best distance <= this
    ratio_pct: int = 80             # accept best*100 < ratio_pct*second
    stereo_row_tol: int = 1         # |y_L - y_R| <= tol (level pixels) after rectification
    max_disparity: int = 128        # level-0 pixels; disparity range [1, max_disparity >> level]
    temporal_window: int = 80       # level-0 pixels; |dx|,|dy| <= window >> level between frames
    # A7 pose
    ransac_hypotheses: int = 128    # P3P minimal samples per frame
    ransac_thr_px: float = 2.0      # reprojection inlier threshold (level-0 pixels)
    ransac_seed: int = 0x5EED
    refine_iters: int = 8           # Gauss-Newton iterations on inliers
    min_inliers: int = 12           # fewer -> frame is LOST
    # A8 local bundle adjustment (config C4); ba_window = 0 disables it
    ba_window: int = 0              # keyframes in the sliding window
    ba_kf_interval: int = 5         # frame g is a keyframe iff g % ba_kf_interval == 0
    ba_iters: int = 5               # Gauss-Newton steps per window solve
    ba_lambda: float = 1.0          # Levenberg damping (px^2 units)
    ba_outlier_px: float = 3.0      # observations farther than this at the start are dropped
    # IMU fusion (thor_slam_amd/imu.py): the bias-corrected gyro rotation as a
    # prior in the pose Gauss-Newton, with a gyroscope-bias state; None = on when the calibration
    # carries the IMU extrinsics (the reference runs cuVSLAM with enable_imu_fusion:=true,
    # Makefile:81; launch/thor_visual_slam.launch.py:69)
    imu_fusion: bool | None = None
    # ... plus the accelerometer leg: velocity / gravity / accelerometer-bias state with the IMU
    # lever arm, a translation prior, and IMU chaining through visual dropouts (None = with
    # imu_fusion)
    imu_accel: bool | None = None
    # ... and, with local BA, the tightly coupled inertial factors: the IMU preintegrated between
    # BA keyframes, a velocity and accelerometer / gyroscope biases per keyframe (tied by the bias
    # random walks) inside the BA (oracle/numpy_ba.py inertial_system); floors of the velocity and
    # position weights' standard deviations (m/s, m)
    ba_inertial: bool = True
    ba_inertial_v_floor: float = 1e-2
    ba_inertial_p_floor: float = 1e-3
    # the record's gyro-rotation rows and the bias random walks between window keyframes (weights
    # from the gyroscope noise density and both random walks of launch/thor_visual_slam.launch.py:
    # 50-53,88-93, floored: rad, m/s^2, rad/s)
    ba_inertial_r_floor: float = 1e-3
    ba_inertial_ba_floor: float = 1e-3
    ba_inertial_bg_floor: float = 1e-3
    # noise model, launch/thor_visual_slam.launch.py:82-93 (calibrated on a 2.5 h rosbag, :97-104)
    gyroscope_noise_density: float = 8.27e-5        # rad/s/sqrt(Hz)   (launch:82)
    accelerometer_noise_density: float = 2.553e-3   # m/s^2/sqrt(Hz)   (launch:85)
    gyroscope_random_walk: float = 1e-8             # rad/s^2/sqrt(Hz) (launch:88)
    accelerometer_random_walk: float = 1.0493e-4    # m/s^3/sqrt(Hz)   (launch:91)
    imu_rot_floor: float = 2e-4     # rad, added in quadrature to the predicted rotation's std (sync, calibration)
    imu_vis_rot_floor: float = 1e-4  # rad, the vision's per-frame rotation error beyond its covariance
    imu_trans_floor: float = 1e-3   # m, added in quadrature to the predicted translation's std
    imu_gyro_bias_sigma: float = 0.01   # rad/s, initial gyroscope-bias std
    imu_accel_bias_sigma: float = 0.05  # m/s^2, initial accelerometer-bias std
    # batches whose vision the prior of the next batch may lack (oracle/numpy_imu.py lagged_priors):
    # the prior of batch s comes from the filter with the vision of batches <= s - 1 - lag absorbed,
    # coasted over the rest, so up to `lag` batches stay in flight; 0 = synchronous (each batch
    # waits for the previous one's vision)
    imu_prior_lag: int = 1
    # loop closure + keyframe pose graph; on when the reference's
    # SlamConfig.enable_loop_closure is (interface.py:155-156; single stereo pair / RGB-D camera)
    loop_kf_interval: int = 5       # frame g is a loop-closure keyframe iff g % loop_kf_interval == 0
    loop_max_keyframes: int = 1024  # keyframe database entries (= pose-graph nodes)
    loop_signature: int = 256       # place-recognition descriptors per keyframe
    loop_min_gap: int = 20          # candidates are at least this many keyframes older
    loop_min_votes: int = 40        # signature votes a candidate needs
    loop_min_inliers: int = 40      # verified RANSAC inliers a loop edge needs
    pg_iters: int = 8               # Gauss-Newton iterations per pose-graph solve
    pg_sigma_t: float = 0.01        # m, std of an edge's translation
    pg_sigma_r: float = 0.005       # rad, std of an edge's rotation
    # asynchronous loop closure (oracle/numpy_loop.py LoopPolicy): the search a keyframe g starts
    # (signature votes, verification, the pose-graph solve of the loop's span) runs on the device
    # beside tracking, and its correction applies from frame g + loop_latency on; 0 = at g itself
    loop_latency: int = 30
    # a verified loop is not closed (no edge, no solve) within this many keyframes after the last
    # closed loop: revisiting a known place would otherwise re-solve the span at every keyframe
    loop_cooldown: int = 5
    # relocalisation after a LOST run (the reference's TrackingState.RELOCALIZING, interface.py:16-23;
    # cuVSLAM's enable_localization_n_mapping, launch/thor_visual_slam.launch.py:42,74): the
    # reloc_after_lost-th consecutive LOST frame breaks the keyframe graph; each tracked keyframe
    # after it searches the keyframes from before the gap (loop-closure votes + verification,
    # due reloc_latency frames later) until one re-anchors the new segment; meanwhile the published
    # pose is None and the state RELOCALIZING (oracle/numpy_loop.py LoopPolicy).  0 = off.  Needs
    # the keyframe database of loop closure.
    reloc_after_lost: int = 3
    reloc_latency: int = 5
    # input kind: RGB-D (BASELINE configs[4]) = per source a colour camera (cam_idx 0, BGR) and a
    # depth image aligned to it (cam_idx 1, u16 mm); depth replaces stereo matching
    rgbd: bool = False
    # RGB-D dense mapping: depth integrated into a dense TSDF volume on the
    # device with the tracked poses; nvblox's parameters and defaults (thor_nvblox.launch.py:26-36).
    # The reference's interface is a list of cameras (config/slam_config.yaml:61-68 nvblox_cameras,
    # of which it ships camera_0 enabled and a second one commented in; scripts/run_pipeline.py:
    # 371-392 publishes every listed camera; launch/thor_nvblox.launch.py:23 num_cameras).  Here the
    # default maps pair 0 on pair 0's own pose; dense_cameras below maps a list of them.
    dense_map: bool = False
    # the rig's cameras that feed the dense map (thor_slam_amd/dense_rig.py): () = pair 0 alone on
    # its own chained pose; "all", or a tuple of pair indices and / or source names (the reference's
    # nvblox_cameras entries, matched against CameraConfig.source_name) = those pairs' left (RGB-D:
    # colour) cameras, every frame of them in one launch, on the rig's BODY pose (the one the
    # published pose, local BA and loop closure use).  Needs dense_map, a rig of several pairs and
    # one device; resolved to ascending pair indices at initialize.
    dense_cameras: tuple | str = ()
    voxel_size: float = 0.05
    tsdf_integrator_max_integration_distance_m: float = 10.0
    tsdf_integrator_truncation_distance_vox: float = 4.0
    tsdf_max_weight: float = 100.0
    # nvblox's colour layer: the RGB image averaged into the voxels near the surface (mesh colours)
    dense_color: bool = True
    # the volume, axis-aligned in the tracking world (rectified camera of the first frame, RDF:
    # x right, y down, z forward): corner (m) and voxel counts (x, y, z); 10 x 4 x 11 m by default
    tsdf_origin: tuple = (-5.0, -2.0, -1.0)
    tsdf_dims: tuple = (200, 80, 220)
    # the rolling window (thor_slam_amd/dense_follow.py): the volume keeps its size and follows the
    # camera in whole voxels, decided on the device once per integrated batch: when the camera's
    # voxel is more than dense_follow_margin voxels from dense_follow_anchor on an axis, the window
    # moves by a multiple of dense_follow_step voxels (1 <= step <= margin); what leaves is dropped.
    # Anchor None = the voxel of the tracking world's origin in the configured volume, so the layout
    # of tsdf_origin / tsdf_dims around the camera is kept.  Needs dense_map and one device.
    dense_follow: bool = False
    dense_follow_margin: int = 32
    dense_follow_step: int = 16
    dense_follow_anchor: tuple | None = None
    # the brick store behind the window (thor_slam_amd/dense_store.py): what leaves the window is kept
    # on the device in a pool of dense_store_bricks 8 x 8 x 8 bricks (14,336 B each with every layer
    # on: 65,536 bricks are about 0.9 GB, about 0.27 GB for tsdf + weight) and comes back when the
    # window returns; get_dense_store reads it.  Needs dense_follow and one device.
    dense_store: bool = False
    dense_store_bricks: int = 65536
    # dense-map outputs (get_mesh / get_esdf / get_esdf_slice; thor_slam_amd/dense.py): nvblox's
    # mesh / ESDF integrator parameters (its defaults: min weight 1e-4, ESDF max distance 2 m, site
    # distance 1 voxel) and the 2-D slice's height band (y down: metres in the tracking world)
    mesh_integrator_min_weight: float = 1e-4
    esdf_integrator_min_weight: float = 1e-4
    esdf_integrator_max_distance_m: float = 2.0
    esdf_integrator_max_site_distance_vox: float = 1.0
    esdf_slice_min_height: float = -0.5
    esdf_slice_max_height: float = 0.5
    # the dense map seen from a pose (get_dense_view; thor_slam_amd/dense_render.py): a ray steps by
    # dense_view_step_scale (in (0, 1]) times the distance the volume reports, at least one voxel,
    # out to dense_view_max_distance_m (None = tsdf_integrator_max_integration_distance_m); a sample
    # is observed from mesh_integrator_min_weight on, as the mesh's cubes are
    dense_view_step_scale: float = 0.5
    dense_view_max_distance_m: float | None = None
    # dense frame-to-model alignment (thor_slam_amd/dense_align.py): before a batch's depth of pair 0
    # goes into the volume, every frame is aligned to the ray-cast map by projective point-to-plane
    # ICP from its tracked pose, and integrated on the aligned pose (on the tracked pose when the
    # alignment fails or the correction exceeds the limits).  Published poses are not changed.
    # dense_align_max_distance_m None = two voxels.  Needs dense_map, pair 0 alone and one device.
    dense_align: bool = False
    dense_align_iterations: int = 10
    dense_align_max_distance_m: float | None = None
    dense_align_min_inliers: int = 200
    dense_align_max_translation_m: float = 0.1
    dense_align_max_rotation_rad: float = 0.1
    # the dense map kept consistent with loop closure and relocalisation (thor_slam_amd/dense_loop.py):
    # the map takes the frames that have a pose-graph node (g % loop_kf_interval == 0), on the pose
    # the loop correction gives them, and keeps their depth in a ring of dense_loop_capacity frames on
    # the device (512 KB each at 640 x 400); when the nodes' poses change, every archived frame whose
    # pose moved by more than dense_loop_min_translation_m (None = half a voxel) or
    # dense_loop_min_rotation_rad is taken out of the volume and integrated again at its new pose.
    # Published poses are not changed.  Exact only below tsdf_max_weight observations per voxel.
    # Needs dense_map, enable_loop_closure and one device; colour, dense_cameras, dense_follow and
    # dense_align are refused.
    dense_loop: bool = False
    dense_loop_capacity: int = 1024
    dense_loop_min_translation_m: float | None = None
    dense_loop_min_rotation_rad: float = 0.005
    # dynamic objects kept out of the dense map (thor_slam_amd/dense_dynamic.py): depth of pair 0 that
    # lands in voxels the map has seen empty (weight >= dense_dynamic_min_weight, tsdf >=
    # dense_dynamic_free_fraction of the truncation distance) is masked, the mask opened by
    # dense_dynamic_open_px and dilated by dense_dynamic_dilate_px pixels, and the depth is integrated
    # without the masked pixels.  Needs dense_map and one device; dense_follow is allowed;
    # dense_cameras, dense_align, dense_loop and colour are refused.
    dense_dynamic: bool = False
    dense_dynamic_min_weight: float = 5.0
    dense_dynamic_free_fraction: float = 0.75
    dense_dynamic_open_px: int = 1
    dense_dynamic_dilate_px: int = 2
    # masked objects that come to rest enter the map (thor_slam_amd/dense_freespace.py): a voxel that
    # dense_dynamic_settle_frames consecutive frames saw within dense_dynamic_band_vox voxels of a
    # surface is no longer masked, from the next batch on; a frame that sees it free again takes the
    # release back.  0 = off (a masked object stays masked for ever).  Needs dense_dynamic.
    dense_dynamic_settle_frames: int = 0
    dense_dynamic_band_vox: float = 1.5
    # dense stereo depth (thor_slam_amd/stereo_depth.py): on a stereo rig, pair 0's depth image is
    # computed on the device from the rectified images (candidate disparities 0 .. max_disparity - 1)
    # and feeds dense_map as an RGB-D camera's depth does (no colour layer: the images are gray, so
    # dense_color is ignored).  Frames g with g % stereo_depth_interval == 0 are matched and integrated.
    stereo_depth: bool = False
    stereo_depth_uniqueness: int = 10   # percent: best cost <= (100 - u) % of the best non-neighbour
    stereo_depth_lr_tol: int = 1        # px, left-right consistency
    stereo_depth_interval: int = 1
    # semi-global aggregation over four paths between the box sums and the winners (rule 3a of
    # thor_slam_amd/stereo_depth.py): fills weakly textured surfaces; penalties in units of the
    # aggregated cost, 0 <= p1 <= p2 <= 2400
    stereo_depth_sgm: bool = False
    stereo_depth_p1: int = 100
    stereo_depth_p2: int = 1200
    # post-filters of the disparity map (rules 9 and 10 of thor_slam_amd/stereo_depth.py), off at 0:
    # the lower median of a 3 / 5 / 7 window's valid values, then 4-connected components of at most
    # stereo_depth_speckle_size pixels (neighbours within stereo_depth_speckle_range / 32 px) removed
    stereo_depth_median: int = 0
    stereo_depth_speckle_size: int = 0
    stereo_depth_speckle_range: int = 32
    # colour for a stereo rig's dense map (thor_slam_amd/depth_register.py): the source's colour
    # camera (HipSlamEngine.set_color_camera / push_color, out of band as the reference's RGB-D
    # stream) is registered to pair 0's stereo depth (with dense_cameras: to every selected pair
    # that has a colour camera) and feeds the colour layer, with a mask where a nearer surface hides
    # a depth pixel from the colour camera.  stereo_color_tol_m: how far behind the nearest surface a
    # pixel still counts as seen (None = one voxel).  A colour image further than
    # stereo_color_max_dt seconds from its frame (the reference's rgbd_sync_threshold_ms = 50), or
    # none, leaves the colour layer alone for that frame.  Needs stereo_depth and dense_map.
    stereo_color: bool = False
    stereo_color_tol_m: float | None = None
    stereo_color_max_dt: float = 0.05
    # pipeline
    batch_size: int = 1             # frames per submission
    sync: bool = False              # wait for every batch before process_frames returns (latency mode)
    # one camera stream per GPU from one process (the rig cuVSLAM's multicam mode
    # takes, launch/thor_visual_slam.launch.py:49,81): the rig's cameras sharded over these devices,
    # rank r on devices[r] (empty = the engine's one device, unsharded).  shard_transport "rccl" =
    # an RCCL clique over the devices (one per rank), "copy" = device copies (ranks may share a device)
    devices: tuple = ()
    shard_transport: str = "rccl"

    def dense_align_params(self) -> dict:
        """The rule's parameters (thor_slam_amd/dense_align.py) that ``dense_align`` runs with: the
        model view as ``get_dense_view`` renders it, out to the integration distance."""
        gate = self.dense_align_max_distance_m
        return {**ALIGN_DEFAULTS, "iterations": self.dense_align_iterations, "min_inliers": self.dense_align_min_inliers,
                "max_distance": 2.0 * self.voxel_size if gate is None else gate,
                "min_weight": self.mesh_integrator_min_weight, "max_depth": self.tsdf_integrator_max_integration_distance_m,
                "step_scale": self.dense_view_step_scale, "max_translation": self.dense_align_max_translation_m,
                "max_rotation": self.dense_align_max_rotation_rad}

    def dense_dynamic_params(self) -> dict:
        """The rule's parameters (thor_slam_amd/dense_dynamic.py) that ``dense_dynamic`` runs with."""
        return {"min_free_weight": self.dense_dynamic_min_weight, "free_fraction": self.dense_dynamic_free_fraction,
                "open_radius": self.dense_dynamic_open_px, "dilate_radius": self.dense_dynamic_dilate_px}

    def validate(self) -> None:
        if not 1 <= self.n_levels <= MAX_LEVELS:
            raise ValueError(f"n_levels must be in [1, {MAX_LEVELS}]")
        if not 1 <= self.n_features <= MAX_FEATURES:
            raise ValueError(f"n_features must be in [1, {MAX_FEATURES}]")
        if not 1 <= self.ransac_hypotheses <= MAX_HYPOTHESES:
            raise ValueError(f"ransac_hypotheses must be in [1, {MAX_HYPOTHESES}]")
        if self.edge_margin < 19:
            raise ValueError("edge_margin must be >= 19 (orientation radius 15, rotated BRIEF radius 19)")
        if not 0 <= self.fast_threshold <= 254:
            raise ValueError("fast_threshold must be in [0, 254]")
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if self.imu_accel and self.imu_fusion is False:
            raise ValueError("imu_accel needs IMU fusion (imu_fusion True or None)")
        if self.stereo_depth:
            if self.rgbd:
                raise ValueError("stereo_depth is for stereo rigs (rgbd=True already has depth)")
            if self.devices:
                raise ValueError("stereo_depth does not run on a sharded rig (devices)")
        check_stereo_depth_params(0, self.stereo_depth_uniqueness, self.stereo_depth_lr_tol)
        if self.stereo_depth_interval < 1:
            raise ValueError("stereo_depth_interval must be >= 1")
        check_stereo_depth_sgm_params(self.stereo_depth_p1, self.stereo_depth_p2)
        if self.stereo_depth_sgm and not self.stereo_depth:
            raise ValueError("stereo_depth_sgm needs stereo_depth=True")
        check_stereo_depth_filter_params(self.stereo_depth_median, self.stereo_depth_speckle_size, self.stereo_depth_speckle_range)
        if (self.stereo_depth_median or self.stereo_depth_speckle_size) and not self.stereo_depth:
            raise ValueError("stereo_depth_median / stereo_depth_speckle_size need stereo_depth=True")
        if self.stereo_color:
            if not (self.stereo_depth and self.dense_map):
                raise ValueError("stereo_color needs stereo_depth=True and dense_map=True")
            if self.rgbd:
                raise ValueError("stereo_color is for stereo rigs (rgbd=True already has colour)")
            if self.devices:
                raise ValueError("stereo_color does not run on a sharded rig (devices)")
            if self.dense_align:
                raise ValueError("stereo_color does not run with dense_align: aligned integration of coloured "
                                 "stereo depth is not built")
            if self.stereo_color_tol_m is not None and not (
                    isinstance(self.stereo_color_tol_m, (int, float)) and 0 <= self.stereo_color_tol_m <= 65.535):
                raise ValueError("stereo_color_tol_m must be None or a distance in [0, 65.535] m")
            if not (isinstance(self.stereo_color_max_dt, (int, float)) and self.stereo_color_max_dt >= 0):
                raise ValueError("stereo_color_max_dt must be >= 0")
        if self.dense_map:
            if not (self.rgbd or self.stereo_depth):
                raise ValueError("dense_map needs depth: rgbd=True (depth input) or stereo_depth=True (stereo rig)")
            if not (self.voxel_size > 0 and self.tsdf_integrator_max_integration_distance_m > 0
                    and self.tsdf_integrator_truncation_distance_vox > 0 and self.tsdf_max_weight >= 1):
                raise ValueError("voxel_size, integration distance, truncation must be > 0, max weight >= 1")
            if len(self.tsdf_dims) != 3 or min(self.tsdf_dims) < 1 or len(self.tsdf_origin) != 3:
                raise ValueError("tsdf_dims must be 3 positive voxel counts, tsdf_origin 3 coordinates")
        if not (isinstance(self.dense_view_step_scale, (int, float)) and 0 < self.dense_view_step_scale <= 1):
            raise ValueError("dense_view_step_scale must be in (0, 1]")
        if self.dense_view_max_distance_m is not None and not (
                isinstance(self.dense_view_max_distance_m, (int, float)) and 0 < self.dense_view_max_distance_m < float("inf")):
            raise ValueError("dense_view_max_distance_m must be None or a finite distance > 0")
        if isinstance(self.dense_cameras, str):
            if self.dense_cameras != "all":
                raise DenseCamerasError("dense_cameras must be (), 'all' or a tuple of pair indices / source names")
        elif len(set(self.dense_cameras)) != len(tuple(self.dense_cameras)):
            raise DenseCamerasError("dense_cameras names a camera twice")
        if self.dense_cameras:
            if not self.dense_map:
                raise DenseCamerasError("dense_cameras needs dense_map=True")
            if self.devices:
                # rank 0 holds only its own cameras' records (and pair 0's pose, not the body's)
                raise DenseCamerasError("dense_cameras does not run on a sharded rig (devices)")
        if self.dense_follow:
            if not self.dense_map:
                raise ValueError("dense_follow needs dense_map=True")
            if self.devices:
                # the camera-sharded RGB-D map lives on rank 0, behind the shard driver
                raise ValueError("dense_follow does not run on a sharded rig (devices)")
            check_follow_params(self.dense_follow_margin, self.dense_follow_step, self.dense_follow_anchor)
        if self.dense_store:
            if not self.dense_follow:
                raise ValueError("dense_store needs dense_follow=True (it keeps what leaves the rolling window)")
            if self.devices:
                raise ValueError("dense_store does not run on a sharded rig (devices)")
            check_store_params(self.dense_store_bricks)
        if self.dense_align:
            if not self.dense_map:
                raise ValueError("dense_align needs dense_map=True")
            if self.dense_cameras:
                raise ValueError("dense_align does not run with dense_cameras (it aligns pair 0's depth on pair 0's pose)")
            if self.devices:
                raise ValueError("dense_align does not run on a sharded rig (devices)")
            check_align_params(**self.dense_align_params(), max_frames=1)
        if self.dense_loop:
            if not self.dense_map:
                raise ValueError("dense_loop needs dense_map=True")
            if not self.enable_loop_closure:
                raise ValueError("dense_loop needs enable_loop_closure=True (it follows the pose graph's corrections)")
            if self.devices:
                raise ValueError("dense_loop does not run on a sharded rig (devices)")
            if self.dense_follow:
                raise ValueError("dense_loop does not run with dense_follow: a frame that left the window cannot be moved")
            if self.dense_align:
                raise ValueError("dense_loop does not run with dense_align: the aligned poses have no pose-graph node")
            if self.dense_cameras:
                raise ValueError("dense_loop does not run with dense_cameras: the archive holds one camera")
            if (self.dense_color and self.rgbd) or self.stereo_color:
                raise ValueError("dense_loop needs dense_color=False and stereo_color=False: colour is not moved yet")
            if self.stereo_depth and self.loop_kf_interval % self.stereo_depth_interval != 0:
                raise ValueError("dense_loop: stereo_depth_interval must divide loop_kf_interval (the node frames are matched)")
            check_loop_params(self.dense_loop_capacity, self.dense_loop_min_translation_m, self.dense_loop_min_rotation_rad)
        if self.dense_dynamic:
            if not self.dense_map:
                raise ValueError("dense_dynamic needs dense_map=True")
            if self.devices:
                raise ValueError("dense_dynamic does not run on a sharded rig (devices)")
            if self.dense_cameras:
                raise ValueError("dense_dynamic does not run with dense_cameras (it masks pair 0's depth on pair 0's pose)")
            if self.dense_align:
                raise ValueError("dense_dynamic does not run with dense_align: aligned integration of filtered depth is not built")
            if self.dense_loop:
                raise ValueError("dense_dynamic does not run with dense_loop: the archive would hold the unfiltered frames")
            if (self.dense_color and self.rgbd) or self.stereo_color:
                raise ValueError("dense_dynamic needs dense_color=False and stereo_color=False: the filtered depth is on "
                                 "the rectified grid, the colour is not")
            check_dynamic_params(**self.dense_dynamic_params(), max_frames=1)
        if isinstance(self.dense_dynamic_settle_frames, bool) or not isinstance(self.dense_dynamic_settle_frames, int):
            raise ValueError("dense_dynamic_settle_frames must be an integer (0 = off)")
        if self.dense_dynamic_settle_frames != 0:
            if not self.dense_dynamic:
                raise ValueError("dense_dynamic_settle_frames needs dense_dynamic=True")
            check_freespace_params(self.dense_dynamic_settle_frames, self.dense_dynamic_band_vox,
                                   self.tsdf_integrator_truncation_distance_vox)
        if not (self.ba_window == 0 or 2 <= self.ba_window <= 10):
            raise ValueError("ba_window must be 0 (off) or in [2, 10]")
        if self.ba_kf_interval < 1 or self.ba_iters < 1:
            raise ValueError("ba_kf_interval and ba_iters must be >= 1")
        if not (1 <= self.loop_max_keyframes <= 1024 and 1 <= self.loop_signature <= 256 and self.loop_kf_interval >= 1):
            raise ValueError("loop_max_keyframes must be in [1, 1024], loop_signature in [1, 256], loop_kf_interval >= 1")
        if self.loop_latency < 0 or self.imu_prior_lag < 0 or self.loop_cooldown < 0:
            raise ValueError("loop_latency, loop_cooldown and imu_prior_lag must be >= 0")
        if self.reloc_after_lost < 0 or self.reloc_latency < 0:
            raise ValueError("reloc_after_lost and reloc_latency must be >= 0")
        if self.devices:
            # local BA runs on rank 0 (state gather of a stereo rig); a camera-sharded RGB-D rig keeps
            # the TSDF on rank 0 (pair 0 is rank 0's camera) and has no local BA or loop closure
            if self.rgbd and self.ba_window:
                raise ValueError("a camera-sharded RGB-D rig (devices) runs without local BA")
            if self.shard_transport not in ("rccl", "copy"):
                raise ValueError("shard_transport must be 'rccl' or 'copy'")
        if not 0 <= self.max_hamming <= 253:
            raise ValueError("max_hamming must be in [0, 253] (the mutual check keeps distances as bytes)")


def level_shapes(width: int, height: int, n_levels: int) -> list[tuple[int, int]]:
    """(W_l, H_l) of every pyramid level: W_{l+1} = W_l >> 1, H_{l+1} = H_l >> 1."""
    out = [(width, height)]
    for _ in range(1, n_levels):
        w, h = out[-1]
        out.append((w >> 1, h >> 1))
    return out


def level_quotas(n_features: int, n_levels: int) -> list[int]:
    """Per-level keypoint budget proportional to level area (4^-l); level 0 takes the remainder."""
    total = sum(4.0 ** -l for l in range(n_levels))
    quotas = [int(n_features * (4.0 ** -l) / total) for l in range(n_levels)]
    quotas[0] = n_features - sum(quotas[1:])
    return quotas
