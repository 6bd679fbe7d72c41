"""``HipSlamEngine`` — the MI355X back end behind the reference ``SlamEngine`` interface.

Drop-in replacement for ``IsaacRosAdapter`` (``thor_slam/slam/adapters/isaac_ros.py:59-458``):

* construction ``HipSlamEngine(num_cameras=N)`` like ``IsaacRosAdapter(num_cameras)``
  (``scripts/run_slam.py:299``);
* ``initialize`` extracts the flat camera list exactly like ``_extract_cameras`` (isaac_ros.py:
  138-157), pairs ``cam_idx`` 0/1 of a source into stereo pairs (the rule of isaac_ros.py:393),
  builds the rectification that cuVSLAM performs internally (``rectified_images:=false``,
  Makefile:80) and allocates the device workspace;
* ``process_frames`` raises ``RuntimeError("Not initialized")`` before ``initialize``
  (isaac_ros.py:329-330), skips cameras whose source or ``cam_idx`` is absent (:337-341),
  converts 3-channel BGR frames to gray, and returns the newest pose (``None`` when tracking is
  lost, per interface.py:197-199);
* ``reset`` -> INITIALIZING (:438-442), ``shutdown`` -> NOT_INITIALIZED (:444-450).

Poses are world_T_base (base_link of the rig; world = base_link at the first frame), obtained by
conjugating the tracked rectified-left-camera motion with base_T_camera from the calibration.
With local BA on (``ba_window > 0``, SURVEY.md §8a A8, one stereo pair) a frame's pose is the
front-end pose carried by the correction of the newest keyframe at or before it that is still in
the window, ``W_ba(kf) inv(W_fe(kf)) W_fe(g)`` (the oldest window keyframe's when the batch has
already evicted it), and ``get_map`` returns the keyframes (BA estimates) and the window's
landmarks.  With several pairs the keyframes of all pairs form ONE window of body poses (the
rig-level solve, ``handle.ba_read(n_pairs)``; each pair keeps its landmarks, ``ba_read(p)``): the
published pose is the rig's front end carried by the body correction ``B_ba(kf) inv(B_fe(kf))``,
and ``get_map`` returns the body keyframes and every pair's landmarks.
``confidence`` follows isaac_ros.py:312.  With ``batch_size > 1`` frames are staged and the
batch runs on the GPU when full (or on ``flush``).  Submission is asynchronous
(``tslam_submit_host``: pinned double-buffered staging, the batch's H2D copy and kernels on the
handle's own streams, results copied back into pinned slots) and completed batches are
published by non-blocking polls, so the host prepares batch s+1 while the device runs batch s;
the returned pose is the latest completed one, as the reference allows (its pose lags the
published frame, isaac_ros.py:429-430).  Local BA, loop closure and the dense map read device
state per batch, so with those on every batch is waited for before the next one is staged.

The engine itself stages, submits and publishes.  Each further concern is a collaborator with its own
state and ``reset()``:

* ``slam/_loop.py``: the keyframe pose graph and its two loop-closure drivers (``_loop``);
* ``slam/_imu_link.py``: the IMU filter's motion priors, BA factors and updates (``_imu_link``; the
  filter itself is ``_imu``);
* ``slam/_dense.py``: the dense TSDF map of ``dense_map`` and its colour cameras (``_dense``);
* ``slam/_shard.py``: the rig sharded one camera stream per GPU, ``devices`` (``_shard``).
"""

from __future__ import annotations

import logging
import threading

import numpy as np
from scipy.spatial.transform import Rotation

from .._lib import POSE_INIT, POSE_LOST, POSE_OK, Handle
from ..calib import (StereoRectification, confidence_from_covariance, extract_cameras, rgbd_pairs, rgbd_undistort,
                     stereo_pairs, stereo_rectify)
from ..camera.rig import RigCalibration
from ..dense_rig import DenseCamerasError, resolve_dense_cameras
from ..camera.types import SynchronizedFrameSet
from ..imu import ImuNoise, ImuPropagator
from ..params import HipSlamConfig
from ..rgbd import pack_rgbd
from ._dense import DenseMap
from ._imu_link import _ImuLink
from ._loop import _AsyncLoop, _LoopGraph, _SyncLoop
from ._se3 import _invert, _quat_xyzw, adjoint, bgr_to_gray
from ._shard import _ShardedRig
from .interface import CameraConfig, MapPoint, SlamConfig, SlamEngine, SlamMap, SlamPose, TrackingState

logger = logging.getLogger(__name__)


class HipSlamEngine(SlamEngine):
    """Stereo visual odometry front end (detect -> match -> pose) running on one MI355X."""

    def __init__(self, num_cameras: int = 2, config: HipSlamConfig | None = None, device: int = 0) -> None:
        self._num_cameras = num_cameras
        self._config = config or HipSlamConfig(num_cameras=num_cameras)
        self._device = device
        self._state = TrackingState.NOT_INITIALIZED
        self._cameras: list[CameraConfig] = []
        self._pairs: list[tuple[int, int]] = []
        self._rects: list[StereoRectification] = []
        self._handle: Handle | None = None
        self._base_T_rect: np.ndarray | None = None
        self._latest_pose: SlamPose | None = None
        self._pose_lock = threading.Lock()
        # the map state _publish grows (BA keyframes, landmarks, loop graph) against readers on other
        # threads (get_map / save_map while process_frames runs; the reference adapter's locks,
        # isaac_ros.py:82,314,429)
        self._map_lock = threading.RLock()
        self._frame_count = 0
        self._staged: list[tuple[np.ndarray, float]] = []
        self._staged_imu: list[tuple | None] = []    # (gyro, accel) per staged frame
        self._imu: ImuPropagator | None = None       # IMU filter (gyro bias; accelerometer leg with imu_accel)
        self._imu_link: _ImuLink | None = None       # its coupling to the batches (set up with the filter)
        self._prev_stamp: float | None = None      # timestamp of the last submitted frame (IMU dt)
        self._torch = None
        self._dev_images = None
        self._host_images = None
        self._keyframe_poses: list[SlamPose] = []
        self._fe_at: dict[int, np.ndarray] = {}      # front-end rect world_T_cam of BA keyframes
        self._kf_final: dict[int, np.ndarray] = {}   # last BA estimate (rect world_T_cam) per keyframe
        self._kf_stamp: dict[int, float] = {}
        self._ba_window: dict | None = None
        self._ba_pairs: list[dict] = []
        self._map_points: dict[int, tuple] = {}   # global landmark id -> (xyz rect-0 frame, desc, observations)
        self._map_offset = np.eye(4)              # map world <- session world, set by relocalize()
        self._map_loaded = False
        self._loop: _LoopGraph | None = None     # set up by initialize() when loop closure is on
        self._in_flight = 0                       # batches submitted, not yet published
        self._shard: _ShardedRig | None = None    # sharded rig (config.devices): handles, group, inputs
        self._dense: DenseMap | None = None       # the dense map (config.dense_map)
        self._dense_pairs: tuple = ()             # config.dense_cameras resolved (() = pair 0 on its own pose)

    # ------------------------------------------------------------------------------------------
    def initialize(self, calibration: RigCalibration, config: SlamConfig | None = None) -> None:
        if isinstance(config, HipSlamConfig):
            self._config = config
        cfg = self._config
        try:
            cfg.validate()
            self._cameras = extract_cameras(calibration, self._num_cameras)
            if len(self._cameras) < self._num_cameras:
                logger.warning("Calibration has %d cameras, expected %d", len(self._cameras), self._num_cameras)
            if cfg.rgbd:   # per source: colour camera (cam_idx 0) + aligned depth (cam_idx 1)
                self._pairs = rgbd_pairs(self._cameras)
                if not self._pairs:
                    raise RuntimeError("HipSlamEngine(rgbd) needs an RGB-D source (colour cam_idx 0, depth cam_idx 1)")
                self._rects = [rgbd_undistort(self._cameras[l]) for l, _ in self._pairs]
            else:
                self._pairs = stereo_pairs(self._cameras)
                if not self._pairs:
                    raise RuntimeError("HipSlamEngine needs at least one stereo source (cam_idx 0 and 1)")
                self._rects = [stereo_rectify(self._cameras[l], self._cameras[r]) for l, r in self._pairs]
            # the cameras of the dense map (config.dense_cameras): ascending pair indices
            self._dense_pairs = resolve_dense_cameras(cfg.dense_cameras, [self._cameras[l].source_name for l, _ in self._pairs])
            import torch  # PyTorch is the device-memory / stream plumbing only

            if not torch.cuda.is_available():
                raise RuntimeError("no ROCm device visible: the MI355X back end has no CPU fallback")
            self._torch = torch
            self._base_T_rects = [self._cameras[l].extrinsics.to_4x4_matrix() @ r.left_optical_T_rect()
                                  for (l, _), r in zip(self._pairs, self._rects)]
            self._base_T_rect = self._base_T_rects[0]
            self._bt_inv = _invert(self._base_T_rect)        # cached for the per-frame publish path
            self._bt_ad = adjoint(self._base_T_rect)
            rect0 = self._rects[0]
            if cfg.rgbd:   # one [BGR | u16 depth] record of 5*H*W bytes per camera
                shape = (cfg.batch_size, len(self._pairs), 5 * rect0.height * rect0.width)
            else:
                shape = (cfg.batch_size, 2 * len(self._pairs), rect0.height, rect0.width)
            if cfg.devices:
                self._shard = _ShardedRig(torch, cfg, self._rects, self._base_T_rects, shape)
                self._handle = self._shard.handles[0]   # every rank ends a batch with the whole rig's poses; rank 0 has the rest
            else:
                self._handle = Handle(self._rects, cfg, max_batch=cfg.batch_size, device=self._device)
                self._dev_images = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{self._device}")
                self._host_images = torch.empty(shape, dtype=torch.uint8).pin_memory()
                if len(self._pairs) > 1:   # the rig's body motion, on the device from all pairs
                    self._handle.set_rig(self._base_T_rects)
            imu = getattr(calibration, "imu_extrinsics", None)   # world(base)_T_imu, RDF-converted by the caller
            base_T_imu = imu.to_4x4_matrix() if imu is not None else np.eye(4)
            self._imu = self._imu_link = None
            # the reference fuses the IMU whenever it has one (enable_imu_fusion:=true, Makefile:81)
            fusion = cfg.imu_fusion if cfg.imu_fusion is not None else imu is not None
            if fusion:
                accel = cfg.imu_accel if cfg.imu_accel is not None else True
                noise = ImuNoise(cfg.gyroscope_noise_density, cfg.gyroscope_random_walk, cfg.accelerometer_noise_density,
                                 cfg.accelerometer_random_walk, cfg.imu_rot_floor, cfg.imu_trans_floor,
                                 ba0_sigma=cfg.imu_accel_bias_sigma, bg0_sigma=cfg.imu_gyro_bias_sigma,
                                 vis_rot_floor=cfg.imu_vis_rot_floor)
                rect_T_imu = _invert(self._base_T_rect) @ base_T_imu   # the IMU in pair 0's rectified-left camera
                self._imu = ImuPropagator(rect_T_imu[:3, :3], noise, lever=rect_T_imu[:3, 3], accel=accel)
                self._imu_link = _ImuLink(self._imu, cfg, self._handle, self._base_T_rects, base_T_imu,
                                          self._set_motion_prior, self._publish_next)
            self._dense = None
            if cfg.dense_map:
                self._dense = DenseMap(cfg, self._handle, self._rects, len(self._pairs), self._dense_pairs, torch, self._device)
                self._dense.init_handle()
            self._loop = None
            if cfg.enable_loop_closure and cfg.devices and cfg.rgbd:
                # rank 0's ring holds only its own cameras' features (no state gather): no rig-wide
                # place recognition
                logger.warning("loop closure is off on a camera-sharded RGB-D rig")
            elif cfg.enable_loop_closure:   # P database entries per keyframe, keyframe-major (slam/_loop.py)
                cap = cfg.loop_max_keyframes * len(self._pairs)
                if cap > 1 << 16:
                    raise ValueError(f"loop_max_keyframes * pairs = {cap} exceeds the 65536-entry database")
                self._handle.loop_init(cap, cfg.loop_signature)
                kind = _SyncLoop
                if self._shard is None:   # the submit path stores the keyframes; searches run as loop jobs
                    self._handle.loop_auto(cfg.loop_kf_interval)
                    kind = _AsyncLoop
                m = [_invert(self._base_T_rects[0]) @ e for e in self._base_T_rects]
                self._loop = kind(self._handle, cfg, len(self._pairs), m)
        except (RuntimeError, DenseCamerasError):
            raise
        except Exception as exc:  # per interface.py:187-188
            raise RuntimeError(f"HipSlamEngine initialisation failed: {exc}") from exc
        self._state = TrackingState.INITIALIZING
        logger.info("Initialized HIP SLAM with %d cameras, %d stereo pair(s)", len(self._cameras), len(self._pairs))

    # ------------------------------------------------------------------------------------------
    def _frame_images(self, frame_set: SynchronizedFrameSet, out: np.ndarray | None = None) -> np.ndarray | None:
        """The frame's input record ([2P][H][W] gray stereo, or [P][5HW] RGB-D), written into
        ``out`` (one flat row of the library's pinned staging, tslam_host_stage) when given — the
        batch then needs no stacking or staging copy — else stacked into a new array.  None when a
        camera of the rig is missing from the set."""
        imgs = []
        if self._config.rgbd:
            for c, d in self._pairs:
                cam = self._cameras[c]
                fs = frame_set.frame_sets.get(cam.source_name)
                if fs is None or max(cam.cam_idx, self._cameras[d].cam_idx) >= len(fs.frames):
                    return None
                bgr = np.asarray(fs.frames[cam.cam_idx].image)
                depth = np.asarray(fs.frames[self._cameras[d].cam_idx].image)
                if bgr.ndim == 2:
                    bgr = np.repeat(bgr[..., None], 3, axis=-1)
                if bgr.shape[:2] != (self._rects[0].height, self._rects[0].width) or depth.shape != bgr.shape[:2]:
                    raise ValueError(f"RGB-D camera {c}: colour {bgr.shape} / depth {depth.shape} do not match its calibration")
                imgs.append(pack_rgbd(bgr, depth.astype(np.uint16, copy=False)))
            return np.stack(imgs) if out is None else self._fill(out, imgs)
        for l, r in self._pairs:
            for gi in (l, r):
                cam = self._cameras[gi]
                fs = frame_set.frame_sets.get(cam.source_name)
                if fs is None or cam.cam_idx >= len(fs.frames):
                    return None
                img = bgr_to_gray(np.asarray(fs.frames[cam.cam_idx].image))
                if img.shape != (self._rects[0].height, self._rects[0].width):
                    raise ValueError(f"camera {gi} image shape {img.shape} does not match its calibration")
                imgs.append(img)
        return np.stack(imgs) if out is None else self._fill(out, imgs)

    @staticmethod
    def _fill(out: np.ndarray, imgs: list) -> np.ndarray:
        rows = out.reshape(len(imgs), -1)
        for i, im in enumerate(imgs):
            np.copyto(rows[i], np.asarray(im, dtype=np.uint8).reshape(-1))
        return out

    def process_frames(self, frame_set: SynchronizedFrameSet) -> SlamPose | None:
        if self._handle is None:
            raise RuntimeError("Not initialized")
        self._frame_count += 1
        if self._shard is None and not self._config.dense_map:   # straight into the pinned staging
            if not self._staged:
                self._stage = self._handle.host_stage()
            imgs = self._frame_images(frame_set, out=self._stage[len(self._staged)])
        else:
            imgs = self._frame_images(frame_set)
        if imgs is None:
            if self._dense is not None:
                self._dense.drop_color()
            with self._pose_lock:
                return self._latest_pose
        if self._dense is not None:   # the colour pushed for this frame counts when it is in time
            self._dense.mark_color(len(self._staged), float(frame_set.timestamp))
        self._staged.append((imgs, float(frame_set.timestamp)))
        self._staged_imu.append(self._imu_of(frame_set))
        if len(self._staged) >= self._config.batch_size:
            self._submit_staged()
        self._drain(block=False)
        if self._loop is not None and self._loop.items:
            with self._map_lock:
                self._loop.advance()   # submit / collect loop jobs without waiting
        with self._pose_lock:
            return self._latest_pose

    @property
    def _async(self) -> bool:
        """Batches may stay in flight across calls (nothing reads per-batch device state; an IMU
        filter that has seen no sample yet predicts nothing, so a rig whose calibration names an
        IMU that sends no data keeps the asynchronous path)."""
        cfg = self._config
        return (not cfg.sync and cfg.ba_window <= 0 and (self._loop is None or self._loop.asynchronous)
                and not cfg.dense_map and (self._imu is None or not self._imu.ready or cfg.imu_prior_lag > 0))

    def _submit_staged(self) -> None:
        n = len(self._staged)
        if n == 0:
            return
        stamps = [ts for _, ts in self._staged]
        if self._imu_link is not None:
            self._imu_link.priors(stamps, self._staged_imu, self._prev_stamp)
        if self._shard is not None:   # through the group driver; results are polled from rank 0's pinned slots
            ptr, stream = self._shard.submit(self._staged, n, before_submit=self._make_room)
            self._in_flight += 1
            self._staged, self._staged_imu = [], []
            self._prev_stamp = stamps[-1]
            if not self._async:
                self._drain(block=True)
            # camera-sharded RGB-D: pair 0 is rank 0's first camera, and rank 0 ends the batch with
            # every pair's chained poses (the pose records' all-gather), so the volume lives on rank
            # 0 and integrates its own input with the device poses — no extra exchange (the batch
            # was waited for: the dense map keeps the engine synchronous)
            self._integrate_depth(ptr, n, stream, cams_per_frame=self._shard.S)
            return
        if self._dense is not None:   # the TSDF reads the batch's depth records on the device
            torch = self._torch
            host = self._host_images.numpy()
            for k, (imgs, _) in enumerate(self._staged):
                host[k] = imgs
            stream = torch.cuda.current_stream(self._device)
            self._dev_images[:n].copy_(self._host_images[:n], non_blocking=True)
            self._handle.submit(self._dev_images.data_ptr(), n, stream.cuda_stream)
            self._integrate_depth(self._dev_images.data_ptr(), n, stream.cuda_stream, stamps=stamps,
                                  has_color=self._dense.take_color(n))
            self._staged, self._staged_imu = [], []
            self._prev_stamp = stamps[-1]
            self._publish(self._read(n), stamps, self._handle.frames_done - n)
            return
        imgs = self._stage[:n]   # the frames were written there as they were staged (host_stage)
        self._make_room()
        self._handle.submit_host(imgs, stamps)
        self._in_flight += 1
        self._staged, self._staged_imu = [], []
        self._prev_stamp = stamps[-1]
        if not self._async:
            self._drain(block=True)

    def _drain(self, block: bool, limit: int | None = None) -> None:
        """Publish completed batches in order (all in flight with ``block``; at most ``limit``)."""
        done = 0
        while self._in_flight > 0 and (limit is None or done < limit):
            res = self._handle.poll_batch(block=block)
            if res is None:
                return
            self._in_flight -= 1
            done += 1
            stamps = self._shard.stamps.popleft() if self._shard is not None else list(res["timestamps"])
            self._publish(res, stamps, res["first_frame"])

    def _publish_next(self) -> bool:
        """Publish the oldest batch in flight, waiting for it.  False: none is in flight."""
        if self._in_flight == 0:
            return False
        self._drain(block=True, limit=1)
        return True

    def _make_room(self) -> None:
        """Before a submit: the handle keeps two batches' results, so the older is published first."""
        if self._in_flight >= 2:
            self._drain(block=True, limit=1)

    def flush(self) -> None:
        """Run the staged frames through the GPU pipeline and publish the poses of every batch
        submitted so far (waits for the device)."""
        if self._handle is None:
            return
        self._submit_staged()
        self._drain(block=True)

    def settle(self) -> None:
        """``flush`` and complete every pending loop-closure search now (oracle LoopPolicy.finish):
        the pose graph, ``loop_closures`` and the next published poses then include them."""
        self.flush()
        if self._loop is not None and self._loop.asynchronous:
            with self._map_lock:
                self._loop.advance(until=1 << 62)
                self._dense_loop_follow()

    # -- IMU fusion -------------------------------------------------------
    @staticmethod
    def _imu_of(frame_set: SynchronizedFrameSet) -> tuple | None:
        """(gyroscope [rad/s], accelerometer [m/s^2] or None) in IMU axes of a synchronised set,
        from ``sensor_data`` (IMUData or a dict with "gyroscope" / "accelerometer"; rig.py:403-407)."""
        d = getattr(frame_set, "sensor_data", None)
        if d is None:
            return None
        get = d.get if isinstance(d, dict) else (lambda k: getattr(d, k, None))
        g, a = get("gyroscope"), get("accelerometer")
        if g is None:
            return None
        return (np.asarray(g, dtype=np.float64).reshape(3), None if a is None else np.asarray(a, dtype=np.float64).reshape(3))

    def _set_motion_prior(self, *args) -> None:
        """The batch's priors on the handle (a sharded rig: on every rank's)."""
        (self._handle if self._shard is None else self._shard).set_motion_prior(*args)

    def process_batch(self, images, timestamps: list[float] | None = None, stream=None) -> dict:
        """Throughput entry: ``images`` is a device uint8 tensor already in HBM: [n, 2P, H, W] gray
        stereo pairs, or [n, P, 5*H*W] RGB-D records (``rgbd.pack_rgbd``).  No colour images come with
        a device batch: with ``stereo_color`` its frames are integrated for their geometry only."""
        if self._handle is None:
            raise RuntimeError("Not initialized")
        if self._shard is not None:
            raise RuntimeError("process_batch takes one device's images; a sharded rig (devices) uses process_frames")
        n = int(images.shape[0])
        s = stream if stream is not None else self._torch.cuda.current_stream(self._device)
        self.flush()
        self._handle.submit(images.data_ptr(), n, s.cuda_stream)
        self._integrate_depth(images.data_ptr(), n, s.cuda_stream, stamps=timestamps)
        res = self._read(n)
        self._publish(res, timestamps or [float(i) for i in range(n)], self._handle.frames_done - n)
        return res

    # -- the dense map (slam/_dense.py) -------------------------------------
    def _integrate_depth(self, records_ptr: int, n: int, stream: int, **kw) -> None:
        """The batch's depth into the dense map, on the loop graph's current correction."""
        if self._dense is not None:
            self._dense.integrate(records_ptr, n, stream, corr=None if self._loop is None else self._loop.corr, **kw)

    def _dense_loop_follow(self) -> None:
        if self._dense is not None:
            self._dense.follow(self._loop)

    def _dense_reader(self, on: bool = True) -> DenseMap | None:
        """What every reader starts with: the dense map with all staged frames in it, or None when it
        or the reader's own option (``on``) is off.  Synchronises."""
        if self._dense is None or not on or self._handle is None:
            return None
        self.flush()
        return self._dense

    @property
    def _world_T_volume(self) -> np.ndarray:
        """The volume's frame (pair 0's rectified left camera at the first frame) in the published world."""
        return self._map_offset @ self._base_T_rect

    def _color_pair(self, pair_or_source_name) -> int:
        if isinstance(pair_or_source_name, str):
            names = [self._cameras[l].source_name for l, _ in self._pairs]
            if pair_or_source_name not in names:
                raise ValueError(f"no stereo pair of source {pair_or_source_name!r}")
            return names.index(pair_or_source_name)
        p = int(pair_or_source_name)
        if not 0 <= p < len(self._pairs):
            raise ValueError(f"pair {p} out of range")
        return p

    def set_color_camera(self, pair_or_source_name, intrinsics, left_T_color) -> None:
        """The colour camera of a stereo pair (``stereo_color``), after ``initialize`` and before
        the first frame: its ``Intrinsics`` (the reference's ``get_rgbd_intrinsics()[0]``) and its
        pose in the pair's left camera, ``left_T_color`` as ``Extrinsics`` (the inverse of
        ``get_rgbd_extrinsics()[1]``).  Only pair 0's, or with ``dense_cameras`` a selected pair's,
        feeds the map."""
        if self._handle is None:
            raise RuntimeError("Not initialized")
        if not self._config.stereo_color:
            raise RuntimeError("set_color_camera needs stereo_color=True")
        if self._frame_count or self._staged:
            raise RuntimeError("set_color_camera comes before the first frame")
        self._dense.add_color_camera(self._color_pair(pair_or_source_name), intrinsics, left_T_color)

    def push_color(self, pair_or_source_name, bgr: np.ndarray, timestamp: float) -> None:
        """The colour camera's BGR image of the frame the next ``process_frames`` call brings, into
        the pinned staging of that frame's batch slot.  An image further than
        ``stereo_color_max_dt`` from its frame's timestamp is not used."""
        p = self._color_pair(pair_or_source_name)
        if self._dense is None or p not in self._dense.color_cams:
            raise RuntimeError(f"pair {p} has no colour camera (set_color_camera)")
        self._dense.color_cams[p].push(len(self._staged), bgr, timestamp)

    def get_registered_depth(self, pair: int = 0) -> tuple | None:
        """(depth u16 [Hc][Wc] in mm in pair ``pair``'s undistorted colour camera, timestamp) of the
        newest frame whose stereo depth was registered to a colour image (``stereo_color``), or
        None.  Synchronises."""
        d = self._dense_reader(self._config.stereo_color)
        return None if d is None else d.registered_depth(int(pair))

    def get_dense_archive(self) -> dict | None:
        """The depth archive of ``dense_loop``, oldest frame first: ``frames`` i64 [n], ``world_T_cam``
        f64 [n][4][4] (the pose each frame is in the dense map with, in the volume's frame),
        ``moved_last`` and ``moved_total`` (frames moved by the last correction, and since the start
        or the last reset).  None unless ``dense_loop`` is on.  Synchronises."""
        d = self._dense_reader(self._config.dense_loop)
        return None if d is None else d.archive()

    def get_depth_image(self, pair: int = 0) -> tuple | None:
        """(depth u16 [H][W] in mm of pair ``pair``'s rectified left camera, timestamp) of the newest
        frame the dense stereo matcher processed for that pair (pair 0, or any pair of
        ``dense_cameras``), or None (``stereo_depth`` with ``dense_map`` only).  Synchronises."""
        d = self._dense_reader(self._config.stereo_depth)
        return None if d is None else d.depth_image(int(pair))

    def get_dense_alignment(self) -> dict | None:
        """The newest batch's frame-to-model alignment (``dense_align``; the rule is
        thor_slam_amd/dense_align.py): ``world_T_cam`` f64 [n][4][4], the poses the batch's depth
        was integrated with, in the volume's frame (the aligned pose where ``stats[:, 0]`` is 0, else
        the tracked pose); ``stats`` i32 [n][4] (status: 0 ok, 1 unused, 2 no model, 3 degenerate,
        4 rejected; iterations run; inliers of the first and of the last iteration); ``residuals``
        f64 [n][2] (their rms point-to-plane residuals, metres); ``normal_eq`` f64 [n][28].  None
        unless ``dense_align`` is on.  Synchronises."""
        d = self._dense_reader(self._config.dense_align)
        return None if d is None else d.alignment()

    def get_dynamic_mask(self) -> dict | None:
        """The free-space mask of the newest frame that went through it (``dense_dynamic``; the rule is
        thor_slam_amd/dense_dynamic.py): ``mask`` u8 [H][W] (1: kept out of the map), ``depth`` u16
        [H][W] in mm on pair 0's rectified grid (what was integrated: 0 under the mask), ``stats`` i32
        [4] (status: 0 ok, 1 unused; valid pixels; candidates; valid pixels under the mask) and the
        frame's ``timestamp``.  None unless ``dense_dynamic`` is on and a frame has gone through.
        Synchronises."""
        d = self._dense_reader(self._config.dense_dynamic)
        return None if d is None else d.dynamic_mask()

    def get_freespace(self) -> dict | None:
        """The free-space layer (``dense_dynamic_settle_frames``; the rule is
        thor_slam_amd/dense_freespace.py) on the volume's grid: ``run`` u16 [nz][ny][nx] (consecutive
        frames that saw a surface in the voxel) and ``settled`` bool [nz][ny][nx] (the voxel is no
        longer masked: what comes to rest there enters the map from the next batch on), with
        ``origin``, ``window_shift`` and ``world_T_volume`` as ``get_dense_map`` gives them.  None
        unless the option is on.  Synchronises."""
        d = self._dense_reader(self._config.dense_dynamic and self._config.dense_dynamic_settle_frames > 0)
        return None if d is None else d.freespace(self._world_T_volume)

    def get_dense_store(self) -> dict | None:
        """What has left the rolling window (``dense_store``; the rule is thor_slam_amd/dense_store.py):
        the store's n bricks of 8 x 8 x 8 voxels that hold a voxel, in ascending (bz, by, bx):
        ``bricks`` i32 [n][3] (bx, by, bz), ``tsdf`` / ``weight`` f32 [n][8][8][8] (z, y, x), with the
        colour layer ``color`` f32 [n][8][8][8][3] and ``color_weight``, with the free-space layer
        ``run`` / ``settled`` as ``get_freespace`` splits them; ``voxel_size``, ``origin`` (the
        configured ``tsdf_origin``: brick b's local voxel (i, j, k) is centred at
        origin + voxel_size (8 b + (i, j, k) + 0.5)), ``world_T_volume`` and ``stats`` (capacity,
        bricks allocated, bricks, voxels stored, voxels dropped, moves, words per voxel).
        ``dense_store.assemble`` joins it with ``get_dense_map`` into the whole map.  None unless the
        option is on.  Synchronises."""
        d = self._dense_reader(self._config.dense_store)
        return None if d is None else d.store(self._world_T_volume)

    def get_dense_map(self) -> dict | None:
        """The TSDF volume (nvblox-shaped): ``tsdf`` / ``weight`` f32 [nz][ny][nx] (metres of
        truncated signed distance; weight 0 = never observed), the voxel grid (``origin``,
        ``voxel_size``, voxel (i, j, k) centred at origin + voxel_size (i, j, k) + voxel_size / 2 in
        the tracking world; with ``dense_follow`` the origin of the window as it stands, ``window_shift``
        voxels from ``tsdf_origin``) and ``world_T_volume`` (4x4: that frame in the published world =
        base_link at the first frame).  None unless ``dense_map`` is on.  Synchronises."""
        d = self._dense_reader()
        return None if d is None else d.volume(self._world_T_volume)

    def get_dense_view(self, world_T_view: np.ndarray | None = None, size: tuple | None = None,
                       intrinsics: tuple | None = None) -> dict | None:
        """The dense map seen from a camera pose (ray casting on the device, k_tsdf_render.hip; the
        rule is thor_slam_amd/dense_render.py): ``depth`` f32 [H][W] (metres along the camera's z
        axis), ``depth_mm`` u16 [H][W] (what ``tsdf_integrate`` reads), ``normals`` f32 [H][W][3]
        (in the volume's frame, pointing into free space), with the colour layer ``colors`` u8
        [H][W][3] (B, G, R); all zero where the map holds no surface.  Also ``intrinsics`` (fx, fy,
        cx, cy), ``world_T_view``, and the volume's ``origin``, ``window_shift`` and
        ``world_T_volume`` as ``get_dense_map`` gives them.

        ``world_T_view``: the camera (optical frame, RDF) in the published world; None = pair 0's
        rectified left camera at the newest published pose (None is returned while there is none).
        ``size`` = (W, H) and ``intrinsics`` = (fx, fy, cx, cy): default pair 0's rectified left
        camera, whose depth fills the map; a ``size`` alone keeps that camera's field of view.
        None unless ``dense_map`` is on.  Synchronises."""
        if self._dense is not None and self._shard is not None:
            raise RuntimeError("get_dense_view does not run on a sharded rig (devices)")
        d = self._dense_reader()
        return None if d is None else d.view(self._world_T_volume, world_T_view, size, intrinsics, self._newest_view)

    def _newest_view(self) -> np.ndarray | None:
        """Pair 0's rectified left camera at the newest published pose, in the published world."""
        with self._pose_lock:
            pose = self._latest_pose
        if pose is None:
            return None
        body = np.eye(4)
        body[:3, :3] = Rotation.from_quat(pose.rotation).as_matrix()
        body[:3, 3] = pose.position
        return body @ self._base_T_rect

    def get_mesh(self, whole: bool = False) -> dict | None:
        """The surface mesh of the TSDF volume (marching cubes on the device, k_dense.hip):
        ``triangles`` f32 [n][3][3] (metres in the tracking world, facing free space), with the
        colour layer ``colors`` f32 [n][3][3] (R, G, B per vertex), and ``world_T_volume``.  None unless ``dense_map`` is on.  Synchronises.

        ``whole=True`` (``dense_store``; k_tsdf_store_mesh.hip, the rule is thor_slam_amd/dense_store.py):
        one mesh of everything the map holds, the rolling window and the brick store together, with
        no seam between them: the same keys, with ``origin`` (the configured ``tsdf_origin``, which
        the vertices are computed from: they do not depend on where the window stands) and
        ``bricks`` (the 8 x 8 x 8 store bricks visited).  Triangles come brick by brick in ascending
        (bz, by, bx).  None unless ``dense_store`` is on."""
        if whole:
            d = self._dense_reader(self._config.dense_store)
            return None if d is None else d.mesh_whole(self._world_T_volume)
        d = self._dense_reader()
        return None if d is None else d.mesh(self._world_T_volume)

    def get_esdf(self) -> dict | None:
        """The Euclidean signed distance field of the volume (k_dense.hip): ``esdf`` f32
        [nz][ny][nx] (metres, negative inside, +-esdf_integrator_max_distance_m beyond it, NaN
        unobserved) on the TSDF grid.  None unless ``dense_map`` is on.  Synchronises."""
        d = self._dense_reader()
        return None if d is None else d.esdf(self._world_T_volume)

    def get_esdf_slice(self) -> dict | None:
        """nvblox's 2-D distance map: unsigned distance f32 [nz][nx] to the nearest surface voxel of
        the height band [esdf_slice_min_height, esdf_slice_max_height) (tracking-world y), NaN
        where the band was never observed.  None unless ``dense_map`` is on.  Synchronises."""
        d = self._dense_reader()
        return None if d is None else d.esdf_slice(self._world_T_volume)

    def _read(self, n: int) -> dict:
        res = self._handle.read_poses(n)
        if len(self._pairs) > 1:
            res["rig"] = self._handle.read_rig_poses(n)
        return res

    def _body_pose(self, res: dict, k: int) -> tuple[int, np.ndarray, np.ndarray]:
        """(status, world_T_base, 6x6 body covariance) of frame k of a batch result."""
        bt = self._base_T_rect
        stats = res["stats"][k, :, 0]
        if len(self._pairs) == 1:
            status = int(stats[0])
            body = bt @ res["T_abs"][k, 0] @ self._bt_inv
            ad = self._bt_ad   # camera-frame twist -> base-frame twist (rotation and lever arm)
            cov = ad @ res["cov"][k, 0] @ ad.T if status == POSE_OK else np.zeros((6, 6))
            return status, body, cov
        # multi-pair rig: the device's generalised PnP over all pairs (k_rig_pose), already in the
        # base frame and chained (world = base_link at the first frame)
        rig = res["rig"]
        status = int(rig["stats"][k, 0])
        cov = rig["cov"][k] if status == POSE_OK else np.zeros((6, 6))
        return status, rig["T_abs"][k].copy(), cov

    def _ba_corrections(self, res: dict, n: int, g0: int):
        """Per frame of the batch: the correction W_ba(kf) inv(W_fe(kf)) (or None) — rect-left
        world_T_cam terms for one pair, world_T_body (base) terms for a rig's body window."""
        cfg = self._config
        if cfg.ba_window <= 0:
            return None
        P = len(self._pairs)
        rig = P > 1
        for k in range(n):
            if (g0 + k) % cfg.ba_kf_interval == 0:
                self._fe_at[g0 + k] = (res["rig"]["T_abs"][k] if rig else res["T_abs"][k, 0]).copy()
        win = self._handle.ba_read(P if rig else 0)
        self._ba_window = win
        self._ba_pairs = [self._handle.ba_read(q) for q in range(P)] if rig else [win]
        for q, w in enumerate(self._ba_pairs):
            self._accumulate_map(w, q)
        live = {}
        for s_, f in enumerate(win["frames"]):
            if f >= 0:
                live[int(f)] = _invert(win["T_cw"][s_])
                self._kf_final[int(f)] = live[int(f)]
        for f in [f for f in self._fe_at if f not in live and f < min(live, default=0)]:
            del self._fe_at[f]   # evicted: its final estimate is kept in _kf_final
        if not live:
            return None
        frames = sorted(live)
        out = []
        for k in range(n):
            g = g0 + k
            kf = max([f for f in frames if f <= g], default=frames[0])
            out.append(live[kf] @ _invert(self._fe_at[kf]))
        return out

    def _accumulate_map(self, win: dict, pair: int = 0) -> None:
        """Merge a window's landmarks (latest BA positions) into the persistent map by global id
        (rect-left frame of pair 0; a rig's pairs keep theirs apart: key gid * n_pairs + pair).
        ``SlamConfig.enable_mapping`` off keeps no map; ``max_map_size`` bounds it (the landmarks
        updated longest ago go first; interface.py:110-111)."""
        cfg = self._config
        if not cfg.enable_mapping:
            return
        mp = self._handle.ba_read_map(pair)
        P = len(self._pairs)
        to_rect0 = _invert(self._base_T_rect) if P > 1 else np.eye(4)   # a rig's BA world is the base frame
        occ = win["frames"] >= 0
        ids, counts = np.unique(win["lm"][occ], return_counts=True)
        keep = ids >= 0
        for i, n in zip(ids[keep], counts[keep]):
            x = to_rect0[:3, :3] @ win["X"][i] + to_rect0[:3, 3]
            key = int(mp["gid"][i]) * P + pair
            self._map_points.pop(key, None)   # re-inserted: most recently updated last
            self._map_points[key] = (x, mp["desc"][i].copy(), int(n))
        while len(self._map_points) > max(int(cfg.max_map_size), 0):
            del self._map_points[next(iter(self._map_points))]

    def _publish(self, res: dict, stamps: list[float], g0: int) -> None:
        with self._map_lock:
            self._publish_locked(res, stamps, g0)
            self._dense_loop_follow()

    def _publish_locked(self, res: dict, stamps: list[float], g0: int) -> None:
        if self._imu_link is not None:
            self._imu_link.record(res)
        latest = None
        state = self._state
        corr = self._ba_corrections(res, len(stamps), g0)
        bt, bt_inv, lp = self._base_T_rect, self._bt_inv, self._loop
        for k, ts in enumerate(stamps):
            status, body, cov = self._body_pose(res, k)
            if corr is not None and status != POSE_LOST:   # a rig's correction is in body terms
                body = corr[k] @ body if len(self._pairs) > 1 else bt @ corr[k] @ res["T_abs"][k, 0] @ bt_inv
            # oracle/numpy_loop.py LoopPolicy.step; the search at the keyframe itself skips LOST frames
            if lp is not None and (lp.asynchronous or status != POSE_LOST):
                g = g0 + k
                raw = bt_inv @ body @ bt                           # rect-left world_T_cam before loop correction
                lp.observe(g, status)
                if status == POSE_OK and g % self._config.loop_kf_interval == 0:
                    lp.node(g, raw, ts)
                lp.advance(until=g)
                body = bt @ lp.corr @ raw @ bt_inv
                if lp.reloc:   # no pose until the new segment is anchored in the map
                    state = TrackingState.RELOCALIZING
                    latest = None
                    continue
            body = self._map_offset @ body
            if status == POSE_LOST:
                state = TrackingState.LOST
                latest = None
                continue
            state = TrackingState.TRACKING if status == POSE_OK else TrackingState.INITIALIZING
            latest = SlamPose(
                position=body[:3, 3].copy(),
                rotation=_quat_xyzw(body),
                timestamp=ts,
                tracking_state=state,
                confidence=confidence_from_covariance(cov) if status == POSE_OK else 1.0,
                covariance=cov,
            )
            if status == POSE_INIT:
                self._keyframe_poses.append(latest)
            g = g0 + k
            if self._config.ba_window > 0 and g % self._config.ba_kf_interval == 0:
                self._kf_stamp[g] = ts
        with self._pose_lock:
            self._latest_pose = latest
            self._state = state
        self._last_result = res

    @property
    def loop_closures(self) -> list[tuple[int, int, int]]:
        """Verified loops so far: (older keyframe frame, newer keyframe frame, inliers)."""
        return list(self._loop.loops) if self._loop is not None else []

    @property
    def pose_graph(self) -> dict | None:
        """The keyframe pose graph: frames, world_T_cam (rect-left) per node, edges (a, b)."""
        if self._loop is None:
            return None
        lp = self._loop
        return {"frames": list(lp.frames), "T": np.array(lp.T).reshape(-1, 4, 4), "edges": list(lp.edges),
                "meas": [m.copy() for m in lp.meas], "cost": lp.cost}

    # ------------------------------------------------------------------------------------------
    def get_tracking_state(self) -> TrackingState:
        return self._state

    def get_map(self) -> SlamMap:
        """Without BA: the (re)initialisation poses.  With BA: every keyframe so far at its latest
        BA estimate (world_T_base) and the landmarks of every pair's window (world frame, with their
        observation counts).  Safe to call from another thread while process_frames runs."""
        with self._map_lock:
            return self._get_map_locked()

    def _get_map_locked(self) -> SlamMap:
        if self._loop is not None and self._loop.frames and (self._config.ba_window <= 0 or self._ba_window is None):
            bt = self._base_T_rect
            kfs = []
            for T, ts in zip(self._loop.T, self._loop.stamps):
                body = self._map_offset @ bt @ T @ _invert(bt)
                kfs.append(SlamPose(position=body[:3, 3].copy(), rotation=Rotation.from_matrix(body[:3, :3]).as_quat(),
                                    timestamp=ts, tracking_state=TrackingState.TRACKING, confidence=1.0))
            smap = SlamMap(keyframe_poses=kfs)
        elif self._config.ba_window <= 0 or self._ba_window is None:
            smap = SlamMap(keyframe_poses=list(self._keyframe_poses))
        else:
            rig = len(self._pairs) > 1   # body window: keyframes are already world_T_base, landmarks in base
            bt = np.eye(4) if rig else self._base_T_rect
            kfs = []
            for f in sorted(self._kf_final):
                body = bt @ self._kf_final[f] @ _invert(bt)
                kfs.append(SlamPose(position=body[:3, 3].copy(), rotation=Rotation.from_matrix(body[:3, :3]).as_quat(),
                                    timestamp=self._kf_stamp.get(f, float(f)), tracking_state=TrackingState.TRACKING,
                                    confidence=1.0))
            points = []
            for win in self._ba_pairs:
                occ = win["frames"] >= 0
                ids, counts = np.unique(win["lm"][occ], return_counts=True)
                keep = ids >= 0
                ids, counts = ids[keep], counts[keep]
                pts = win["X"][ids] @ bt[:3, :3].T + bt[:3, 3]
                points += [MapPoint(position=p.copy(), observations=int(c)) for p, c in zip(pts, counts)]
            # SlamConfig.enable_mapping / max_map_size (interface.py:110-111)
            points = points[:max(int(self._config.max_map_size), 0)] if self._config.enable_mapping else []
            smap = SlamMap(points=points, keyframe_poses=kfs)
        pose = self._latest_pose
        if pose is not None:
            smap.timestamp = pose.timestamp
        return smap

    # -- map persistence / relocalisation (interface.py:228-256) -----------
    def save_map(self, path: str) -> bool:
        """Write the landmarks gathered by local BA (world = base_link frame, rBRIEF descriptors,
        global ids, observation counts) and every keyframe pose to ``path`` (NumPy .npz, no
        pickles).  False when there is nothing to save (local BA off or no landmark yet)."""
        with self._map_lock:
            return self._save_map_locked(path)

    def _save_map_locked(self, path: str) -> bool:
        if not self._map_points or self._handle is None:
            return False
        bt = self._base_T_rect
        gids = np.array(sorted(self._map_points), dtype=np.int64)
        xyz = np.stack([self._map_points[g][0] for g in gids])
        desc = np.stack([self._map_points[g][1] for g in gids]).astype(np.uint32)
        obs = np.array([self._map_points[g][2] for g in gids], dtype=np.int64)
        smap = self.get_map()
        kf = np.stack([p.to_4x4_matrix() for p in smap.keyframe_poses]) if smap.keyframe_poses else np.zeros((0, 4, 4))
        with open(path, "wb") as fh:
            np.savez(fh, points=xyz @ bt[:3, :3].T + bt[:3, 3], desc=desc, gid=gids, observations=obs,
                     keyframe_world_T_base=kf, keyframe_stamps=np.array([p.timestamp for p in smap.keyframe_poses]),
                     base_T_rect=bt)
        return True

    def load_map(self, path: str) -> bool:
        """Load a map written by ``save_map`` and upload it for ``relocalize``."""
        if self._handle is None:
            raise RuntimeError("Not initialized")
        try:
            with np.load(path, allow_pickle=False) as z:
                pts, desc = np.asarray(z["points"], dtype=np.float64), np.asarray(z["desc"], dtype=np.uint32)
        except (OSError, KeyError, ValueError) as exc:
            logger.warning("load_map(%s) failed: %s", path, exc)
            return False
        if len(self._pairs) > 1:   # a rig relocalises in the base frame from every pair (tslam_relocalize_rig)
            self._handle.map_upload(pts, desc)
        else:
            inv_bt = _invert(self._base_T_rect)
            self._handle.map_upload(pts @ inv_bt[:3, :3].T + inv_bt[:3, 3], desc)   # into the rect-left frame
        self._map_loaded = True
        return True

    def relocalize(self) -> bool:
        """Pose the latest processed frame in the loaded map (descriptor matching + P3P-RANSAC on
        the device; a rig: every pair's view, joined by the rig pose, so a map any one pair saw
        relocalises it); on success the published poses continue in the map's world frame."""
        if self._handle is None:
            raise RuntimeError("Not initialized")
        if not self._map_loaded or self._handle.frames_done == 0:
            return False
        self.flush()
        if len(self._pairs) > 1:   # every pair matches the map; the rig pose solves the body
            res = self._handle.relocalize_rig(self._handle.frames_done - 1)
            if int(res["stats"][0]) != POSE_OK:
                return False
            map_pose = _invert(res["T"])                                 # map world_T_base of that frame
        else:
            res = self._handle.relocalize(self._handle.frames_done - 1)
            if int(res["stats"][0]) != POSE_OK:
                return False
            bt = self._base_T_rect
            map_pose = bt @ _invert(res["T"]) @ _invert(bt)              # map world_T_base of that frame
        with self._pose_lock:
            cur = self._latest_pose
        session = (_invert(self._map_offset) @ cur.to_4x4_matrix()) if cur is not None else np.eye(4)
        self._map_offset = map_pose @ _invert(session)
        if cur is not None:
            body = map_pose
            with self._pose_lock:
                self._latest_pose = SlamPose(position=body[:3, 3].copy(), rotation=Rotation.from_matrix(body[:3, :3]).as_quat(),
                                             timestamp=cur.timestamp, tracking_state=TrackingState.TRACKING,
                                             confidence=cur.confidence, covariance=cur.covariance)
                self._state = TrackingState.TRACKING
        return True

    def reset(self) -> None:
        self._in_flight = 0
        with self._pose_lock:
            self._latest_pose = None
        self._staged, self._staged_imu, self._prev_stamp = [], [], None
        for part in (self._imu_link, self._dense):
            if part is not None:
                part.reset()
        self._keyframe_poses = []
        self._fe_at, self._kf_final, self._kf_stamp, self._ba_window, self._ba_pairs = {}, {}, {}, None, []
        self._map_points, self._map_offset = {}, np.eye(4)
        if self._loop is not None:
            self._loop = self._loop.fresh()
        if self._shard is not None:
            self._shard.reset()
        elif self._handle is not None:
            self._handle.reset()
        self._state = TrackingState.INITIALIZING
        self._frame_count = 0

    def shutdown(self) -> None:
        if self._handle is not None and (self._staged or self._in_flight):
            try:   # the tail of the stream: staged frames run as a short last batch and are published
                self.flush()
            except RuntimeError as exc:
                logger.warning("shutdown: the last %d staged frame(s) were not tracked: %s", len(self._staged), exc)
        if self._shard is not None:
            self._shard.close()
            self._shard = None
        elif self._handle is not None:
            self._handle.close()
        self._handle = None
        self._state = TrackingState.NOT_INITIALIZED

    @property
    def frame_count(self) -> int:
        return self._frame_count

    @property
    def num_cameras(self) -> int:
        return self._num_cameras

    @property
    def handle(self) -> Handle | None:
        return self._handle

    @property
    def rectifications(self) -> list[StereoRectification]:
        return list(self._rects)
