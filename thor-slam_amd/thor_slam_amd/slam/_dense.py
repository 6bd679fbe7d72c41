"""The engine's dense map (nvblox's role in the reference pipeline,
``scripts/run_pipeline.py:218-256``): every batch's depth into a TSDF volume on the device, with the
batch's tracked poses.

The depth is pair 0's part of the RGB-D records, or on a stereo rig (``stereo_depth``) the dense
stereo matcher's (``thor_slam_amd/stereo_depth.py``) of every ``stereo_depth_interval``-th frame.
``dense_cameras`` integrates those cameras of the rig instead, every frame of them in one launch per
run (``tslam_tsdf_integrate_rig``) on the rig's body poses (``thor_slam_amd/dense_rig.py``).
``dense_follow`` lets the volume follow the camera in whole voxels, decided on the device once per
integrated batch (``thor_slam_amd/dense_follow.py``); the readers then report the window's effective
``origin`` and its ``window_shift``; with ``dense_store`` what leaves the window goes to a brick store
on the device and comes back with the window (``thor_slam_amd/dense_store.py``).  ``dense_align`` aligns a batch's depth to the map before it goes
in (``thor_slam_amd/dense_align.py``).  ``dense_loop`` keeps the map consistent with loop closure and
relocalisation (``thor_slam_amd/dense_loop.py``): the map takes the pose-graph node frames, on the
loop-corrected pose, keeps their depth in an archive on the device, and after the nodes' poses
changed the archived frames that moved are taken out of the volume and integrated again at their new
poses.  ``dense_dynamic`` keeps depth that lands in voxels the map has seen empty out of it
(``thor_slam_amd/dense_dynamic.py``): a batch's depth goes through the free-space mask, and the
filtered copy is what is integrated.  ``stereo_color`` colours a stereo rig's map from the source's
centre colour camera (``thor_slam_amd/depth_register.py``): the colour is registered to the stereo
depth on the device."""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from ..dense_freespace import split
from ..dense_store import split_words
from ..dense_render import check_render_params, scaled_intrinsics, view_in_volume
from ..depth_register import DEFAULT_MAX_SPLAT, check_register_params, color_camera, compose_color_T_rect


@dataclass
class ColorCamera:
    """A stereo pair's colour camera (``stereo_color``): pinned staging and device images per batch
    slot, per slot whether a colour image in time was pushed, and the timestamp of a pushed image
    that waits for its frame."""

    shape: tuple
    host: object
    dev: object
    has: list
    pushed: float | None = None

    def push(self, slot: int, bgr, timestamp: float) -> None:
        img = np.asarray(bgr)
        if img.shape != self.shape or img.dtype != np.uint8:
            raise ValueError(f"colour image {img.shape} {img.dtype} does not match its calibration {self.shape} uint8")
        np.copyto(self.host.numpy()[slot], img)
        self.pushed = float(timestamp)

    def mark(self, slot: int, frame_ts: float, max_dt: float) -> None:
        """The frame staged in ``slot``: the colour pushed for it counts when it is in time."""
        ts, self.pushed = self.pushed, None
        self.has[slot] = ts is not None and abs(ts - frame_ts) <= max_dt

    def take(self, n: int) -> list:
        """Which of the batch's n slots hold a colour image; their images go to the device."""
        has = list(self.has[:n])
        self.has = [False] * len(self.has)
        if any(has):
            self.dev[:n].copy_(self.host[:n], non_blocking=True)
        return has

    def reset(self) -> None:
        self.has, self.pushed = [False] * len(self.has), None


class DenseMap:
    def __init__(self, cfg, handle, rects: list, n_pairs: int, dense_pairs: tuple, torch=None, device: int = 0) -> None:
        self.cfg, self.h, self.rects, self.P = cfg, handle, rects, n_pairs
        self.dense = dense_pairs              # config.dense_cameras resolved (() = pair 0 on its own pose)
        self.torch, self.device = torch, device
        self.hw = rects[0].width * rects[0].height
        # the colour layer needs colour input: a stereo rig's images are gray, so dense_color is
        # ignored with stereo_depth, unless the rig's colour camera is used (stereo_color)
        self.color = bool((cfg.dense_color and not cfg.stereo_depth) or cfg.stereo_color)
        self.color_cams: dict = {}            # pair -> ColorCamera (add_color_camera)
        self.color_zero: dict | None = None   # what a pair without a colour camera is integrated with
        self.view_key = None                  # view()'s camera (size, intrinsics, range) on the handle
        self.reset()

    def reset(self) -> None:
        self.sd_last: dict = {}    # pair -> (slot, timestamp) of its newest stereo depth image
        self.reg_last: dict = {}   # pair -> (slot, timestamp) of its newest registered frame
        self.dyn_last: tuple | None = None   # (slot, timestamp) of the newest frame that went through the free-space mask
        self.loop_seen = 0         # dense_loop: corrections of the pose graph the map has followed
        for cc in self.color_cams.values():
            cc.reset()

    def init_handle(self) -> None:
        """The volume and the options' workspaces on the handle."""
        cfg, h = self.cfg, self.h
        if self.color:
            h.tsdf_color(True)
        h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                    cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
        if cfg.dense_follow:   # the window follows the camera (thor_slam_amd/dense_follow.py)
            h.tsdf_follow(cfg.dense_follow_anchor, cfg.dense_follow_margin, cfg.dense_follow_step)
        if cfg.dense_align:   # frame-to-model alignment before integration (thor_slam_amd/dense_align.py)
            h.tsdf_align_init(pair=0, rect=bool(cfg.stereo_depth), max_frames=cfg.batch_size, **cfg.dense_align_params())
        if cfg.dense_loop:   # the node frames' depth is kept, to follow the pose graph (thor_slam_amd/dense_loop.py)
            h.tsdf_archive_init(cfg.dense_loop_capacity, interval=cfg.loop_kf_interval, pair=0, rect=bool(cfg.stereo_depth))
        if cfg.dense_dynamic:   # depth in known free space is kept out (thor_slam_amd/dense_dynamic.py)
            h.tsdf_dynamic_init(pair=0, rect=bool(cfg.stereo_depth), max_frames=cfg.batch_size, **cfg.dense_dynamic_params())
            if cfg.dense_dynamic_settle_frames:   # masked objects that come to rest are released (thor_slam_amd/dense_freespace.py)
                h.tsdf_freespace_init(settle_frames=cfg.dense_dynamic_settle_frames, occupied_band_vox=cfg.dense_dynamic_band_vox)
        if cfg.dense_store:   # what leaves the window is kept (thor_slam_amd/dense_store.py): after every layer exists
            h.tsdf_store_init(cfg.dense_store_bricks)
        if cfg.stereo_depth:   # a stereo rig: the depth comes from the dense matcher (slots per camera)
            h.stereo_depth_init(max_frames=cfg.batch_size * max(1, len(self.dense)),
                                uniqueness=cfg.stereo_depth_uniqueness, lr_tol=cfg.stereo_depth_lr_tol)
            if cfg.stereo_depth_sgm:
                h.stereo_depth_sgm(p1=cfg.stereo_depth_p1, p2=cfg.stereo_depth_p2)
            if cfg.stereo_depth_median or cfg.stereo_depth_speckle_size:
                h.stereo_depth_filter(median=cfg.stereo_depth_median, speckle_size=cfg.stereo_depth_speckle_size,
                                      speckle_range=cfg.stereo_depth_speckle_range)

    # -- the colour camera of a stereo rig (thor_slam_amd/depth_register.py) ----------------------
    def add_color_camera(self, p: int, intrinsics, left_T_color) -> None:
        cfg, torch, r = self.cfg, self.torch, self.rects[p]
        ccam = color_camera(intrinsics)
        T = compose_color_T_rect(left_T_color.to_4x4_matrix(), r.left_optical_T_rect())
        tol = cfg.voxel_size if cfg.stereo_color_tol_m is None else cfg.stereo_color_tol_m
        tol_mm = int(math.floor(tol * 1000.0 + 0.5))
        check_register_params(int(r.width), int(r.height), ccam["width"], ccam["height"], ccam["f_c"], ccam["cxc"],
                              ccam["cyc"], T, tol_mm=tol_mm, max_frames=cfg.batch_size)
        self.h.depth_register_init(ccam["width"], ccam["height"], ccam["f_c"], ccam["cxc"], ccam["cyc"], T,
                                   map=ccam["map"], tol_mm=tol_mm, max_splat=DEFAULT_MAX_SPLAT,
                                   max_frames=cfg.batch_size, pair=p)
        shape = (cfg.batch_size, ccam["height"], ccam["width"], 3)
        dev = f"cuda:{self.device}"
        self.color_cams[p] = ColorCamera(shape[1:], torch.empty(shape, dtype=torch.uint8).pin_memory(),
                                         torch.zeros(shape, dtype=torch.uint8, device=dev), [False] * cfg.batch_size)
        if self.color_zero is None:   # a zero mask and a black image
            self.color_zero = {"mask": torch.zeros((cfg.batch_size, r.height, r.width), dtype=torch.uint8, device=dev),
                               "bgr": torch.zeros((cfg.batch_size, r.height, r.width, 3), dtype=torch.uint8, device=dev)}

    def mark_color(self, slot: int, frame_ts: float) -> None:
        for cc in self.color_cams.values():
            cc.mark(slot, frame_ts, self.cfg.stereo_color_max_dt)

    def drop_color(self) -> None:
        """The frame set the pushed images belong to was dropped."""
        for cc in self.color_cams.values():
            cc.pushed = None

    def take_color(self, n: int) -> dict:
        """The batch's colour images, and per pair which slots hold one."""
        return {p: cc.take(n) for p, cc in self.color_cams.items()}

    def _register_color(self, p: int, depth_ptr: int, frame_bytes: int, k0: int, m: int, has: list, stream: int,
                        stamps: list | None) -> dict:
        """Pair p's colour registered to the m depth frames at ``depth_ptr`` (batch slots k0 ..), into
        registration slots 0 .. m - 1; the slots of frames without a colour image get a zero mask and
        keep their registered depth, so the newest registered frame (``reg_last``) stays readable
        until a newer one is registered.  Returns the colour part of the pair's integrate call."""
        cc, h = self.color_cams[p], self.h
        cbytes = int(np.prod(cc.shape))
        j = 0
        while j < m:
            e = j
            while e < m and has[k0 + e] == has[k0 + j]:
                e += 1
            if has[k0 + j]:
                h.depth_register(depth_ptr + j * frame_bytes, frame_bytes, cc.dev.data_ptr() + (k0 + j) * cbytes,
                                 cbytes, e - j, first_slot=j, pair=p, stream=stream)
                self.reg_last[p] = (e - 1, None if stamps is None else float(stamps[k0 + e - 1]))
            else:
                h.depth_register_blank(e - j, first_slot=j, pair=p, stream=stream)
            j = e
        ptrs, nbytes = h.depth_register_buffers(p)
        return dict(color=ptrs["bgr"], color_stride=nbytes["bgr"], mask=ptrs["mask"], mask_stride=nbytes["mask"])

    # -- integration -----------------------------------------------------------------------------
    def integrate(self, records_ptr: int, n: int, stream: int, cams_per_frame: int | None = None,
                  stamps: list | None = None, has_color: dict | None = None, corr: np.ndarray | None = None) -> None:
        """The depth of the batch of n frames the handle has just tracked into the volume, with the
        batch's device-resident tracked poses (untracked frames are skipped), on the batch's stream.
        ``cams_per_frame``: the records per frame of the buffer (a sharded rig: rank 0's cameras,
        pair 0 first).  ``has_color[pair]`` says which of the frames came with a colour image
        (``stereo_color``; None: a device batch, geometry only); ``corr``: the loop graph's
        current correction (``dense_loop``)."""
        g0 = self.h.frames_done - n
        if self.cfg.stereo_depth:
            self._integrate_stereo(g0, n, stream, stamps, has_color, corr)
        else:
            self._integrate_records(records_ptr, g0, n, stream, 5 * self.hw * (cams_per_frame or self.P), corr, stamps)

    def _integrate_records(self, ptr: int, g0: int, n: int, stream: int, stride: int, corr, stamps: list | None = None) -> None:
        """RGB-D records ([BGR | u16 depth] per camera, ``stride`` bytes per frame)."""
        cfg, h, hw = self.cfg, self.h, self.hw
        depth = ptr + 3 * hw
        if cfg.dense_loop:
            # only frames that can have a pose-graph node go in, and into the archive (the device
            # picks g % loop_kf_interval == 0, tracked; frame 0 initialises and has none), on the
            # correction times their tracked pose
            skip = 1 if g0 == 0 else 0
            if n > skip:
                h.tsdf_archive_integrate(depth + skip * stride, stride, n - skip, first_frame=g0 + skip,
                                         world_T_corr=corr, stream=stream)
        elif self.dense:   # the selected cameras' parts of the batch's records, on the rig's body poses
            h.tsdf_integrate_rig(
                [dict(pair=p, depth=ptr + p * 5 * hw + 3 * hw, stride_bytes=stride,
                      color=ptr + p * 5 * hw if self.color else None) for p in self.dense],
                n, first_frame=g0, stream=stream)
        elif cfg.dense_align:   # aligned to the map first, integrated on the aligned poses
            h.tsdf_align(depth, stride, n, first_frame=g0, stream=stream)
            h.tsdf_integrate_aligned(depth, stride, n, color_dev_ptr=ptr if self.color else None, stream=stream)
        elif cfg.dense_dynamic:   # masked against the map's free space first, the filtered depth integrated
            self._integrate_filtered(depth, stride, n, g0, stream, None if stamps is None else float(stamps[n - 1]))
        elif self.color:   # the record's BGR part with its depth part
            h.tsdf_integrate_rgbd(ptr, depth, stride, n, first_frame=g0, pair=0, stream=stream)
        else:
            h.tsdf_integrate(depth, stride, n, first_frame=g0, pair=0, stream=stream)

    def _integrate_filtered(self, depth: int, stride: int, n: int, g0: int, stream: int, stamp) -> None:
        """``dense_dynamic``: n frames' depth through the free-space mask, then the filtered depth (on
        the rectified grid, in the mask state's slots) into the volume on the same poses."""
        h = self.h
        h.tsdf_dynamic(depth, stride, n, first_frame=g0, stream=stream)
        ptrs, nbytes = h.tsdf_dynamic_buffers()
        h.tsdf_integrate_rect(ptrs["depth"], nbytes["depth"], n, first_frame=g0, pair=0, stream=stream)
        self.dyn_last = (n - 1, stamp)

    def _integrate_stereo(self, g0: int, n: int, stream: int, stamps: list | None, has_color: dict | None, corr) -> None:
        """Stereo depth (k_stereo_depth.hip), in the rectified camera: one launch per run of
        consecutive frames g with g % stereo_depth_interval == 0 (the whole batch at interval 1); with
        ``dense_cameras`` camera ci's run in slots ci m .., then every camera's views in one launch."""
        cfg, h, dense = self.cfg, self.h, self.dense
        depth_ptr, _, frame_bytes = h.stereo_depth_buffers()

        def stamp(g):
            return None if stamps is None else float(stamps[g - g0])

        if cfg.dense_loop:   # only the node frames are matched
            for g in range(g0, g0 + n):
                if g % cfg.loop_kf_interval == 0 and g > 0:
                    h.stereo_depth(g, 1, pair=0, stream=stream)
                    h.tsdf_archive_integrate(depth_ptr, frame_bytes, 1, first_frame=g, world_T_corr=corr, stream=stream)
                    self.sd_last[0] = (0, stamp(g))
            return
        every = cfg.stereo_depth_interval
        runs = [(g0, n)] if every == 1 else [(g, 1) for g in range(g0, g0 + n) if g % every == 0]
        colored = [] if has_color is None else [p for p in (dense or (0,)) if p in self.color_cams]
        none = [False] * n
        for g, m in runs:
            if dense:
                views = []
                for ci, p in enumerate(dense):
                    h.stereo_depth(g, m, pair=p, stream=stream, first_slot=ci * m)
                    self.sd_last[p] = (ci * m + m - 1, stamp(g + m - 1))
                    views.append(dict(pair=p, rect=True, depth=depth_ptr + ci * m * frame_bytes, stride_bytes=frame_bytes))
                if colored:   # a pair without a colour camera: a black image and a zero mask
                    z = self.color_zero
                    blank = dict(color=z["bgr"].data_ptr(), color_stride=3 * self.hw, mask=z["mask"].data_ptr(),
                                 mask_stride=self.hw)
                    h.tsdf_integrate_rig_color(
                        [dict(**v, **(self._register_color(v["pair"], v["depth"], frame_bytes, g - g0, m,
                                                           has_color.get(v["pair"], none), stream, stamps)
                                      if v["pair"] in colored else blank)) for v in views],
                        m, first_frame=g, stream=stream)
                else:
                    h.tsdf_integrate_rig(views, m, first_frame=g, stream=stream)
                continue
            h.stereo_depth(g, m, pair=0, stream=stream)
            if cfg.dense_align:   # aligned to the map first, integrated on the aligned poses
                h.tsdf_align(depth_ptr, frame_bytes, m, first_frame=g, stream=stream)
                h.tsdf_integrate_aligned(depth_ptr, frame_bytes, m, stream=stream)
            elif cfg.dense_dynamic:   # masked against the map's free space first
                self._integrate_filtered(depth_ptr, frame_bytes, m, g, stream, stamp(g + m - 1))
            elif colored:   # pair 0's colour registered to the depth, with its mask
                col = self._register_color(0, depth_ptr, frame_bytes, g - g0, m, has_color.get(0, none), stream, stamps)
                h.tsdf_integrate_rect_color(col["color"], col["color_stride"], col["mask"], col["mask_stride"],
                                            depth_ptr, frame_bytes, m, first_frame=g, pair=0, stream=stream)
            else:
                h.tsdf_integrate_rect(depth_ptr, frame_bytes, m, first_frame=g, pair=0, stream=stream)
            self.sd_last[0] = (m - 1, stamp(g + m - 1))

    def follow(self, loop) -> None:
        """After the pose graph's nodes changed (a loop closed, a segment relocalised): every node's
        frame and pose to the archive, which moves the frames whose pose changed by more than the
        thresholds; queued on the handle's last stream, so before the next batch's integration."""
        cfg = self.cfg
        if not cfg.dense_loop or loop is None:
            return
        seen = len(loop.loops) + len(loop.relocs)
        if seen == self.loop_seen:
            return
        self.loop_seen = seen
        min_t = 0.5 * cfg.voxel_size if cfg.dense_loop_min_translation_m is None else cfg.dense_loop_min_translation_m
        self.h.tsdf_archive_move(loop.frames, np.array(loop.T).reshape(-1, 4, 4), min_t, cfg.dense_loop_min_rotation_rad)

    # -- readers (the engine's get_* methods describe them) ----------------------------------------
    def archive(self) -> dict:
        a = self.h.tsdf_archive_read()
        return {k: a[k] for k in ("frames", "world_T_cam", "moved_last", "moved_total")}

    def alignment(self) -> dict:
        return self.h.tsdf_align_read()

    def dynamic_mask(self) -> dict | None:
        if self.dyn_last is None:
            return None
        slot, stamp = self.dyn_last
        return {**self.h.tsdf_dynamic_read(slot), "timestamp": stamp}

    def freespace(self, world_T_volume: np.ndarray) -> dict:
        h = self.h
        run, settled = split(h.tsdf_freespace_read())
        shift, origin = h.tsdf_window()
        return {"run": run, "settled": settled, "origin": origin, "window_shift": shift, "world_T_volume": world_T_volume}

    def store(self, world_T_volume: np.ndarray) -> dict:
        cfg, h = self.cfg, self.h
        freespace = bool(cfg.dense_dynamic and cfg.dense_dynamic_settle_frames)
        bricks, words = h.tsdf_store_read()
        out = split_words(words, self.color, freespace)
        if freespace:
            out["run"], out["settled"] = split(out.pop("freespace"))
        return {**out, "bricks": bricks, "voxel_size": float(cfg.voxel_size),
                "origin": np.array(cfg.tsdf_origin, dtype=np.float64), "world_T_volume": world_T_volume,
                "stats": h.tsdf_store_stats()}

    def depth_image(self, pair: int) -> tuple | None:
        if pair not in self.sd_last:
            return None
        slot, stamp = self.sd_last[pair]
        return self.h.stereo_depth_read(slot)[0], stamp

    def registered_depth(self, pair: int) -> tuple | None:
        if pair not in self.reg_last:
            return None
        slot, stamp = self.reg_last[pair]
        return self.h.depth_register_read(slot, pair)["depth"], stamp

    def volume(self, world_T_volume: np.ndarray) -> dict:
        cfg, h = self.cfg, self.h
        tsdf, weight = h.tsdf_read()
        out = {}
        if self.color:
            out["color"], out["color_weight"] = h.tsdf_read_color()
        shift, origin = h.tsdf_window()
        return {**out, "tsdf": tsdf, "weight": weight, "origin": origin, "window_shift": shift,
                "voxel_size": float(cfg.voxel_size),
                "truncation_m": cfg.tsdf_integrator_truncation_distance_vox * cfg.voxel_size,
                "world_T_volume": world_T_volume}

    def view(self, world_T_volume: np.ndarray, world_T_view, size: tuple | None, intrinsics: tuple | None,
             newest_view) -> dict | None:
        """``newest_view()``: pair 0's rectified left camera at the newest published pose (or None),
        for a ``world_T_view`` of None."""
        cfg, h, r = self.cfg, self.h, self.rects[0]
        size = (int(r.width), int(r.height)) if size is None else (int(size[0]), int(size[1]))
        if intrinsics is None:
            intrinsics = scaled_intrinsics((r.width, r.height), (r.fx, r.fy, r.cx, r.cy), size)
        intrinsics = tuple(float(v) for v in intrinsics)
        if world_T_view is None:
            world_T_view = newest_view()
            if world_T_view is None:
                return None
        world_T_view = np.array(world_T_view, dtype=np.float64).reshape(4, 4)
        max_depth = cfg.dense_view_max_distance_m
        if max_depth is None:
            max_depth = cfg.tsdf_integrator_max_integration_distance_m
        key = (size, intrinsics, float(max_depth))
        if self.view_key != key:   # a new camera: its ray-length table and images
            check_render_params(size[0], size[1], *intrinsics, cfg.mesh_integrator_min_weight, 0.0, float(max_depth),
                                cfg.dense_view_step_scale)
            h.tsdf_render_init(size[0], size[1], *intrinsics, min_weight=cfg.mesh_integrator_min_weight,
                               min_depth=0.0, max_depth=float(max_depth), step_scale=cfg.dense_view_step_scale,
                               max_views=1, outputs=15 if self.color else 7)
            self.view_key = key
        h.tsdf_render(view_in_volume(world_T_volume, world_T_view)[None])
        out = h.tsdf_render_read(0)
        shift, origin = h.tsdf_window()
        res = {"depth": out["depth_m"], "depth_mm": out["depth_mm"], "normals": out["normal"], "intrinsics": intrinsics,
               "world_T_view": world_T_view, "origin": origin, "window_shift": shift, "world_T_volume": world_T_volume}
        if self.color:
            res["colors"] = out["color"]
        return res

    def mesh(self, world_T_volume: np.ndarray) -> dict:
        cfg = self.cfg
        if self.color:
            tris, cols = self.h.mesh(cfg.mesh_integrator_min_weight, colors=True)
            return {"triangles": tris, "colors": cols, "world_T_volume": world_T_volume}
        return {"triangles": self.h.mesh(cfg.mesh_integrator_min_weight), "world_T_volume": world_T_volume}

    def mesh_whole(self, world_T_volume: np.ndarray) -> dict:
        """The window and the brick store in one mesh (thor_slam_amd/dense_store.py)."""
        cfg, h = self.cfg, self.h
        out = {}
        if self.color:
            out["triangles"], out["colors"] = h.mesh_whole(cfg.mesh_integrator_min_weight, colors=True)
        else:
            out["triangles"] = h.mesh_whole(cfg.mesh_integrator_min_weight)
        return {**out, "world_T_volume": world_T_volume, "origin": np.array(cfg.tsdf_origin, dtype=np.float64),
                "bricks": h.mesh_whole_bricks}

    def esdf(self, world_T_volume: np.ndarray) -> dict:
        cfg = self.cfg
        esdf = self.h.esdf(cfg.esdf_integrator_max_distance_m, cfg.esdf_integrator_max_site_distance_vox,
                           cfg.esdf_integrator_min_weight)
        shift, origin = self.h.tsdf_window()
        return {"esdf": esdf, "origin": origin, "window_shift": shift, "voxel_size": float(cfg.voxel_size),
                "world_T_volume": world_T_volume}

    def esdf_slice(self, world_T_volume: np.ndarray) -> dict:
        cfg = self.cfg
        shift, origin = self.h.tsdf_window()
        s, y_org, ny = cfg.voxel_size, float(origin[1]), int(cfg.tsdf_dims[1])
        y0 = int(np.clip(np.floor((cfg.esdf_slice_min_height - y_org) / s), 0, ny - 1))
        y1 = int(np.clip(np.ceil((cfg.esdf_slice_max_height - y_org) / s), y0 + 1, ny))
        dist = self.h.esdf_slice(y0, y1, cfg.esdf_integrator_max_distance_m,
                                 cfg.esdf_integrator_max_site_distance_vox, cfg.esdf_integrator_min_weight)
        return {"distance": dist, "band": (y0, y1), "origin": origin, "window_shift": shift,
                "voxel_size": float(s), "world_T_volume": world_T_volume}
