"""The sharded rig (``HipSlamConfig(devices=[d0, d1, ...])``; cuVSLAM's multicam mode,
launch/thor_visual_slam.launch.py:49,81): one camera stream per GPU from this one process.

One handle per device (the whole rig on each, rank r owning cameras [r*S, (r+1)*S)), driven by the
library as one sharded rig (``tslam_group_*``: an RCCL clique over the devices, or device copies with
``shard_transport="copy"``), with the state gather to rank 0 (``TSLAM_SHARD_GATHER``: local BA, loop
closure and relocalisation run on rank 0's handle) and pinned result slots (asynchronous polling, like
``tslam_submit_host``'s); pinned staging and a device input per rank and batch parity.  The published
poses are bit-identical to the one-device engine's."""

from __future__ import annotations

import collections

from .._lib import Handle, HandleGroup


class _ShardedRig:
    def __init__(self, torch, cfg, rects: list, base_T_rects: list, shape: tuple) -> None:
        """``shape``: the whole rig's input batch, (batch_size, cameras, ...)."""
        self.torch = torch
        self.devices = [int(d) for d in cfg.devices]
        world = len(self.devices)
        n_cams = shape[1]
        if n_cams % world:
            raise RuntimeError(f"{n_cams} cameras do not split over {world} devices")
        self.handles = []
        for d in self.devices:
            h = Handle(rects, cfg, max_batch=cfg.batch_size, device=d)
            if len(rects) > 1:
                h.set_rig(base_T_rects)
            self.handles.append(h)
        self.group = HandleGroup(self.handles, cfg.shard_transport)
        # results through the slots; the state gather (rank 0's ring as the one-handle path's) is the
        # stereo rig's: a camera-sharded RGB-D rig moves pair blocks and keeps no rig-wide ring
        self.handles[0].shard_options(gather=not cfg.rgbd, results=True, pipeline=True)
        self.S = n_cams // world   # cameras per rank
        part = (cfg.batch_size, self.S) + tuple(shape[2:])
        self.batches = 0
        self.stamps: collections.deque = collections.deque()   # per batch in flight: the driver's slots carry frame indices only
        self.dev = [[torch.empty(part, dtype=torch.uint8, device=f"cuda:{d}") for _ in range(2)] for d in self.devices]
        self.host = [[torch.empty(part, dtype=torch.uint8).pin_memory() for _ in range(2)] for _ in self.devices]
        self.h2d = [[None, None] for _ in self.devices]

    def submit(self, staged: list, n: int, before_submit=None) -> tuple:
        """The staged (images, timestamp) frames (any count up to batch_size) through the group
        driver, rank r getting its cameras' slice; ``before_submit`` runs once the inputs are on their
        way.  Returns rank 0's device input and the stream it was copied on."""
        torch, S = self.torch, self.S
        k = self.batches & 1
        ptrs, streams = [], []
        for r, d in enumerate(self.devices):
            if self.h2d[r][k] is not None:   # the pinned buffer of this parity: batch s-2's copy is done
                self.h2d[r][k].synchronize()
            host = self.host[r][k].numpy()
            for i, (imgs, _) in enumerate(staged):
                host[i] = imgs[r * S:(r + 1) * S]
            stream = torch.cuda.current_stream(d)
            # the device input of this parity: the driver made this stream wait for batch s-2
            self.dev[r][k][:n].copy_(self.host[r][k][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            self.h2d[r][k] = ev
            ptrs.append(self.dev[r][k].data_ptr())
            streams.append(stream.cuda_stream)
        if before_submit is not None:
            before_submit()
        self.group.submit(ptrs, n, streams)
        self.stamps.append([ts for _, ts in staged])
        self.batches += 1
        return ptrs[0], streams[0]

    def set_motion_prior(self, *args) -> None:
        """Every rank's handle: each refines its frame range and chains the whole batch."""
        for h in self.handles:
            h.set_motion_prior(*args)

    def reset(self) -> None:
        self.stamps.clear()
        for h in self.handles:
            h.reset()

    def close(self) -> None:
        self.group.close()
        for h in self.handles:
            h.close()
