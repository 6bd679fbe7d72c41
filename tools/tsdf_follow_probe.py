"""What the dense map's rolling window costs (tslam_tsdf_follow / tslam_tsdf_shift, k_tsdf.hip).

    python tools/tsdf_follow_probe.py [--frames 16] [--reps 10] [--out profiles/tsdf_follow_probe.json]

The default volume of HipSlamConfig (200 x 80 x 220 voxels of 0.05 m) with the colour layer, one
RGB-D camera at 640x480, `frames` frames per call on the tracked device poses (what the engine's
_integrate_depth does: no host synchronise).  On one handle, in one run, HIP events around `reps`
back-to-back calls after a warm-up, three trials, the cases alternated:

  follow_on    an integrate call with following on that does not move (k_tsdf_follow and the two
               k_tsdf_move launches that return at once, then the integration at the effective origin),
  follow_off   the same call with following off,
  shift        an explicit move by one step (tslam_tsdf_shift by +step, then -step, ... in x, which
               is the coalesced axis and at the default step 16 takes the wide-vector path),
  shift_odd    the same by one voxel in x (the scalar path),
  copy         a device-to-device copy of the bytes the move handles: every layer read once and
               written once, twice (out to the scratch and back) = hipMemcpyAsync of 24 B per voxel,
               two times.

follow_on - follow_off is the price every call pays; shift / copy says how far the move is from a
plain copy of the same bytes.  Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    W, H, B = args.width, args.height, args.frames
    cfg = HipSlamConfig(rgbd=True)
    src = SyntheticRGBDSource(width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rect = rgbd_undistort(cams[ci])
    dev = torch.from_numpy(np.ascontiguousarray(src.render_rgbd_sequence(B)[:, None, :])).cuda()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    h = Handle([rect], cfg, max_batch=B)
    h.submit(dev.data_ptr(), B, s)
    tracked = int((h.read_poses(B)["stats"][:, 0, 0] == 0).sum())
    h.tsdf_color(True)
    h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
    hw, step = W * H, cfg.dense_follow_step
    nv = int(np.prod(cfg.tsdf_dims))

    def integrate():
        h.tsdf_integrate_rgbd(dev.data_ptr(), dev.data_ptr() + 3 * hw, 5 * hw, B, first_frame=0, stream=s)

    sign = [1]

    def shift(n):
        def run():
            h.tsdf_shift((sign[0] * n, 0, 0), stream=s)
            sign[0] = -sign[0]
        return run

    a, b = torch.empty(6 * nv, dtype=torch.float32, device="cuda"), torch.empty(6 * nv, dtype=torch.float32, device="cuda")

    def copy():
        b.copy_(a, non_blocking=True)
        a.copy_(b, non_blocking=True)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps   # us per call

    def follow(on):
        def run():
            h.tsdf_follow(margin=cfg.dense_follow_margin, step=step, enable=on)
            return integrate
        return run

    cases = {"follow_on": follow(True), "follow_off": follow(False), "shift": lambda: shift(step), "shift_odd": lambda: shift(1),
             "copy": lambda: copy}
    h.tsdf_follow(margin=cfg.dense_follow_margin, step=step)       # allocates the record and the scratch
    res = {k: [] for k in cases}
    for k, mk in cases.items():
        timed(mk(), 2)                                              # warm-up (code objects, first touch)
    for _ in range(3):
        for k, mk in cases.items():
            res[k].append(timed(mk(), args.reps - args.reps % 2))   # an even number: the shifts end where they began
    moved = h.tsdf_window()[0].tolist()
    observed = int((h.tsdf_read()[1] > 0).sum())
    h.close()

    best = {k: min(v) for k, v in res.items()}
    out = {
        "what": "rolling window of the dense map: HIP events around %d back-to-back calls after a warm-up, three trials, "
                "the cases alternated, one handle, one session" % (args.reps - args.reps % 2),
        "width": W, "height": H, "frames_per_call": B, "tracked_frames": tracked, "poses": "device",
        "volume_dims": list(cfg.tsdf_dims), "volume_voxels": nv, "voxel_size_m": cfg.voxel_size, "color_layer": True,
        "step_voxels": step, "window_shift_at_the_end": moved, "observed_voxels_at_the_end": observed,
        "us_per_call_trials": {k: [round(t, 1) for t in v] for k, v in res.items()},
        "us_per_call": {k: round(t, 1) for k, t in best.items()},
        "follow_on_minus_off_us": round(best["follow_on"] - best["follow_off"], 1),
        "shift_over_copy": round(best["shift"] / best["copy"], 2),
        "shift_odd_over_copy": round(best["shift_odd"] / best["copy"], 2),
        "bytes_per_move": 4 * 24 * nv,
        "copy_GBps": round(4 * 24 * nv / (best["copy"] * 1e-6) / 1e9, 1),
        "shift_GBps": round(4 * 24 * nv / (best["shift"] * 1e-6) / 1e9, 1),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
