"""What depth registration costs (tslam_depth_register, k_depth_register.hip).

    python tools/depth_register_probe.py [--frames 64] [--reps 5] [--out profiles/depth_register_probe.json]

A 640x400 stereo handle; the depth is the left camera's rendered depth of the synthetic room (four
distinct frames, repeated to `frames`), the colour camera sits 37.5 mm beside it.  Two colour sizes:
1280x800 (the reference's rgb_output_resolution beside 640x400 stereo) and 640x400.  Per size, on one
handle in one run: two warm-up calls, then three trials of `reps` calls of `frames` frames each; the
library's own HIP events around the three passes of every call (tslam_depth_register_profile) give
clear / splat / gather, and the best call of all trials is reported per pass.

Each pass is set against its floor, a plain device-to-device copy (torch, HIP events, same warm-up and
trials) that moves the bytes the pass must move.  A copy of N bytes reads N and writes N, so the floor
of a pass that must move M bytes is a copy of M / 2.  Per frame, with d = depth pixels and c = colour
pixels:

  clear    4 c               the z-buffer written
  splat    2 d + 4 c         the depth read, every z-buffer word updated at least once
  gather   13 d + 6 c        depth read (2 d), z-buffer and colour gathered (4 d + 3 d), bgr and mask
                             written (3 d + d), the z-buffer read and the registered depth written (4 c + 2 c)

The ratio time / floor is reported; no bar is set.  Needs the GPU: there is no fallback.
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
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.depth_register import color_camera, compose_color_T_rect
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticStereoColorSource

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    W, H, n = 640, 400, args.frames
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps   # us per call

    def copy_us(nbytes):
        a = torch.empty(int(nbytes), dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        timed(lambda: b.copy_(a), 2)
        return min(timed(lambda: b.copy_(a), args.reps) for _ in range(3))

    results = {}
    for Wc, Hc in ((1280, 800), (640, 400)):
        src = SyntheticStereoColorSource(width=W, height=H, color_width=Wc, color_height=Hc)
        cams = extract_cameras(CameraRig([src]).calibration, 2)
        (li, ri), = stereo_pairs(cams)
        rect = stereo_rectify(cams[li], cams[ri])
        depth, color = [], []
        for f in range(4):
            _, z = src.scene.render(src.camera_pose(f, 0), src.get_intrinsics()[0], None, return_depth=True)
            depth.append(np.clip(np.floor(z * 1000.0 + 0.5), 0, 65535).astype(np.uint16))
            color.append(src.render_color(f))
        ddev = torch.from_numpy(np.stack([depth[f % 4] for f in range(n)]).view(np.int16)).cuda()
        cdev = torch.from_numpy(np.stack([color[f % 4] for f in range(n)])).cuda()
        ccam = color_camera(src.get_rgbd_intrinsics()[0])
        T = compose_color_T_rect(src.left_T_color().to_4x4_matrix(), rect.left_optical_T_rect())
        h = Handle([rect], HipSlamConfig(), max_batch=1)
        h.depth_register_init(ccam["width"], ccam["height"], ccam["f_c"], ccam["cxc"], ccam["cyc"], T, map=ccam["map"],
                              max_frames=n)
        h.depth_register_profile(True)
        d, c = W * H, Wc * Hc

        def call():
            h.depth_register(ddev.data_ptr(), 2 * d, cdev.data_ptr(), 3 * c, n, stream=s)

        for _ in range(2):
            call()
        torch.cuda.synchronize()
        passes, calls = [], []
        for _ in range(3):
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                p = h.depth_register_profile(True, read=True)
                torch.cuda.synchronize()
                passes.append(p)
                calls.append(1000.0 * e0.elapsed_time(e1))
        out = h.depth_register_read(n - 1)
        h.close()
        moved = {"clear": 4 * c * n, "splat": (2 * d + 4 * c) * n, "gather": (13 * d + 6 * c) * n}
        best = {k: 1000.0 * min(p[k] for p in passes) for k in moved}
        floor = {k: copy_us(v / 2) for k, v in moved.items()}
        results[f"{W}x{H}->{Wc}x{Hc}"] = {
            "frames_per_call": n, "calls_timed": len(passes),
            "us_per_call": round(min(calls), 1), "us_per_pass": {k: round(v, 1) for k, v in best.items()},
            "bytes_moved": moved, "floor_copy_us": {k: round(v, 1) for k, v in floor.items()},
            "ratio_to_floor": {k: round(best[k] / floor[k], 2) for k in moved},
            "us_per_frame": round(min(calls) / n, 2),
            "mask_fraction": round(float(out["mask"].mean()), 4), "registered_fraction": round(float((out["depth"] > 0).mean()), 4),
        }
    res = {"what": "depth registration: the library's HIP events around the three passes of a call, two warm-up calls, "
                   "three trials x %d calls, the best call per pass; floors: device copies of half the bytes a pass moves" % args.reps,
           "cases": results}
    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
