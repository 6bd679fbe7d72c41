"""Time the dense stereo matcher (tslam_stereo_depth, k_stereo_depth.hip) on resident data.

    python tools/stereo_depth_probe.py [--frames 64] [--disp 128] [--reps 10] [--out profiles/stereo_depth_c2.json]
    python tools/stereo_depth_probe.py --sgm [--p1 100] [--p2 1200] [--out profiles/stereo_depth_sgm_c2.json]
    python tools/stereo_depth_probe.py --filter [--median 5] [--speckle-size 50] [--out profiles/stereo_depth_filter_c2.json]

C2 geometry by default (640x400, one pair, D = 128, 64 frames resident in the ring).  One batch is
tracked first so the ring holds rectified images; after a warm-up launch the matcher runs `reps`
times between two HIP events on the launch stream.  For the cost relative to tracking the same run
times k_detect alone (inside a batch, also between events) over the same frames.  The bytes per
frame are what the algorithm must move (both images read once, depth + disp32 written, the two u8
winner maps written and read once); (x, d) cells = W * H * D per frame.  Needs the GPU: there is
no fallback.

With --sgm the same run then turns semi-global aggregation on (tslam_stereo_depth_sgm, k_sd_sgm.hip)
and times it the same way on the same frames, so both figures come from one session.  Its bytes per
frame are what its stages must move through device memory: the volume A (u16, W * H * D cells)
written once, read by each of the four path passes and not again; S written by the first pass, read
and written by the other three, read by the winners; plus the box matcher's images and outputs.

With --filter the same run then turns the post-filters on (tslam_stereo_depth_filter, k_sd_filter.hip)
in three settings, the median alone, the speckle filter alone and both, and times the matcher with
them the same way on the same frames: the filter stage is the difference to the box matcher's time
of this session.  As a cross-check the stage is also timed on its own through
tslam_stereo_depth_filter_apply on the unfiltered disp32 (that route adds a clamping copy).  Its
bytes per frame are what its launches must move: 2 B read and 2 B written per pixel by the median,
the labelling's 2 B read and 8 B written, 4 B read by the sum, 6 B read and 4 B written by the last
pass, which also writes the depth.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))

HBM_PEAK_TBS = 8.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--disp", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--sgm", action="store_true", help="also time semi-global aggregation on the same input")
    ap.add_argument("--p1", type=int, default=100)
    ap.add_argument("--p2", type=int, default=1200)
    ap.add_argument("--filter", action="store_true", help="also time the median and speckle filters on the same input")
    ap.add_argument("--median", type=int, default=5)
    ap.add_argument("--speckle-size", type=int, default=50)
    ap.add_argument("--speckle-range", type=int, default=32)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticStereoSource

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    W, H, B, D = args.width, args.height, args.frames, args.disp
    src = SyntheticStereoSource(seed=0, width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    rect = stereo_rectify(cams[li], cams[ri])
    uniq = src.render_stereo_sequence(8)
    frames = uniq[[i % 8 for i in range(B)]]
    dev = torch.from_numpy(frames).cuda()
    h = Handle([rect], HipSlamConfig(), max_batch=B)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    h.submit(dev.data_ptr(), B, s)
    torch.cuda.synchronize()
    h.stereo_depth_init(max_frames=B, n_disp=D)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps   # us per call

    run = lambda: h.stereo_depth(0, B, pair=0, stream=s)   # noqa: E731
    timed(run, 2)                                          # warm-up (code object, attribute call)
    trials = [timed(run, args.reps) for _ in range(3)]
    us_batch = min(trials)
    depth, disp32 = h.stereo_depth_read(B - 1)
    valid = float((depth > 0).mean())

    sgm = None
    if args.sgm:
        h.stereo_depth_sgm(p1=args.p1, p2=args.p2)
        timed(run, 2)
        sgm_trials = [timed(run, args.reps) for _ in range(3)]
        sgm_valid = float((h.stereo_depth_read(B - 1)[0] > 0).mean())
        h.stereo_depth_sgm(enable=False)
        cells = W * H * ((D + 3) & ~3)
        vol_bytes = 2 * cells * (1 + 4)                 # A: written, read by 4 passes
        sum_bytes = 2 * cells * (1 + 3 * 2 + 1)         # S: written, 3 x (read + written), read by the winners
        sgm_bytes = 2 * W * H + 2 * 2 * W * H + 2 * 2 * W * H + vol_bytes + sum_bytes
        sgm_us = min(sgm_trials) / B
        sgm = {
            "p1": args.p1, "p2": args.p2, "paths": 15,
            "us_per_batch_trials": [round(t, 1) for t in sgm_trials],
            "us_per_frame": round(sgm_us, 2),
            "bytes_per_frame": sgm_bytes,
            "achieved_GBps": round(sgm_bytes / sgm_us / 1e3, 2),
            "share_of_8TBps_peak": round(sgm_bytes / sgm_us / 1e6 / HBM_PEAK_TBS, 5),
            "over_box_matcher": round(min(sgm_trials) / us_batch, 2),
            "valid_fraction_last_frame": round(sgm_valid, 4),
        }

    flt = None
    if args.filter:
        px = W * H
        settings = {   # name -> (median, speckle_size, bytes per pixel that must move)
            "median": (args.median, 0, 2 + 2 + 2 + 2 + 2),              # disp32 -> median; median -> disp32, depth
            "speckle": (0, args.speckle_size, 2 + 8 + 4 + 2 + 4 + 4),   # label: read, label + count; sum: count; apply: disp32, label -> disp32, depth
            "both": (args.median, args.speckle_size, 4 + 2 + 8 + 4 + 2 + 4 + 4),
        }
        h.stereo_depth(0, B, pair=0, stream=s)
        raw = torch.from_numpy(np.stack([h.stereo_depth_read(f)[1] for f in range(B)]).view(np.int16)).cuda()   # unfiltered disp32
        flt = {"median_window": args.median, "speckle_size": args.speckle_size, "speckle_range": args.speckle_range,
               "box_us_per_frame": round(us_batch / B, 2)}
        for name, (m, size, bpp) in settings.items():
            h.stereo_depth_filter(median=m, speckle_size=size, speckle_range=args.speckle_range)
            timed(run, 2)
            with_trials = [timed(run, args.reps) for _ in range(3)]
            depth_f = h.stereo_depth_read(B - 1)[0]
            alone = lambda: h.stereo_depth_filter_apply(raw.data_ptr(), W, H, rect.fx * rect.baseline, B, stream=s)   # noqa: E731
            timed(alone, 2)
            alone_trials = [timed(alone, args.reps) for _ in range(3)]
            us = (min(with_trials) - us_batch) / B
            flt[name] = {
                "matcher_and_filter_us_per_batch_trials": [round(t, 1) for t in with_trials],
                "filter_us_per_frame": round(us, 2),                       # beside the matcher's own trials above
                "filter_apply_us_per_batch_trials": [round(t, 1) for t in alone_trials],
                "filter_apply_us_per_frame": round(min(alone_trials) / B, 2),   # includes the clamping copy (4 B / px more)
                "bytes_per_frame": bpp * px,
                "achieved_GBps": round(bpp * px / max(us, 1e-3) / 1e3, 2),
                "over_box_matcher": round(us * B / us_batch, 3),
                "valid_fraction_last_frame": round(float((depth_f > 0).mean()), 4),
            }
        h.stereo_depth_filter(enable=False)

    h.begin_batch(dev.data_ptr(), B)
    h.run_kernel("rectify_pyramid", s)
    timed(lambda: h.run_kernel("detect", s), 2)
    det_trials = [timed(lambda: h.run_kernel("detect", s), args.reps) for _ in range(3)]
    h.end_batch()
    h.close()

    us_frame = us_batch / B
    bytes_frame = 2 * W * H + 2 * 2 * W * H + 2 * 2 * W * H   # images + u16 outputs + u8 winner maps (write, read)
    out = {
        "what": "tslam_stereo_depth, HIP events around %d back-to-back calls, best of 3 trials" % args.reps,
        "width": W, "height": H, "n_disp": D, "frames": B,
        "us_per_batch_trials": [round(t, 1) for t in trials],
        "us_per_frame": round(us_frame, 2),
        "bytes_per_frame": bytes_frame,
        "achieved_GBps": round(bytes_frame / us_frame / 1e3, 2),
        "share_of_8TBps_peak": round(bytes_frame / us_frame / 1e6 / HBM_PEAK_TBS, 5),
        "cells_per_frame": W * H * D,
        "cells_per_second": round(W * H * D / us_frame * 1e6, 0),
        "valid_fraction_last_frame": round(valid, 4),
        "k_detect_us_per_batch_trials": [round(t, 1) for t in det_trials],
        "k_detect_us_per_frame_both_cameras": round(min(det_trials) / B, 3),
        "stereo_depth_over_k_detect": round(us_batch / min(det_trials), 1),
    }
    if sgm is not None:
        out["sgm"] = sgm
    if flt is not None:
        out["filter"] = flt
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
