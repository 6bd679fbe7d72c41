"""What the free-space depth mask costs (tslam_tsdf_dynamic, k_tsdf_dynamic.hip).

    python tools/tsdf_dynamic_probe.py [--frames 64] [--reps 10] [--out profiles/tsdf_dynamic_probe.txt]

The volume of bench.py's C5 configuration (176 x 72 x 176 voxels of 0.05 m), one RGB-D camera at
640 x 400.  `unique` rendered frames are replayed as a triangle wave into one batch of `frames`
frames, tracked, and integrated on the tracked device poses; an object (a block of depth 1.5 m in
mid-air) is then put into every frame, so that the mask has something to find.  On one handle, in one
run, HIP events around `reps` back-to-back calls after a warm-up, three trials, the cases alternated:

  dynamic           tslam_tsdf_dynamic of the batch (poses, classify, apply),
  integrate_rect    tslam_tsdf_integrate_rect of the filtered depth it leaves (what follows it in
                    the engine), on the same poses,
  integrate         tslam_tsdf_integrate of the raw depth of the same frames (what the engine does
                    without the option).

Also the bytes the rule must move per frame: 2 B read and 3 B written per pixel (depth in, depth and
mask out), one 8-byte gather (tsdf, weight) per valid pixel, and the mask words (a candidate word and
a valid-pixel word per 64 pixels) written once and read once; over the call's time that is a rate,
not a share of any peak.  There is no pass bar: nothing of the kind existed before.  Needs the GPU:
there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))

C5_ORIGIN, C5_DIMS = (-7.2, -1.8, -4.4), (176, 72, 176)   # bench.py's TSDF_ORIGIN / TSDF_DIMS


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.dense_dynamic import DEFAULTS
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    W, H, B, U = args.width, args.height, args.frames, args.unique
    hw = W * H
    cfg = HipSlamConfig(rgbd=True, dense_map=True, dense_color=False, dense_dynamic=True)
    src = SyntheticRGBDSource(width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rect = rgbd_undistort(cams[ci])
    uniq = src.render_rgbd_sequence(U)
    wave = [abs((i + U - 1) % (2 * U - 2) - (U - 1)) if U > 1 else 0 for i in range(B)]   # 0 1 .. U-1 .. 1 0 1 ..
    rec = np.ascontiguousarray(uniq[wave][:, None, :])
    dev = torch.from_numpy(rec).cuda()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    h = Handle([rect], cfg, max_batch=B)
    h.submit(dev.data_ptr(), B, s)
    tracked = int((h.read_poses(B)["stats"][:, 0, 0] == 0).sum())
    h.tsdf_init(C5_ORIGIN, C5_DIMS, 0.05, 4.0, 10.0, 100.0)
    depth, stride = dev.data_ptr() + 3 * hw, 5 * hw
    h.tsdf_integrate(depth, stride, B, first_frame=0, stream=s)
    torch.cuda.synchronize()
    # the object: every frame's depth with a block of 1.5 m in mid-air (the records' poses are tracked already)
    obj = rec.copy()
    for f in range(B):
        d = obj[f, 0, 3 * hw:].view(np.uint16).reshape(H, W)
        d[H // 2 - 40:H // 2 + 40, W // 2 - 60:W // 2 + 60] = 1500
    dev_obj = torch.from_numpy(obj).cuda()
    odepth = dev_obj.data_ptr() + 3 * hw
    h.tsdf_dynamic_init(pair=0, rect=False, max_frames=B, **DEFAULTS)
    h.tsdf_dynamic(odepth, stride, B, first_frame=0, stream=s)
    stats = np.stack([h.tsdf_dynamic_read(f)["stats"] for f in range(B)])
    filtered = h.tsdf_dynamic_buffers()[0]["depth"]

    cases = {
        "dynamic": lambda: h.tsdf_dynamic(odepth, stride, B, first_frame=0, stream=s),
        "integrate_rect": lambda: h.tsdf_integrate_rect(filtered, 2 * hw, B, first_frame=0, stream=s),
        "integrate": lambda: h.tsdf_integrate(odepth, stride, B, first_frame=0, stream=s),
    }

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps   # us per call

    res = {k: [] for k in cases}
    for fn in cases.values():
        timed(fn, 2)                                  # warm-up (code objects, first touch)
    for _ in range(3):
        for k, fn in cases.items():
            res[k].append(timed(fn, args.reps))
    h.close()

    best = {k: min(v) for k, v in res.items()}
    used = stats[:, 0] == 0
    valid = float(stats[used, 1].mean()) if used.any() else 0.0
    words = (W + 63) // 64 * H
    bytes_frame = {"depth_in": 2 * hw, "depth_out": 2 * hw, "mask_out": hw, "voxel_gather": int(8 * valid),
                   "mask_words_written_and_read": 2 * 16 * words}
    total = sum(bytes_frame.values())
    out = {
        "what": "free-space depth mask: HIP events around %d back-to-back calls of %d frames after a warm-up, three trials, "
                "the cases alternated, one handle, one session" % (args.reps, B),
        "width": W, "height": H, "frames": B, "unique_frames": U, "tracked_frames": tracked, "volume_dims": list(C5_DIMS),
        "voxel_size_m": 0.05, "parameters": DEFAULTS, "table_lookup": not rect.is_identity,
        "used_frames": int(used.sum()), "valid_pixels_mean": round(valid, 1),
        "candidates_mean": round(float(stats[used, 2].mean()), 1) if used.any() else 0.0,
        "masked_valid_pixels_mean": round(float(stats[used, 3].mean()), 1) if used.any() else 0.0,
        "us_per_call_trials": {k: [round(t, 1) for t in v] for k, v in res.items()},
        "us_per_call": {k: round(t, 1) for k, t in best.items()},
        "us_per_frame": {k: round(t / B, 2) for k, t in best.items()},
        "bytes_per_frame": bytes_frame, "bytes_per_frame_total": total,
        "dynamic_gb_per_s": round(total * B / best["dynamic"] / 1e3, 1),
    }
    lines = [
        "tslam_tsdf_dynamic at %d x %d, calls of %d frames, volume %s (HIP events, best of three trials of %d calls)"
        % (W, H, B, "x".join(map(str, C5_DIMS)), args.reps),
        "  dynamic         %9.1f us per call  %7.2f us per frame" % (best["dynamic"], best["dynamic"] / B),
        "  integrate_rect  %9.1f us per call  %7.2f us per frame  (the filtered depth, same frames)"
        % (best["integrate_rect"], best["integrate_rect"] / B),
        "  integrate       %9.1f us per call  %7.2f us per frame  (the raw depth, same frames)"
        % (best["integrate"], best["integrate"] / B),
        "  bytes the rule must move per frame: %d (%s); %.1f GB/s over the dynamic call"
        % (total, ", ".join("%s %d" % kv for kv in bytes_frame.items()), out["dynamic_gb_per_s"]),
        json.dumps(out),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
