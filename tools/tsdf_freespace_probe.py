"""What the free-space layer costs (tslam_tsdf_freespace_*, k_tsdf_freespace.hip).

    python tools/tsdf_freespace_probe.py [--frames 64] [--reps 10] [--out profiles/tsdf_freespace_probe.txt]

The case of tools/tsdf_dynamic_probe.py: the volume of bench.py's C5 configuration (176 x 72 x 176
voxels of 0.05 m), one RGB-D camera at 640 x 400, `unique` rendered frames replayed as a triangle
wave into one batch of `frames` frames, tracked and integrated on the tracked device poses, then an
object (a block of depth 1.5 m in mid-air) put into every frame.  On one handle, in one run, HIP events
around `reps` back-to-back calls after a warm-up, three trials, the cases alternated:

  dynamic_off   tslam_tsdf_dynamic without the layer (the call as it was before the layer existed),
  dynamic_on    the same call with the layer: the classify kernel gathers one more word per valid
                pixel, and k_tsdf_poses + k_freespace_update follow the mask's kernels,
  integrate     tslam_tsdf_integrate of the same raw frames: the launch whose walk k_freespace_update
                shares (same bricks, same frames, same projections; it moves 8 B per voxel it
                touches, the update 4 B and only where the word changed).

Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/tsdf_freespace_probe.py
--reps 3) the same run gives k_freespace_update's and k_tsdf_integrate's own durations side by side.
There is no pass bar.  Needs the GPU: there is no fallback.
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
    ap.add_argument("--settle-frames", type=int, default=30)
    ap.add_argument("--band-vox", type=float, default=1.5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.dense_dynamic import DEFAULTS
    from thor_slam_amd.dense_freespace import split
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
    obj = rec.copy()
    for f in range(B):
        d = obj[f, 0, 3 * hw:].view(np.uint16).reshape(H, W)
        d[H // 2 - 40:H // 2 + 40, W // 2 - 60:W // 2 + 60] = 1500
    dev_obj = torch.from_numpy(obj).cuda()
    odepth = dev_obj.data_ptr() + 3 * hw
    h.tsdf_dynamic_init(pair=0, rect=False, max_frames=B, **DEFAULTS)

    def layer(on: bool) -> None:
        h.tsdf_freespace_init(settle_frames=args.settle_frames, occupied_band_vox=args.band_vox, enable=on)

    cases = {
        "dynamic_off": (False, lambda: h.tsdf_dynamic(odepth, stride, B, first_frame=0, stream=s)),
        "dynamic_on": (True, lambda: h.tsdf_dynamic(odepth, stride, B, first_frame=0, stream=s)),
        "integrate": (None, lambda: h.tsdf_integrate(odepth, stride, B, first_frame=0, stream=s)),
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
    for rnd in range(4):                             # the first round is the warm-up (code objects, first touch)
        for k, (on, fn) in cases.items():
            if on is not None:
                layer(on)                            # a new, zero layer (or none) before every timed run; synchronises
            t = timed(fn, args.reps)
            if rnd:
                res[k].append(t)
    layer(True)
    h.tsdf_dynamic(odepth, stride, B, first_frame=0, stream=s)
    run, settled = split(h.tsdf_freespace_read())
    stats = np.stack([h.tsdf_dynamic_read(f)["stats"] for f in range(B)])
    h.close()

    best = {k: min(v) for k, v in res.items()}
    nv = int(np.prod(C5_DIMS))
    touched = int((run > 0).sum())
    out = {
        "what": "free-space layer: HIP events around %d back-to-back calls of %d frames after a warm-up round, three trials, "
                "the cases alternated, one handle, one session" % (args.reps, B),
        "width": W, "height": H, "frames": B, "unique_frames": U, "tracked_frames": tracked, "volume_dims": list(C5_DIMS),
        "voxel_size_m": 0.05, "settle_frames": args.settle_frames, "occupied_band_vox": args.band_vox,
        "table_lookup": not rect.is_identity, "used_frames": int((stats[:, 0] == 0).sum()),
        "voxels": nv, "voxels_with_a_run_after_one_call": touched, "settled_after_one_call": int(settled.sum()),
        "layer_bytes": 4 * nv, "bytes_stored_by_one_call_at_most": 4 * touched,
        "us_per_call_trials": {k: [round(t, 1) for t in v] for k, v in res.items()},
        "us_per_call": {k: round(t, 1) for k, t in best.items()},
        "us_per_frame": {k: round(t / B, 2) for k, t in best.items()},
        "layer_us_per_call": round(best["dynamic_on"] - best["dynamic_off"], 1),
    }
    lines = [
        "tslam_tsdf_dynamic with and without the free-space layer at %d x %d, calls of %d frames, volume %s "
        "(HIP events, best of three trials of %d calls)" % (W, H, B, "x".join(map(str, C5_DIMS)), args.reps),
        "  dynamic_off  %9.1f us per call  %7.2f us per frame  (no layer)" % (best["dynamic_off"], best["dynamic_off"] / B),
        "  dynamic_on   %9.1f us per call  %7.2f us per frame  (classify with the layer, then the layer's update)"
        % (best["dynamic_on"], best["dynamic_on"] / B),
        "  integrate    %9.1f us per call  %7.2f us per frame  (the raw depth, same frames: the walk the update shares)"
        % (best["integrate"], best["integrate"] / B),
        "  the layer: %d voxels, %d B; one call from a zero layer leaves a run in %d voxels (%d B stored at most), %d settled"
        % (nv, 4 * nv, touched, 4 * touched, int(settled.sum())),
        json.dumps(out),
    ]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == "__main__":
    main()
