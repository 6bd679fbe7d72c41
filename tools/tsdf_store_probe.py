"""What the brick store behind the dense map's rolling window costs (tslam_tsdf_store_init,
k_tsdf_store.hip).

    python tools/tsdf_store_probe.py [--frames 16] [--reps 10] [--out profiles/tsdf_store_probe.json]

tools/tsdf_follow_probe.py's setting: the default volume of HipSlamConfig (200 x 80 x 220 voxels of
0.05 m) with the colour layer, one RGB-D camera at 640x480, `frames` frames per call on the tracked
device poses, the default pool of 65,536 bricks.  On one handle, in one run, HIP events around `reps`
back-to-back calls after a warm-up, three trials, the cases alternated (the store is created and
freed between the timed parts, never inside one):

  nomove_on / nomove_off   an integrate call with following on that does not move, the store on / off:
                           the difference is k_tsdf_store_out and k_tsdf_store_in returning at once;
  out_on / out_off         `reps` explicit moves by one step (+16 voxels in x) of a window that was
                           just integrated: with the store on every move's outgoing slab is stored
                           (nothing comes in: the store has nothing ahead);
  in_on / in_off           the `reps` moves back (-16 in x): with the store on every move's incoming
                           slab comes from the populated store (what goes out at the far side is empty).

After out and in the window is where it began and, with the store on, holds what it held.  Needs the
GPU: there is no fallback.
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
    hw, step, reps = W * H, cfg.dense_follow_step, args.reps
    h.tsdf_follow(margin=cfg.dense_follow_margin, step=step)

    def integrate():
        h.tsdf_integrate_rgbd(dev.data_ptr(), dev.data_ptr() + 3 * hw, 5 * hw, B, first_frame=0, stream=s)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(n):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / n   # us per call

    def trial(on: bool) -> dict:
        """nomove, out and in with the store on or off; the window ends where it began."""
        h.tsdf_store_init(cfg.dense_store_bricks if on else 0)
        integrate()
        out = {"nomove": timed(integrate, reps)}
        out["out"] = timed(lambda: h.tsdf_shift((step, 0, 0), stream=s), reps)
        stats = h.tsdf_store_stats() if on else None
        out["in"] = timed(lambda: h.tsdf_shift((-step, 0, 0), stream=s), reps)
        return out, stats, (h.tsdf_store_stats() if on else None)

    for on in (True, False):                                        # warm-up (code objects, first touch)
        trial(on)
    res = {f"{k}_{tag}": [] for k in ("nomove", "out", "in") for tag in ("on", "off")}
    away = back = None
    for _ in range(3):
        for on, tag in ((True, "on"), (False, "off")):
            t, a, b = trial(on)
            for k, v in t.items():
                res[f"{k}_{tag}"].append(v)
            if on:
                away, back = a, b
    shift = h.tsdf_window()[0].tolist()
    h.close()

    best = {k: min(v) for k, v in res.items()}
    out = {
        "what": "brick store behind the rolling window: HIP events around %d back-to-back calls after a warm-up, three "
                "trials, store on and off alternated, one handle, one session" % reps,
        "width": W, "height": H, "frames_per_call": B, "tracked_frames": tracked, "poses": "device",
        "volume_dims": list(cfg.tsdf_dims), "voxel_size_m": cfg.voxel_size, "color_layer": True, "step_voxels": step,
        "store_bricks": cfg.dense_store_bricks, "window_shift_at_the_end": shift,
        "store_after_the_moves_out": away, "store_after_the_moves_back": back,
        "us_per_call_trials": {k: [round(t, 1) for t in v] for k, v in res.items()},
        "us_per_call": {k: round(t, 1) for k, t in best.items()},
        "nomove_on_minus_off_us": round(best["nomove_on"] - best["nomove_off"], 1),
        "out_on_over_off": round(best["out_on"] / best["out_off"], 2),
        "in_on_over_off": round(best["in_on"] / best["in_off"], 2),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
