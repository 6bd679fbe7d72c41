"""What a view of the dense map costs (tslam_tsdf_render, k_tsdf_render.hip).

    python tools/tsdf_render_probe.py [--frames 16] [--reps 10] [--out profiles/tsdf_render_probe.json]

The default volume of HipSlamConfig (200 x 80 x 220 voxels of 0.05 m) with the colour layer, filled as
tools/tsdf_follow_probe.py fills it: one RGB-D camera at 640x480, `frames` frames integrated on the
tracked device poses.  Views of that camera (640x480, all four outputs) at the batch's tracked poses.
On one handle, in one run, HIP events around `reps` back-to-back calls after a warm-up, three trials,
the cases alternated:

  render_1     one view per call, at frame 0's pose,
  render_16    `frames` views per call, at the batch's device poses (us per view = call / views),
  mesh         tslam_mesh_extract on the same volume (count, one small read back, emit; no copy of
               the triangles to the host),
  integrate_1  tslam_tsdf_integrate_rgbd of one frame,

the last two being the existing costs a user weighs a view against.  The reference
(thor_slam_amd/dense_render.py) on the read-back volume gives the samples per ray of the render_1
view; 64 bytes are gathered per sample (eight tsdf and eight weights), which gives the implied gather
rate.  Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import ctypes
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

    from thor_slam_amd import dense_render as DR
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
    poses = h.read_poses(B)
    tracked = int((poses["stats"][:, 0, 0] == 0).sum())
    h.tsdf_color(True)
    h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
    hw = W * H
    h.tsdf_integrate_rgbd(dev.data_ptr(), dev.data_ptr() + 3 * hw, 5 * hw, B, first_frame=0, stream=s)
    cam = (W, H, rect.fx, rect.fy, rect.cx, rect.cy)
    prm = dict(min_weight=cfg.mesh_integrator_min_weight, min_depth=0.0, max_depth=cfg.tsdf_integrator_max_integration_distance_m,
               step_scale=cfg.dense_view_step_scale)
    h.tsdf_render_init(*cam, max_views=B, **prm)
    T0 = poses["T_abs"][0, 0]

    # the reference's samples per ray for the render_1 view, and the device's image against it
    tsdf, weight = h.tsdf_read()
    col, cw = h.tsdf_read_color()
    ref = DR.render_view(tsdf, weight, cfg.tsdf_origin, cfg.voxel_size, cam, T0, color=col, color_weight=cw, **prm)
    h.tsdf_render(T0[None], stream=s)
    got = h.tsdf_render_read(0)
    equal = bool(np.array_equal(got["depth_m"], ref["depth_m"]) and np.array_equal(got["color"], ref["color"]))
    samples = ref["samples"]
    normal_samples = 6 * int((ref["depth_m"] > 0).sum())

    n_tris = ctypes.c_int64()

    def mesh():
        h.lib.tslam_mesh_extract(h.h, float(cfg.mesh_integrator_min_weight), ctypes.byref(n_tris), ctypes.c_void_p(s))

    cases = {
        "render_1": lambda: h.tsdf_render(T0[None], stream=s),
        "render_16": lambda: h.tsdf_render(None, n_views=B, first_frame=0, stream=s),
        "mesh": mesh,
        "integrate_1": lambda: h.tsdf_integrate_rgbd(dev.data_ptr(), dev.data_ptr() + 3 * hw, 5 * hw, 1, first_frame=0, stream=s),
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
    total = int(samples.sum()) + normal_samples
    out = {
        "what": "a view of the dense map: HIP events around %d back-to-back calls after a warm-up, three trials, the cases "
                "alternated, one handle, one session" % args.reps,
        "width": W, "height": H, "frames_integrated": B, "tracked_frames": tracked, "volume_dims": list(cfg.tsdf_dims),
        "voxel_size_m": cfg.voxel_size, "color_layer": True, "outputs": "depth_m, depth_mm, normal, color",
        "step_scale": cfg.dense_view_step_scale, "device_equals_reference": equal,
        "hit_fraction": round(float((ref["depth_m"] > 0).mean()), 4),
        "samples_per_ray_mean": round(float(samples.mean()), 2), "samples_per_ray_max": int(samples.max()),
        "rays_clipped_away": round(float((samples == 0).mean()), 4),
        "samples_per_view_with_normals": total,
        "us_per_call_trials": {k: [round(t, 1) for t in v] for k, v in res.items()},
        "us_per_call": {k: round(t, 1) for k, t in best.items()},
        "us_per_view": {"render_1": round(best["render_1"], 1), "render_16": round(best["render_16"] / B, 1)},
        "gathered_GBps": {"render_1": round(64 * total / (best["render_1"] * 1e-6) / 1e9, 1),
                          "render_16": round(64 * total / (best["render_16"] / B * 1e-6) / 1e9, 1)},
        "gathered_GBps_note": "64 B per sample of the render_1 view; render_16's other views are close to it, not equal",
        "mesh_triangles": int(n_tris.value),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
