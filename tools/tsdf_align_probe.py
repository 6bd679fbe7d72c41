"""What a dense frame-to-model alignment costs (tslam_tsdf_align, k_tsdf_align.hip).

    python tools/tsdf_align_probe.py [--frames 16] [--reps 10] [--out profiles/tsdf_align_probe.json]

The default volume of HipSlamConfig (200 x 80 x 220 voxels of 0.05 m), filled as
tools/tsdf_render_probe.py fills it: one RGB-D camera at 640x480, `frames` frames integrated on the
tracked device poses.  The same frames are then aligned to that map from their tracked device poses
with the default parameters.  On one handle, in one run, HIP events around `reps` back-to-back calls
after a warm-up, three trials, the cases alternated:

  align_1 / align_16          tslam_tsdf_align of one frame / of `frames` frames per call (the render
                              at T0 and iterations x (accumulate, solve)),
  align_1_it1 / align_16_it1  the same with iterations = 1: the render and one iteration, so that
                              (align - it1) / (iterations run - 1) is an iteration's cost,
  render_1 / render_16        tslam_tsdf_render of the same views, depth_m and normals only,
  integrate_1 / integrate_16  tslam_tsdf_integrate of the same frames,

the last four being what the same frames cost already.  A frame that converges early stops taking
part, so a call's time depends on the iterations its frames run: they are reported.  There is no pass
bar: nothing of the kind existed before.  Needs the GPU: there is no fallback.
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
    cfg = HipSlamConfig(rgbd=True, dense_map=True, dense_align=True)
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
    h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
    hw = W * H
    depth, stride = dev.data_ptr() + 3 * hw, 5 * hw
    h.tsdf_integrate(depth, stride, B, first_frame=0, stream=s)
    prm = cfg.dense_align_params()
    h.tsdf_render_init(W, H, rect.fx, rect.fy, rect.cx, rect.cy, min_weight=prm["min_weight"], min_depth=0.0,
                       max_depth=prm["max_depth"], step_scale=prm["step_scale"], max_views=B, outputs=5)

    def align(n, iterations):
        def run():
            h.tsdf_align(depth, stride, n, first_frame=0, stream=s)
        return iterations, run

    cases = {
        "align_1": align(1, prm["iterations"]), "align_16": align(B, prm["iterations"]),
        "align_1_it1": align(1, 1), "align_16_it1": align(B, 1),
        "render_1": (None, lambda: h.tsdf_render(None, n_views=1, first_frame=0, stream=s)),
        "render_16": (None, lambda: h.tsdf_render(None, n_views=B, first_frame=0, stream=s)),
        "integrate_1": (None, lambda: h.tsdf_integrate(depth, stride, 1, first_frame=0, stream=s)),
        "integrate_16": (None, lambda: h.tsdf_integrate(depth, stride, B, first_frame=0, stream=s)),
    }
    state = {"iterations": None}

    def prepare(iterations):
        if iterations is not None and state["iterations"] != iterations:   # init synchronises: outside the timed span
            h.tsdf_align_init(pair=0, rect=False, max_frames=B, **{**prm, "iterations": iterations})
            state["iterations"] = iterations

    def timed(case, reps):
        iterations, fn = case
        prepare(iterations)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps   # us per call

    # what the alignment does on these frames (the volume as integrated above, before the timed
    # integrate calls add to it)
    prepare(prm["iterations"])
    cases["align_16"][1]()
    report = h.tsdf_align_read()
    res = {k: [] for k in cases}
    for case in cases.values():
        timed(case, 2)                                # warm-up (code objects, first touch)
    for _ in range(3):
        for k, case in cases.items():
            res[k].append(timed(case, args.reps))
    h.close()

    best = {k: min(v) for k, v in res.items()}
    out = {
        "what": "dense frame-to-model alignment: HIP events around %d back-to-back calls after a warm-up, three trials, the "
                "cases alternated, one handle, one session" % args.reps,
        "width": W, "height": H, "frames": B, "tracked_frames": tracked, "volume_dims": list(cfg.tsdf_dims),
        "voxel_size_m": cfg.voxel_size, "parameters": prm,
        "status": report["stats"][:, 0].tolist(), "iterations_run": report["stats"][:, 1].tolist(),
        "inliers_first_last": report["stats"][:, 2:].tolist(),
        "rms_first_last_mm": [[round(1e3 * float(v), 3) for v in r] for r in report["residuals"]],
        "us_per_call_trials": {k: [round(t, 1) for t in v] for k, v in res.items()},
        "us_per_call": {k: round(t, 1) for k, t in best.items()},
        "us_per_frame": {k: round(t / (B if k.split("_")[1] == "16" else 1), 1) for k, t in best.items()},
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
