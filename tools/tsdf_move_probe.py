"""What moving archived depth frames costs (tslam_tsdf_archive_move, k_tsdf_move_frames.hip).

    python tools/tsdf_move_probe.py [--frames 256] [--reps 5] [--out profiles/tsdf_move_probe.json]

The default volume of HipSlamConfig (200 x 80 x 220 voxels of 0.05 m) and one rectified camera at
640 x 400.  `frames` analytic depth frames (a wall with a nearer box, seen from poses along an arc) are
integrated and archived; a move then sends every one of them to a pose 5 cm and 0.02 rad away, and
the next move sends them back, so every timed call selects all `frames` frames.  On one handle, in
one run, HIP events around `reps` back-to-back calls after a warm-up, three trials, the cases
alternated:

  move        tslam_tsdf_archive_move of all frames (selection, k_tsdf_reintegrate, the ring's poses),
  move_none   the same call with the poses the frames already have: nothing is selected,
  integrate   tslam_tsdf_integrate_rect of the same frames on host poses: the yardstick, a move
              being two integrations' worth of projection per frame.

There is no pass bar: nothing of the kind existed before.  Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))


def rot_y(a):
    import numpy as np

    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def render(T, W, H, fx, fy, cx, cy, wall_z=6.0, box=((-1.0, -0.5, 3.5), (0.5, 2.0, 6.0))):
    """Depth u16 mm of the wall z = wall_z and the box from world_T_cam T."""
    import numpy as np

    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones((H, W))], axis=-1) @ T[:3, :3].T
    C = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        best = (wall_z - C[2]) / d[..., 2]
        lo, hi = (np.array(box[0]) - C) / d, (np.array(box[1]) - C) / d
    near, far = np.minimum(lo, hi).max(axis=-1), np.maximum(lo, hi).min(axis=-1)
    best = np.where((near <= far) & (near > 0) & (near < best), near, best)
    return np.clip(np.rint(best * 1000.0), 0, 65535).astype(np.uint16)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import StereoRectification
    from thor_slam_amd.params import HipSlamConfig

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    W, H, N = args.width, args.height, args.frames
    fx = fy = 0.6 * W
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    cfg = HipSlamConfig(stereo_depth=True, dense_map=True, dense_loop=True, stereo_depth_interval=5)
    rect = StereoRectification(W, H, fx, fy, cx, cy, 0.075, np.eye(3), np.eye(3), None, None, True)
    poses_a = np.stack([np.eye(4)] * N)
    for i in range(N):
        a = 0.6 * (i / max(N - 1, 1) - 0.5)
        poses_a[i, :3, :3] = rot_y(a)
        poses_a[i, :3, 3] = (2.0 * a, 0.05 * np.sin(0.3 * i), 0.5 * np.cos(a) - 0.5)
    poses_b = poses_a.copy()
    for i in range(N):
        poses_b[i, :3, :3] = poses_a[i, :3, :3] @ rot_y(0.02)
        poses_b[i, :3, 3] += (0.03, -0.02, 0.035)
    depth = np.stack([render(T, W, H, fx, fy, cx, cy) for T in poses_a])
    dev = torch.from_numpy(depth.view(np.int16)).cuda()
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    h = Handle([rect], HipSlamConfig(n_features=256, n_levels=1), max_batch=1)
    h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
    h.tsdf_archive_init(capacity=N, rect=True)
    h.tsdf_archive_integrate(dev.data_ptr(), 2 * W * H, N, first_frame=0, world_T_cam=poses_a, stream=s)
    observed = int((h.tsdf_read()[1] > 0).sum())
    frames = np.arange(N)
    min_t, min_r = 0.5 * cfg.voxel_size, cfg.dense_loop_min_rotation_rad
    state = {"at_a": True}

    def move():
        h.tsdf_archive_move(frames, poses_b if state["at_a"] else poses_a, min_t, min_r, stream=s)
        state["at_a"] = not state["at_a"]

    def move_none():
        h.tsdf_archive_move(frames, poses_a if state["at_a"] else poses_b, min_t, min_r, stream=s)

    def integrate():
        h.tsdf_integrate_rect(dev.data_ptr(), 2 * W * H, N, first_frame=0, world_T_cam=poses_a, stream=s)

    cases = {"move": move, "move_none": move_none, "integrate": integrate}

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps   # ms per call

    moved = []
    for fn in cases.values():
        timed(fn, 2)                                  # warm-up (code objects, first touch)
    res = {k: [] for k in cases}
    for _ in range(3):
        for k, fn in cases.items():
            res[k].append(timed(fn, args.reps))
            if k != "integrate":
                moved.append((k, h.tsdf_archive_read(0)["moved_last"]))
    h.close()
    assert all(m == (N if k == "move" else 0) for k, m in moved), moved
    best = {k: min(v) for k, v in res.items()}
    out = {
        "what": "depth frames moved in the TSDF volume: HIP events around %d back-to-back calls after a warm-up, three trials, "
                "the cases alternated, one handle, one session" % args.reps,
        "width": W, "height": H, "frames": N, "volume_dims": list(cfg.tsdf_dims), "voxel_size_m": cfg.voxel_size,
        "observed_voxels": observed, "selected_per_move": N,
        "ms_per_call_trials": {k: [round(t, 3) for t in v] for k, v in res.items()},
        "ms_per_call": {k: round(t, 3) for k, t in best.items()},
        "us_per_frame": {k: round(1000.0 * t / N, 2) for k, t in best.items()},
        "move_over_integrate": round(best["move"] / best["integrate"], 2),
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
