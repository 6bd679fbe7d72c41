"""Time the rig's dense-map launch (tslam_tsdf_integrate_rig, k_tsdf.hip) against one launch per camera.

    python tools/tsdf_rig_probe.py [--frames 64] [--reps 10] [--out profiles/tsdf_rig_c5.json]

C5 geometry: the 4-camera RGB-D bracket rig at 1280x720, the bench's TSDF volume (176 x 72 x 176
voxels of 0.05 m), the colour layer on, host poses (the ground-truth body poses of the synthetic
trajectory), `frames` frames per call (64 x 4 cameras = 256 views: one launch).  On the same handle,
the same device records and the same poses it times

  rig          one tslam_tsdf_integrate_rig over the four cameras, and
  per_camera   four tslam_tsdf_integrate_rgbd calls, camera after camera, each on that camera's
               world_T_cam = (E_0^-1 T) E_p (what the rig launch computes on the device),

each between two HIP events around `reps` back-to-back calls after a warm-up, three trials, in one
session.  Host poses make every call wait for its staged poses (one stream synchronisation per
launch), on both sides alike.  The volume keeps integrating across the calls: the weights run into
max_weight on both sides, the voxel traffic does not depend on that.  `--unique` distinct frames
are rendered and replayed as a triangle wave.

Bytes that must move per call (what the algorithm cannot avoid): every touched voxel's tsdf and
weight read and written once per LAUNCH (16 B; 48 B with the colour layer), so the per-camera route
pays that once per camera, and each view's pixels that a voxel looks up (depth 2 B + BGR 3 B per
pixel at most, once per view on both routes).  The per-camera route also integrates camera-major, so
its volume differs from the rig's beyond rounding as soon as a weight reaches max_weight; the probe
reports how far the two volumes are apart after ONE call each on a fresh volume.
Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))

NAMES = ("192.168.2.21", "192.168.2.22", "192.168.2.23", "192.168.2.25")
TSDF_ORIGIN = (-7.2, -1.8, -4.4)      # bench.py's C5 volume
TSDF_DIMS = (176, 72, 176)
HBM_PEAK_TBS = 8.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4, help="distinct rendered frames, replayed in a triangle wave")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    from thor_slam_amd import dense_rig
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.rgbd import pack_rgbd
    from thor_slam_amd.synthetic import synthetic_rgbd_rig

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    W, H, B, U = args.width, args.height, args.frames, max(1, min(args.unique, args.frames))
    joints = json.loads((ROOT / "tests" / "golden" / "brackets_joints.json").read_text())
    srcs, rig = synthetic_rgbd_rig(joints, NAMES, W, H)
    cams = extract_cameras(rig.calibration, 2 * len(NAMES))
    pairs = rgbd_pairs(cams)
    rects = [rgbd_undistort(cams[c]) for c, _ in pairs]
    E = [cams[c].extrinsics.to_4x4_matrix() @ r.left_optical_T_rect() for (c, _), r in zip(pairs, rects)]
    by_name = {s.name: s for s in srcs}
    P, hw = len(pairs), W * H
    tri = [i if i < U else 2 * (U - 1) - i for i in (k % max(1, 2 * (U - 1)) for k in range(B))]   # 0 1 2 3 2 1 0 ...
    uniq = np.stack([np.stack([pack_rgbd(*by_name[cams[c].source_name].render_rgbd(i)) for c, _ in pairs]) for i in range(U)])
    dev = torch.from_numpy(uniq).cuda()[torch.tensor(tri, device="cuda")].contiguous()          # [B][P][5 hw]
    traj = srcs[0].trajectory
    inv0 = np.linalg.inv(traj[0])
    wtb = np.stack([inv0 @ traj[i] for i in tri])
    wtc = [np.stack([dense_rig.rig_world_T_cam(E, T, p) for T in wtb]) for p in range(P)]

    h = Handle(rects, HipSlamConfig(rgbd=True), max_batch=1)
    h.set_rig(E)
    h.tsdf_color(True)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    base, stride = dev.data_ptr(), 5 * hw * P
    rig_cams = [dict(pair=p, depth=base + p * 5 * hw + 3 * hw, color=base + p * 5 * hw, stride_bytes=stride) for p in range(P)]

    def run_rig():
        h.tsdf_integrate_rig(rig_cams, B, world_T_base=wtb, stream=s)

    def run_per_camera():
        for p in range(P):
            h.tsdf_integrate_rgbd(base + p * 5 * hw, base + p * 5 * hw + 3 * hw, stride, B, world_T_cam=wtc[p], pair=p, stream=s)

    def fresh():
        h.tsdf_init(TSDF_ORIGIN, TSDF_DIMS, 0.05, 4.0, 10.0, 100.0)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps   # us per call

    # one call each on a fresh volume: what they observe, and how far apart the two orders end
    vols = {}
    for name, fn in (("rig", run_rig), ("per_camera", run_per_camera)):
        fresh()
        fn()
        vols[name] = h.tsdf_read() + h.tsdf_read_color()
    observed = int((vols["rig"][1] > 0).sum())
    colored = int((vols["rig"][3] > 0).sum())
    observed_alone = []
    for p in range(P):
        fresh()
        h.tsdf_integrate_rgbd(base + p * 5 * hw, base + p * 5 * hw + 3 * hw, stride, B, world_T_cam=wtc[p], pair=p, stream=s)
        observed_alone.append(int((h.tsdf_read()[1] > 0).sum()))

    res = {}
    for name, fn in (("rig", run_rig), ("per_camera", run_per_camera)):   # the two routes alternate per trial below
        fresh()
        timed(fn, 2)                                                       # warm-up (code object)
        res[name] = []
    for _ in range(3):
        for name, fn in (("rig", run_rig), ("per_camera", run_per_camera)):
            res[name].append(timed(fn, args.reps))
    h.close()

    nv = int(np.prod(TSDF_DIMS))
    views = B * P
    launches = {"rig": -(-B // dense_rig.chunk_frames(P)), "per_camera": P * -(-B // 256)}
    # touched voxels read and written once per launch: (tsdf, weight) 16 B, the colour layer 32 B more
    vox_bytes = {"rig": launches["rig"] * observed * 48, "per_camera": -(-B // 256) * sum(observed_alone) * 48}
    out = {
        "what": "tslam_tsdf_integrate_rig over %d cameras vs %d tslam_tsdf_integrate_rgbd calls, HIP events around %d "
                "back-to-back calls after a warm-up, three trials alternated, one session" % (P, P, args.reps),
        "width": W, "height": H, "cameras": P, "frames_per_call": B, "views_per_call": views, "unique_frames": U,
        "volume_dims": list(TSDF_DIMS), "volume_voxels": nv, "voxel_size_m": 0.05, "color_layer": True, "poses": "host",
        "launches_per_call": launches,
        "observed_voxels_after_one_call": observed, "colored_voxels_after_one_call": colored,
        "observed_voxels_each_camera_alone": observed_alone,
        "rig_us_per_call_trials": [round(t, 1) for t in res["rig"]],
        "per_camera_us_per_call_trials": [round(t, 1) for t in res["per_camera"]],
        "rig_us_per_call": round(min(res["rig"]), 1),
        "per_camera_us_per_call": round(min(res["per_camera"]), 1),
        "rig_over_per_camera": round(min(res["rig"]) / min(res["per_camera"]), 3),
        "rig_us_per_view": round(min(res["rig"]) / views, 2),
        "voxel_state_bytes_per_call": vox_bytes,
        "image_bytes_per_call_at_most": views * hw * 5,
        "rig_vs_per_camera_after_one_call": {
            "weight_equal": bool(np.array_equal(vols["rig"][1], vols["per_camera"][1])),
            "tsdf_max_abs_diff_m": float(np.abs(vols["rig"][0] - vols["per_camera"][0]).max()),
            "color_max_abs_diff": float(np.abs(vols["rig"][2] - vols["per_camera"][2]).max()),
        },
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
