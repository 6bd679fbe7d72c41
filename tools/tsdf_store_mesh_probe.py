"""What the mesh of the whole dense map costs (tslam_mesh_extract_whole, k_tsdf_store_mesh.hip) next
to the window's mesh (tslam_mesh_extract, k_dense.hip).

    python tools/tsdf_store_mesh_probe.py [--reps 12] [--slabs 4] [--out profiles/tsdf_store_mesh_probe.json]

The default volume of HipSlamConfig (200 x 80 x 220 voxels of 0.05 m) with the colour layer and the
default pool of 65,536 bricks.  The map is an analytic height field written with tslam_tsdf_write
(weight 1 within 4 voxels of the surface, 0 elsewhere), so the surface runs through the whole volume.

  same_voxels   shift 0, store on and empty: both calls mesh the same voxels.  `reps` calls of each,
                alternated, after a warm-up; wall time of the call (it waits for the triangle count)
                and of the call plus a device synchronise (the emit kernel has ended): medians, min
                and max.
  after_drive   `slabs` times: write the height field at the window's place, move the window on by
                its whole x extent (every voxel goes to the store); then `reps` whole-map calls with
                the brick and triangle counts.

Needs the GPU: there is no fallback.
"""

from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--slabs", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import ctypes

    import numpy as np
    import torch

    from thor_slam_amd._lib import Handle, _check
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    cfg = HipSlamConfig(rgbd=True)
    src = SyntheticRGBDSource(width=640, height=480)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    h = Handle([rgbd_undistort(cams[ci])], cfg, max_batch=2)
    h.tsdf_color(True)
    h.tsdf_init(cfg.tsdf_origin, cfg.tsdf_dims, cfg.voxel_size, cfg.tsdf_integrator_truncation_distance_vox,
                cfg.tsdf_integrator_max_integration_distance_m, cfg.tsdf_max_weight)
    h.tsdf_store_init(cfg.dense_store_bricks)
    nx, ny, nz = cfg.tsdf_dims
    s, minw = cfg.voxel_size, cfg.mesh_integrator_min_weight

    def field(x0: int):
        """The height field over the window whose first absolute x voxel is x0."""
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        x, z = (i + x0) * s, k * s
        d = (j - (0.5 * ny + 0.3 * ny * np.sin(0.9 * x) * np.cos(0.7 * z))) * s
        seen = np.abs(d) < 4 * s
        tsdf = np.where(seen, np.clip(d, -4 * s, 4 * s), 0.0).astype(np.float32)
        color = np.where(seen[..., None], np.stack([i % 251, j % 251, k % 251], axis=-1), 0).astype(np.float32)
        return tsdf, seen.astype(np.float32), color

    def write(x0: int):
        t, w, c = field(x0)
        h.tsdf_write(t, w)
        h.tsdf_write_color(c, w)

    def call(whole: bool):
        """(us until the call returns, us until the device is idle, triangles, bricks)"""
        n, nb = ctypes.c_int64(), ctypes.c_int64()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if whole:
            _check(h.lib.tslam_mesh_extract_whole(h.h, minw, ctypes.byref(n), ctypes.byref(nb), None))
        else:
            _check(h.lib.tslam_mesh_extract(h.h, minw, ctypes.byref(n), None))
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return 1e6 * (t1 - t0), 1e6 * (t2 - t0), int(n.value), int(nb.value)

    def summary(rows):
        out = {}
        for name, col in (("call_us", 0), ("call_and_sync_us", 1)):
            v = [r[col] for r in rows]
            out[name] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
        out["triangles"], out["bricks"] = rows[-1][2], rows[-1][3]
        return out

    write(0)
    for _ in range(3):                                              # warm-up: code objects, the buffers' growth
        call(True), call(False)
    rows = {True: [], False: []}
    for _ in range(args.reps):
        for whole in (True, False):
            rows[whole].append(call(whole))
    same = {"whole": summary(rows[True]), "window": summary(rows[False])}
    same["whole_over_window"] = round(same["whole"]["call_and_sync_us"]["median"] / same["window"]["call_and_sync_us"]["median"], 2)
    tw = h.mesh_whole(minw)
    tm = h.mesh(minw)
    same["same_triangles"] = bool(len(tw) == len(tm) and np.array_equal(np.sort(tw.reshape(-1, 9).view(np.uint32), axis=0),
                                                                          np.sort(tm.reshape(-1, 9).view(np.uint32), axis=0)))
    for n in range(args.slabs):                                     # the drive
        if n:
            write(n * nx)
        h.tsdf_shift((nx, 0, 0))
    write(args.slabs * nx)
    stats = h.tsdf_store_stats()
    call(True)
    drive = summary([call(True) for _ in range(args.reps)])
    drive["store"] = stats
    window_after = summary([call(False) for _ in range(args.reps)])
    h.close()
    out = {"what": "tslam_mesh_extract_whole next to tslam_mesh_extract: wall time of %d calls each after a warm-up, alternated, "
                   "one handle, one session; an analytic height field through the whole volume" % args.reps,
           "volume_dims": list(cfg.tsdf_dims), "voxel_size_m": s, "color_layer": True, "store_bricks": cfg.dense_store_bricks,
           "same_voxels": same, "after_drive": {"slabs": args.slabs, "whole": drive, "window": window_after}}
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
