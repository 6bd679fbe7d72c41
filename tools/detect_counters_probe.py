"""k_detect's flush-round counters on a bench batch, beside the CPU restatement (profiling aid).

    python tools/detect_counters_probe.py [--batch 2048] [--sim-frames 32] [--out FILE.json]

Runs two batches of the C2 bench frames so the thresholds are learnt, switches counting on
(`tslam_detect_counters`), runs a third batch and reads its counters; then runs the first
--sim-frames frames again as a batch of their own under the thresholds in use and counts the same
images with tools/detect_tail_sim.py (oracle, CPU).  Prints and writes both, per level and in all.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd", ROOT / "tools"):
    sys.path.insert(0, str(p))


def _totals(levels: list) -> dict:
    import detect_tail_sim as SIM

    out = {s: {k: sum(lev[s][k] for lev in levels) for k in levels[0][s]} for s in SIM.STAGES}
    out["blocks"] = sum(lev["blocks"] for lev in levels)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--sim-frames", type=int, default=32)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import detect_tail_sim as SIM
    from bench import render_frames, triangle_indices
    from oracle import numpy_slam as O
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticStereoSource

    src = SyntheticStereoSource(seed=0, width=640, height=400)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    rect = stereo_rectify(cams[li], cams[ri])
    cfg = HipSlamConfig(n_features=args.features)
    B, S, L = args.batch, args.sim_frames, cfg.n_levels
    uniq = render_frames(0, 48, 8)
    frames = uniq[triangle_indices(2 * B, len(uniq))]
    dev = torch.from_numpy(frames).cuda()
    h = Handle([rect], cfg, max_batch=B)
    s = torch.cuda.current_stream().cuda_stream
    h.submit(dev[:B].data_ptr(), B, s)
    h.submit(dev[B:].data_ptr(), B, s)
    h.read_poses(B)
    h.detect_counters()   # counting on
    h.submit(dev[:B].data_ptr(), B, s)
    h.read_poses(B)
    batch = h.detect_counters()
    tfull = cfg.fast_threshold + 1
    te = np.maximum(h.frame_block("det_thr", 0, np.uint32)[:2 * L].reshape(2, L), tfull)
    h.submit(dev[:S].data_ptr(), S, s)
    h.read_poses(S)
    small = h.detect_counters()
    fails = [h.frame_block("det_fail", f, np.uint32)[:2 * L].reshape(2, L) for f in range(S)]
    h.close()
    want = None
    for f in range(S):
        for cam, mp in enumerate((rect.map_left, rect.map_right)):
            levels = O.pyramid(O.remap(frames[f, cam], mp), L)
            want = SIM.add_rounds(want, SIM.pyramid_rounds(levels, te[cam], cfg.edge_margin))
            flagged = [l for l in range(L) if fails[f][cam, l]]
            if flagged:
                want = SIM.add_rounds(want, SIM.pyramid_rounds(levels, [tfull] * L, cfg.edge_margin), levels=flagged)
    equal = all(small[l][st][k] == want[l][st][k] for l in range(L) for st in SIM.STAGES for k in small[l][st]) and \
        all(small[l]["blocks"] == want[l]["blocks"] for l in range(L))
    res = {
        "te_per_camera_level": te.tolist(),
        "batch_frames": B, "batch_counters": batch, "batch_totals": _totals(batch),
        "sim_frames": S, "device_counters": small, "device_totals": _totals(small),
        "simulation": want, "simulation_totals": _totals(want), "device_equals_simulation": equal,
    }
    t = res["simulation_totals"]
    per = 2 * S
    print("te", te.tolist())
    print("per image, %d frames: phase B rounds %.1f with every wave's own tail, %.1f pooled; NMS %.1f, %.1f pooled" % (
        S, sum(t[st]["inloop"] + t[st]["partial"] for st in ("bright", "dark")) / per,
        sum(t[st]["inloop"] + t[st]["pooled"] for st in ("bright", "dark")) / per,
        (t["nms"]["inloop"] + t["nms"]["partial"]) / per, (t["nms"]["inloop"] + t["nms"]["pooled"]) / per))
    print("device == simulation on %d frames: %s" % (S, equal))
    print("batch of %d: %s" % (B, json.dumps(res["batch_totals"])))
    if args.out:
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
