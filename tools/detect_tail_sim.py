"""k_detect's flush rounds restated on the CPU (oracle only, no GPU).

    python tools/detect_tail_sim.py [--width 640 --height 400 --levels 4 --features 2000]
                                    [--seed 0 --frame 2 --cam 0] [--te 55,68,62,27]

k_detect deals the (row, quad) items of a band block to its 8 waves, item `it` to wave
(it % 512) / 64.  A wave queues its candidate quads (phase B: bright and dark side apart; NMS: the
quads with a nonzero score word), flushes 64 at a time inside its loop and is left with a tail of
fewer than 64.  Phase B pools the tails of a block's waves into rounds of 64; an NMS tail is
flushed by its wave.  This tool counts, per level and stage, the rounds inside the loops, the rounds
the tails make pooled per block (`pooled`) and flushed by every wave on its own (`partial`), and the
lanes they fill: `tslam_detect_counters` returns inloop / pooled / lanes for phase B and inloop /
partial / lanes for the NMS of the same image and thresholds (tests/test_gpu_detect_tails.py
compares them).

Without --te the thresholds are learnt as the device learns them, from the frames before --frame
(per level 2 below the K-th survivor's score, the minimum over the frames, t + 1 where a level
comes short of its quota).  Only the packed (dword-row) paths with edge_margin >= 7 queue anything;
other levels count zero.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

from oracle import numpy_slam as O  # noqa: E402

THREADS, WAVES, ROUND = 512, 8, 64
BAND_ROWS_MAX = 32
STAGES = ("bright", "dark", "nms")


def band_rows(width: int, height: int, n_levels: int) -> list[int]:
    """Detect's band height per level (build_geometry in tslam_api.cpp)."""
    wh = O.level_shapes(width, height, n_levels)
    w0 = wh[0][0]
    br0 = BAND_ROWS_MAX if (2 * BAND_ROWS_MAX + 10) * w0 <= 48 * 1024 else 24 if (2 * 24 + 10) * w0 <= 78 * 1024 else 16
    budget = (2 * br0 + 10) * w0
    out = []
    for l, (w, h) in enumerate(wh):
        if l == 0:
            out.append(br0)
            continue
        maxr = max(br0, min(124, (budget // w - 10) // 2))
        nb = (h + maxr - 1) // maxr
        out.append(((h + nb - 1) // nb + 1) & ~1)
    return out


def packed_levels(width: int, height: int, n_levels: int) -> list[bool]:
    """Levels on detect's dword paths: W % 4 == 0 and the level's pyramid offset % 4 == 0."""
    off, out = 0, []
    for w, h in O.level_shapes(width, height, n_levels):
        out.append(w % 4 == 0 and off % 4 == 0)
        off += w * h
    return out


def _zero() -> dict:
    z = {s: {"inloop": 0, "pooled": 0, "lanes": 0, "partial": 0} for s in STAGES}
    z["blocks"] = 0
    return z


def _add_block(acc: dict, stage: str, per_wave: np.ndarray) -> None:
    """One block's queue totals per wave -> rounds."""
    tails = per_wave % ROUND
    acc[stage]["inloop"] += int((per_wave // ROUND).sum())
    acc[stage]["lanes"] += int(tails.sum())
    acc[stage]["pooled"] += int((tails.sum() + ROUND - 1) // ROUND)
    acc[stage]["partial"] += int((tails > 0).sum())


def _per_wave(flags: np.ndarray) -> np.ndarray:
    """Items in dealing order (raster over the block's item rectangle) -> queued items per wave."""
    it = np.flatnonzero(flags.ravel())
    return np.bincount((it % THREADS) // ROUND, minlength=WAVES)


def phase_a_quads(level: np.ndarray, te: int) -> tuple[np.ndarray, np.ndarray]:
    """fast4_any per quad: [H][W // 4] bools, some pixel of the quad passes the compass test at te
    on the bright / dark side (pixels with the circle outside the image: False; detect never asks)."""
    h, w = level.shape
    im = level.astype(np.int32)
    b = np.zeros((h, w), bool)
    d = np.zeros((h, w), bool)
    c = im[3:h - 3, 3:w - 3]
    up, dn = im[0:h - 6, 3:w - 3], im[6:h, 3:w - 3]
    rt, lf = im[3:h - 3, 6:w], im[3:h - 3, 0:w - 6]
    b[3:h - 3, 3:w - 3] = np.minimum(np.maximum(up, dn), np.maximum(rt, lf)) >= c + te
    d[3:h - 3, 3:w - 3] = np.maximum(np.minimum(up, dn), np.minimum(rt, lf)) <= c - te
    w4 = w // 4
    return b[:, :4 * w4].reshape(h, w4, 4).any(2), d[:, :4 * w4].reshape(h, w4, 4).any(2)


def level_queues(level: np.ndarray, te: int, br: int, margin: int) -> list[dict]:
    """Per band block of one packed level at threshold te (band height br): the entries each of
    the 8 waves queues in all, per stage."""
    if margin < 7:
        raise ValueError("edge_margin < 7 takes detect's border path, which this tool does not restate")
    h, w = level.shape
    w4 = w // 4
    qb, qd = phase_a_quads(level, te)
    sc = O.fast_scores(level)
    nzq = np.where(sc >= te, sc, 0)[:, :4 * w4].reshape(h, w4, 4).any(2)
    q = np.arange(w4)
    nzq &= ((4 * q + 4 > margin) & (4 * q < w - margin))[None, :]
    qa, nq = (margin - 1) >> 2, ((w - margin) >> 2) + 1 - ((margin - 1) >> 2)
    none = np.zeros(WAVES, np.int64)
    blocks = []
    for y0 in range(0, h, br):
        ra, rb = max(0, margin - y0), min(br + 2, h - margin + 2 - y0)
        rows = slice(y0 - 1 + ra, y0 - 1 + rb)
        ylo, yhi = max(y0, margin), min(y0 + br, h - margin)
        blocks.append({
            "bright": _per_wave(qb[rows, qa:qa + nq]) if rb > ra else none,
            "dark": _per_wave(qd[rows, qa:qa + nq]) if rb > ra else none,
            "nms": _per_wave(nzq[ylo:yhi]) if yhi > ylo else none,
        })
    return blocks


def level_rounds(level: np.ndarray, te: int, br: int, margin: int) -> dict:
    """The rounds of one packed level at threshold te (band height br)."""
    acc = _zero()
    for blk in level_queues(level, te, br, margin):
        acc["blocks"] += 1
        for s in STAGES:
            _add_block(acc, s, blk[s])
    return acc


def pyramid_rounds(levels: list[np.ndarray], te: list[int], margin: int) -> list[dict]:
    """Per level the rounds of one image's pyramid; te[l] the threshold in use (>= t + 1)."""
    h, w = levels[0].shape
    br = band_rows(w, h, len(levels))
    packed = packed_levels(w, h, len(levels))
    return [level_rounds(lev, int(te[l]), br[l], margin) if packed[l] else _zero() for l, lev in enumerate(levels)]


def image_rounds(img0: np.ndarray, te: list[int], n_levels: int, margin: int) -> list[dict]:
    """pyramid_rounds of a rectified level-0 image."""
    return pyramid_rounds(O.pyramid(img0, n_levels), te, margin)


def add_rounds(total: list[dict] | None, more: list[dict], levels=None) -> list[dict]:
    """total += more (the levels in `levels`, default all)."""
    if total is None:
        total = [_zero() for _ in more]
    for l, (t, m) in enumerate(zip(total, more)):
        if levels is not None and l not in levels:
            continue
        for s in STAGES:
            for k in t[s]:
                t[s][k] += m[s][k]
        t["blocks"] += m["blocks"]
    return total


def learnt_te(images: list[np.ndarray], cfg) -> list[int]:
    """The next batch's te per level after a batch of these rectified images of one camera."""
    quotas = O.level_quotas(cfg.n_features, cfg.n_levels)
    te = [255] * cfg.n_levels
    for img in images:
        for l, lev in enumerate(O.pyramid(img, cfg.n_levels)):
            s = np.sort(O.decode_keys(O.nms_keys(O.fast_scores(lev), cfg.fast_threshold, cfg.edge_margin))[2])[::-1]
            nxt = cfg.fast_threshold + 1
            if s.size >= quotas[l] and quotas[l] > 0:
                nxt = max(nxt, int(s[quotas[l] - 1]) - 2)
            te[l] = min(te[l], nxt)
    return te


def table(levels: list[dict]) -> str:
    s = _zero()
    for lev in levels:
        add_rounds([s], [lev])
    rows = [("level", "blocks") + tuple(f"{st} {k}" for st in STAGES for k in ("inloop", "partial", "pooled", "lanes"))]
    for name, lev in [(str(l), lev) for l, lev in enumerate(levels)] + [("all", s)]:
        rows.append((name, str(lev["blocks"])) + tuple(str(lev[st][k]) for st in STAGES for k in ("inloop", "partial", "pooled", "lanes")))
    wid = [max(len(r[i]) for r in rows) for i in range(len(rows[0]))]
    lines = ["  ".join(c.rjust(n) for c, n in zip(r, wid)) for r in rows]
    b_now = sum(s[st]["inloop"] + s[st]["partial"] for st in ("bright", "dark"))
    b_pool = sum(s[st]["inloop"] + s[st]["pooled"] for st in ("bright", "dark"))
    n_now, n_pool = s["nms"]["inloop"] + s["nms"]["partial"], s["nms"]["inloop"] + s["nms"]["pooled"]
    lines.append(f"phase B rounds: every wave its own tail {b_now}, pooled {b_pool}; NMS rounds: {n_now}, pooled {n_pool}")
    return "\n".join(lines)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--frame", type=int, default=2, help="index of the rendered frame that is counted")
    ap.add_argument("--cam", type=int, default=0, help="0: left, 1: right")
    ap.add_argument("--te", default="", help="thresholds per level, comma separated (default: learnt from the frames before)")
    args = ap.parse_args()
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticStereoSource

    cfg = HipSlamConfig(n_features=args.features, n_levels=args.levels)
    src = SyntheticStereoSource(seed=args.seed, width=args.width, height=args.height)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    rect = stereo_rectify(cams[li], cams[ri])
    mp = rect.map_left if args.cam == 0 else rect.map_right
    frames = src.render_stereo_sequence(args.frame + 1)
    imgs = [O.remap(fr[args.cam], mp) for fr in frames]
    te = [int(v) for v in args.te.split(",")] if args.te else (
        learnt_te(imgs[:-1], cfg) if args.frame > 0 else [cfg.fast_threshold + 1] * args.levels)
    print(f"{args.width} x {args.height}, {args.levels} levels, frame {args.frame} cam {args.cam}, te {te}, "
          f"band rows {band_rows(args.width, args.height, args.levels)}")
    print(table(image_rounds(imgs[-1], te, args.levels, cfg.edge_margin)))


if __name__ == "__main__":
    main()
