"""Hand-made images for detect's flush rounds (pooled tails) and its smoothing edge columns
(tests/test_detect_tails_cpu.py checks on the oracle alone that each does what it was chosen for,
tests/test_gpu_detect_tails.py runs them on the device).

k_detect deals the (row, quad) items of a band block to 8 waves (item `it` to wave (it % 512) / 64);
a wave flushes its candidate queue 64 entries at a time inside its loop and is left with a tail
(phase B pools the tails of the block's waves into rounds of 64).  tools/detect_tail_sim.py restates
the dealing; the images here put chosen numbers of entries into chosen waves.
"""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np

import frontend_cases as FC
from helpers import make_source, rig_calibration
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.params import HipSlamConfig

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import detect_tail_sim as SIM  # noqa: E402

# id -> (W, H, n_levels, n_features)
GEOMETRIES = {
    "T64": (64, 64, 1, 100),      # the smallest legal image: fewer than 64 items per wave, every round a tail
    "T72": (128, 72, 1, 300),     # last band 8 rows: shorter than a smoothing row group, so the second group is empty
    "T128": (128, 96, 1, 300),
    "T336": (336, 244, 3, 600),   # packed paths at every level, several bands, last bands short
    "T332": (332, 250, 3, 600),   # level 0 dword rows without LDS-DMA; levels 1, 2 scalar (they queue nothing)
}
N_FRAMES = 3
FLAT = 90
DOT = 255

# per band of level 0 of T336 (32 rows each): wave -> queue entries.  Per-wave tails of 0 (64 and
# 128: emptied exactly by the flushes inside the loop), 1 (65), 2, 32, 33 and 63; per-block tail
# totals of 128, 63, 0, 1, 0, 64 and 65.
PLAN = {
    0: {0: 63, 3: 63, 6: 2},
    1: {1: 63},
    2: {2: 64},
    3: {3: 65},
    4: {4: 128},
    5: {0: 32, 5: 32},
    6: {1: 32, 6: 33},
}


@functools.lru_cache(maxsize=None)
def rect_for(gid: str):
    """Plain lens: the images reach the pyramid as they are."""
    w, h, _, _ = GEOMETRIES[gid]
    cams = extract_cameras(rig_calibration(make_source(FC.SEED, w, h, distorted=False)), 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


def cfg_for(gid: str) -> HipSlamConfig:
    _, _, levels, features = GEOMETRIES[gid]
    return HipSlamConfig(n_features=features, n_levels=levels)


def both_image(width: int = 128, height: int = 96) -> np.ndarray:
    """Flat 128 with 110 pixel pairs, 255 at x = 4q and 0 at x = 4q + 2: the 255 has every circle
    pixel darker (score 127), the 0 every one brighter (score 128), so the quad is a candidate on
    both sides and both pixels survive the NMS."""
    img = np.full((height, width), 128, np.uint8)
    for y in range(20, 70, 5):
        for q in range(5, 27, 2):
            img[y, 4 * q] = 255
            img[y, 4 * q + 2] = 0
    return img


def item_position(width: int, height: int, br: int, margin: int, stage: str, band: int, it: int):
    """(y, quad) of item `it` of a band block in the phase-B (`dark` / `bright`) or `nms` dealing, or
    None where the stage would not queue a dot there or a neighbouring band would see it too."""
    y0 = band * br
    if stage == "nms":
        w4 = width // 4
        ylo, yhi = max(y0, margin), min(y0 + br, height - margin)
        y, q = ylo + it // w4, it % w4
        if y >= yhi or not (4 * q + 4 > margin and 4 * q < width - margin):
            return None
    else:
        qa, nq = (margin - 1) >> 2, ((width - margin) >> 2) + 1 - ((margin - 1) >> 2)
        ra, rb = max(0, margin - y0), min(br + 2, height - margin + 2 - y0)
        r, q = ra + it // nq, qa + it % nq
        y = y0 - 1 + r
        if r >= rb:
            return None
    if not (max(y0 + 1, margin) <= y <= min(y0 + br - 2, height - margin - 1)):
        return None   # rows y0 - 1, y0, y0 + br - 1, y0 + br are scored by two bands
    return y, q


def plan_image(stage: str, gid: str = "T336", plan: dict | None = None) -> np.ndarray:
    """Single 255 pixels on flat 90 (each one queue entry of its own quad and nothing else: dark
    side in phase B, a nonzero score word in the NMS), placed so that wave w of band b queues
    plan[b][w] entries of `stage`."""
    plan = PLAN if plan is None else plan
    w, h, levels, _ = GEOMETRIES[gid]
    margin = cfg_for(gid).edge_margin
    br = SIM.band_rows(w, h, levels)[0]
    img = np.full((h, w), FLAT, np.uint8)
    placed: list[tuple[int, int]] = []
    for band, waves in plan.items():
        for wave, n in waves.items():
            it = 64 * wave
            while n > 0:
                pos = item_position(w, h, br, margin, stage, band, it)
                assert it < (br + 2) * (w // 4), f"band {band} wave {wave}: no room for its entries"
                it += 1 if it % 64 != 63 else SIM.THREADS - 63
                if pos is None:
                    continue
                y, x = pos[0], 4 * pos[1] + 1
                if any(abs(y - py) <= 3 and abs(x - px) <= 3 for py, px in placed):
                    continue   # a dot on another's circle would change its neighbours' scores
                img[y, x] = DOT
                placed.append((y, x))
                n -= 1
    return img


def row_image(gid: str = "T336") -> np.ndarray:
    """One row of dots, 8 apart: the items of one row reach two of a block's waves only."""
    w, h, _, _ = GEOMETRIES[gid]
    img = np.full((h, w), FLAT, np.uint8)
    img[40, 21:w - 20:8] = DOT
    return img


def edges_image(gid: str) -> np.ndarray:
    """Noise in the first and last 8 columns of every level (8 << l at level 0), flat between."""
    w, h, levels, _ = GEOMETRIES[gid]
    n = 8 << (levels - 1)
    img = np.full((h, w), FLAT, np.uint8)
    rng = np.random.default_rng(104)
    img[:, :n] = rng.integers(0, 256, (h, n), dtype=np.uint8)
    img[:, w - n:] = rng.integers(0, 256, (h, n), dtype=np.uint8)
    return img


def image(gid: str, content: str) -> np.ndarray:
    w, h, _, _ = GEOMETRIES[gid]
    if content == "both":
        return both_image(w, h)
    if content in ("plan_dark", "plan_nms"):
        return plan_image(content[5:], gid)
    if content == "row":
        return row_image(gid)
    if content == "edges":
        return edges_image(gid)
    if content == "flat":
        return FC.flat_pair(w, h)[0]
    if content == "noise":
        return FC.noise_pair(w, h)[0]
    raise KeyError(content)


# (geometry, content): what the device tests run
CASES = [
    ("T128", "both"), ("T336", "plan_dark"), ("T336", "plan_nms"), ("T64", "flat"), ("T336", "flat"), ("T336", "row"),
    ("T64", "noise"), ("T128", "noise"), ("T336", "noise"), ("T332", "noise"),
    ("T72", "edges"), ("T336", "edges"), ("T332", "edges"),
]


@functools.lru_cache(maxsize=None)
def scenario(gid: str, content: str) -> dict:
    """Three repeated frames (left = right) with their oracle run (computed once, read-only)."""
    rect, cfg = rect_for(gid), cfg_for(gid)
    img = image(gid, content)
    frames = np.stack([np.stack([img, img])] * N_FRAMES)
    frames.setflags(write=False)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(rect, cfg, frames)}
