"""Hand-made images for k_describe's keypoint list and its batched stores
(tests/test_describe_chain_cpu.py checks on the oracle alone that each does what it was chosen for,
tests/test_gpu_describe_chain.py runs them on the device).

k_describe serves a 128 x 64 tile of a level per block: it lists the tile's keypoints from the
y-sorted records of the tile's rows (at most LIST_CAP positions at a time), deals list entry g to
wave g % 8, and a wave stores the descriptors of eight keypoints at a time (and of what is left
after its last one).  The images here put chosen numbers of keypoints into chosen level-0 tiles:
single 255 pixels, each one keypoint and nothing else, on noise too weak for a corner of its own
(so that every keypoint has its own orientation and descriptor).
"""

from __future__ import annotations

import functools

import numpy as np

import frontend_cases as FC
from helpers import make_source, rig_calibration
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.params import HipSlamConfig

SIZES = {"w256": (256, 128), "w250": (250, 130)}   # both levels on 16-byte rows / neither (byte staging)
N_LEVELS = 2
N_FEATURES = 600          # level 0's quota (480) holds every dot of the fullest image
TILE_W, TILE_H, WAVES = 128, 64, 8
LIST_CAP = 512            # TS_DT_LIST (tslam_describe.h)
STEP = 5                  # dots this far apart: none lies on another's FAST circle or NMS neighbourhood
DOT = 255
# level-0 keypoints per tile (tx, ty) of the left and the right image of three frames.  A tile of n
# keypoints gives wave w ceil((n - w) / 8): 0 and 1 (n = 1), 1 (8), 2 and 1 (9), 8 (64: one full
# set of stores and nothing left), 9 and 8 (65), 9 (72), 17 and 16 (130: two full sets and one).
PLANS = (
    ({(0, 0): 1, (1, 0): 8, (0, 1): 9, (1, 1): 64}, {(0, 0): 65, (1, 0): 72, (0, 1): 130}),
    ({(0, 0): 72, (1, 0): 130, (0, 1): 1, (1, 1): 9}, {(0, 0): 8, (1, 0): 65, (0, 1): 64, (1, 1): 1}),
    ({(0, 0): 130, (1, 0): 9, (0, 1): 65, (1, 1): 8}, {(0, 0): 64, (1, 0): 1, (0, 1): 72, (1, 1): 130}),
)
WANTED_COUNTS = (1, 8, 9, 64, 65, 72)   # and one tile of >= 129
WANTED_PER_WAVE = (0, 1, 8, 9)          # and one wave of >= 17
BLANK_FROM = 58           # rows 58.. flat: the second tile row of level 0 holds no keypoint
# natural overflow: noise at 336 x 244 with a quota that keeps more than LIST_CAP records in the 64
# rows of a level-0 tile
OVERFLOW_SIZE, OVERFLOW_FEATURES = "G1", 3000


@functools.lru_cache(maxsize=None)
def rect_for(width: int, height: int):
    """Plain lens: the images reach the pyramid as they are."""
    cams = extract_cameras(rig_calibration(make_source(FC.SEED, width, height, distorted=False)), 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


def cfg_for() -> HipSlamConfig:
    return HipSlamConfig(n_features=N_FEATURES, n_levels=N_LEVELS)


def dots_image(width: int, height: int, plan: dict, seed: int, margin: int = 19) -> np.ndarray:
    """Noise of 86..94 (no FAST corner: the threshold is 20) with plan[(tx, ty)] dots in level-0 tile
    (tx, ty), row by row from the tile's first legal pixel."""
    img = np.random.default_rng(seed).integers(86, 95, (height, width), dtype=np.uint8)
    for (tx, ty), n in plan.items():
        xs = range(max(tx * TILE_W, margin), min((tx + 1) * TILE_W, width - margin), STEP)
        ys = range(max(ty * TILE_H, margin), min((ty + 1) * TILE_H, height - margin), STEP)
        spots = [(y, x) for y in ys for x in xs]
        assert n <= len(spots), f"tile {(tx, ty)}: room for {len(spots)} dots, {n} wanted"
        for y, x in spots[:n]:
            img[y, x] = DOT
    return img


def tile_counts(image_result: dict, level: int = 0) -> dict:
    """(tx, ty) -> keypoints of one oracle image in that tile of `level`."""
    kp, valid = image_result["kp"], np.asarray(image_result["valid"], dtype=bool)
    sel = valid & (kp["level"] == level)
    out: dict = {}
    for x, y in zip(kp["x"][sel], kp["y"][sel]):
        key = (int(x) // TILE_W, int(y) // TILE_H)
        out[key] = out.get(key, 0) + 1
    return out


def per_wave(n: int) -> list[int]:
    """Keypoints of each of a block's waves for a tile of n (list entry g goes to wave g % 8)."""
    return [(n - w + WAVES - 1) // WAVES if n > w else 0 for w in range(WAVES)]


def row_range_positions(image_result: dict, height: int, level: int = 0) -> list[int]:
    """Per tile row of `level`: the y-sorted records of its 64 rows (what a tile lists from)."""
    kp, valid = image_result["kp"], np.asarray(image_result["valid"], dtype=bool)
    y = kp["y"][valid & (kp["level"] == level)]
    return [int(((y >= r) & (y < r + TILE_H)).sum()) for r in range(0, height, TILE_H)]


def _scenario(width: int, height: int, cfg, frames: np.ndarray) -> dict:
    frames.setflags(write=False)
    rect = rect_for(width, height)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(rect, cfg, frames), "size": (width, height)}


@functools.lru_cache(maxsize=None)
def flush_scenario(size: str, n_frames: int = len(PLANS)) -> dict:
    """Frames of PLANS, repeated in turn up to n_frames (left and right differ, frame k + 1 differs
    from frame k in every tile)."""
    w, h = SIZES[size]
    one = [np.stack([dots_image(w, h, left, 10 + 2 * i), dots_image(w, h, right, 11 + 2 * i)])
           for i, (left, right) in enumerate(PLANS)]
    return _scenario(w, h, cfg_for(), np.stack([one[i % len(one)] for i in range(n_frames)]))


@functools.lru_cache(maxsize=None)
def blank_scenario(size: str) -> dict:
    """Dots in the right tile of the first tile row only and nothing from row BLANK_FROM on: level
    0's first tile has no keypoint of its own, its second tile row none at all."""
    w, h = SIZES[size]
    img = dots_image(w, h, {(1, 0): 20}, 20)
    img[BLANK_FROM:] = 90
    return _scenario(w, h, cfg_for(), np.stack([np.stack([img, img])] * 2))


@functools.lru_cache(maxsize=None)
def overflow_scenario() -> dict:
    w, h = FC.HAND_SIZES[OVERFLOW_SIZE]
    cfg = HipSlamConfig(n_features=OVERFLOW_FEATURES, n_levels=FC.HAND_LEVELS)
    one = FC.noise_pair(w, h)
    return _scenario(w, h, cfg, np.stack([one] * 2))


