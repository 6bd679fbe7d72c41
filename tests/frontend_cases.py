"""Shapes and hand-made images for the front-end parity tests off the 16-byte grid
(tests/test_frontend_cases_cpu.py checks their preconditions on the oracle alone,
tests/test_gpu_geometry.py runs them on the device).

The front-end kernels choose their code path from the level geometry ("Supported
geometries"): ``level_paths`` restates those predicates from ``level_shapes`` and the pyramid
offsets, and ``EXPECTED_PATHS`` lists the pattern each geometry below was chosen for.
"""

from __future__ import annotations

import functools

import numpy as np

from helpers import make_source, rig_calibration, scenario
from oracle import numpy_slam as O
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.params import HipSlamConfig, level_quotas, level_shapes

# id -> (W, H, n_levels, n_features, distorted)
GEOMETRIES = {
    "G1": (336, 244, 3, 600, True),    # rectify byte path (336 % 64); levels 1, 2 dword rows without 16-byte rows
    "G2": (332, 250, 3, 600, False),   # level 0 dword without DMA; levels 1 (166), 2 (83) scalar; pyr_off[2] % 4 == 2
    "G3": (329, 251, 3, 600, True),    # odd pitch; level 1 (164) dword-wide but pyr_off[1] % 4 == 3; odd H
    "G4": (448, 330, 4, 600, True),    # W % 64 == 0 yet W[3] = 56 leaves rectify's wide path; level 3 is 56 x 41
    "G5": (2044, 64, 1, 600, False),   # quad index 510 of 511; rectify LDS 65,408 B; long padding
    "G6": (64, 2047, 1, 600, False),   # y up to 2027 in the keys; 64 bands; the smallest pitch
    "G7": (64, 64, 1, 100, False),     # the smallest legal image
    "G8": (83, 82, 2, 100, False),     # coarsest level exactly 41 x 41 = 2 * edge_margin + 3
    "G9": (2044, 88, 2, 600, True),    # rectify LDS 81,760 B (above 64 KiB), remapped; level 1 (1022) scalar at a long pitch
    "G10": (2047, 64, 1, 600, False),  # the widest image: scalar paths at pitch 2047, the 11-bit x of the keys
}
N_FRAMES = 3
SEED = 1


def cfg_items(gid: str) -> tuple:
    _, _, levels, features, _ = GEOMETRIES[gid]
    return (("n_features", features), ("n_levels", levels))


def geometry_scenario(gid: str) -> dict:
    """``helpers.scenario`` (frames, rectification, oracle run) of one geometry."""
    w, h, _, _, distorted = GEOMETRIES[gid]
    return scenario(seed=SEED, n=N_FRAMES, width=w, height=h, distorted=distorted, cfg_items=cfg_items(gid))


def pyramid_offsets(width: int, height: int, n_levels: int) -> list[int]:
    """Byte offset of every level inside one image's pyramid block (levels packed back to back;
    the block itself is padded to 16 bytes, so an image's base never changes these residues)."""
    off, out = 0, []
    for w, h in level_shapes(width, height, n_levels):
        out.append(off)
        off += w * h
    return out


def level_paths(width: int, height: int, n_levels: int) -> dict:
    """The path predicates of the front-end kernels: ``rectify_wide`` for the whole image and per
    level ``(dma, dword, describe_wide)`` = detect's LDS-DMA staging, detect's packed smoothing /
    FAST / NMS, describe's 16-byte tile staging."""
    wh = level_shapes(width, height, n_levels)
    off = pyramid_offsets(width, height, n_levels)
    rectify_wide = width % 64 == 0 and all(w % 16 == 0 and o % 16 == 0 for (w, _), o in zip(wh[1:], off[1:]))
    levels = [(w % 16 == 0 and o % 16 == 0, w % 4 == 0 and o % 4 == 0, w % 16 == 0 and o % 16 == 0)
              for (w, _), o in zip(wh, off)]
    return {"rectify_wide": rectify_wide, "levels": levels}


T, F = True, False
# per level (dma, dword, describe_wide); what each geometry was chosen to flip
EXPECTED_PATHS = {
    "G1": {"rectify_wide": F, "levels": [(T, T, T), (F, T, F), (F, T, F)]},
    "G2": {"rectify_wide": F, "levels": [(F, T, F), (F, F, F), (F, F, F)]},
    "G3": {"rectify_wide": F, "levels": [(F, F, F), (F, F, F), (F, F, F)]},
    "G4": {"rectify_wide": F, "levels": [(T, T, T), (T, T, T), (T, T, T), (F, T, F)]},
    "G8": {"rectify_wide": F, "levels": [(F, F, F), (F, F, F)]},
}


# -- hand-made images ----------------------------------------------------------------------------
CONTENTS = ("noise", "periodic", "blocks", "flat")
HAND_SIZES = {"G1": (336, 244), "G3": (329, 251)}   # packed paths / scalar paths
HAND_LEVELS, HAND_FEATURES = 3, 600
# side of the 0 / 255 squares of `blocks` per size (chosen so that some level has more than 256 NMS
# survivors in one score bin and more survivors than its quota, test_frontend_cases_cpu.py)
BLOCK_SQUARE = {"G1": 6, "G3": 6}


def noise_pair(width: int, height: int) -> np.ndarray:
    """Independent uniform bytes, different for left and right: [2][H][W]."""
    return np.random.default_rng(101).integers(0, 256, (2, height, width), dtype=np.uint8)


def periodic_pair(width: int, height: int, t: int = 0) -> np.ndarray:
    """A 25 x 41 random tile, each pixel doubled to 2 x 2 (period 50 x 82), tiled over the image;
    the left image is the right one moved 8 columns to the right, frame t + 1 is frame t moved 3
    columns to the left."""
    tile = np.random.default_rng(102).integers(0, 256, (41, 25), dtype=np.uint8)
    tile = np.repeat(np.repeat(tile, 2, axis=0), 2, axis=1)
    y = np.arange(height)[:, None] % tile.shape[0]
    x = np.arange(width)[None, :]
    right = tile[y, (x + 3 * t) % tile.shape[1]]
    left = tile[y, (x + 3 * t - 8) % tile.shape[1]]
    return np.stack([left, right])


def blocks_pair(width: int, height: int, square: int = 6) -> np.ndarray:
    """Random squares of 0 and 255, the left image moved 3 columns to the right."""
    rng = np.random.default_rng(103)
    cells = rng.integers(0, 2, ((height + square - 1) // square, (width + 3 + square - 1) // square), dtype=np.uint8) * 255
    wide = np.repeat(np.repeat(cells, square, axis=0), square, axis=1)[:height]
    return np.stack([wide[:, :width], wide[:, 3:width + 3]])


def flat_pair(width: int, height: int) -> np.ndarray:
    return np.full((2, height, width), 90, np.uint8)


def content_frames(sid: str, content: str, n: int = N_FRAMES) -> np.ndarray:
    """[n][2][H][W]: `periodic` as its shifted frames, every other content repeated."""
    w, h = HAND_SIZES[sid]
    if content == "periodic":
        return np.stack([periodic_pair(w, h, t) for t in range(n)])
    one = {"noise": noise_pair, "flat": flat_pair}[content](w, h) if content != "blocks" else blocks_pair(w, h, BLOCK_SQUARE[sid])
    return np.stack([one] * n)


@functools.lru_cache(maxsize=None)
def hand_rect(sid: str):
    """The rectification of the synthetic source at that size (plain lens: the images reach the
    pyramid as they are, so that `periodic` stays periodic and `blocks` keeps its edges)."""
    w, h = HAND_SIZES[sid]
    cams = extract_cameras(rig_calibration(make_source(SEED, w, h, distorted=False)), 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


def hand_cfg(fast_threshold: int | None = None) -> HipSlamConfig:
    kw = {} if fast_threshold is None else {"fast_threshold": fast_threshold}
    return HipSlamConfig(n_features=HAND_FEATURES, n_levels=HAND_LEVELS, **kw)


def run_oracle(rect, cfg, frames: np.ndarray) -> list:
    trk = O.OracleTracker(cfg, dict(fx=rect.fx, fy=rect.fy, cx=rect.cx, cy=rect.cy, baseline=rect.baseline,
                                    map_l=rect.map_left, map_r=rect.map_right))
    return [trk.step(fr[0], fr[1]) for fr in frames]


@functools.lru_cache(maxsize=None)
def hand_scenario(sid: str, content: str, fast_threshold: int | None = None) -> dict:
    """Frames, rectification, configuration and oracle run of one hand-made 3-frame sequence."""
    rect, cfg = hand_rect(sid), hand_cfg(fast_threshold)
    frames = content_frames(sid, content)
    frames.setflags(write=False)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": run_oracle(rect, cfg, frames)}


@functools.lru_cache(maxsize=None)
def mixed_scenario(sid: str) -> dict:
    """Six frames for batches of 1: rendered, rendered, blocks, flat, noise, rendered — a threshold
    learnt on texture, then a score-bucket overflow, then nothing, then recovery."""
    w, h = HAND_SIZES[sid]
    rect, cfg = hand_rect(sid), hand_cfg()
    ren = make_source(SEED, w, h, distorted=False).render_stereo_sequence(3)
    frames = np.stack([ren[0], ren[1], blocks_pair(w, h, BLOCK_SQUARE[sid]), flat_pair(w, h), noise_pair(w, h), ren[2]])
    frames.setflags(write=False)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": run_oracle(rect, cfg, frames)}


# -- keypoints on the limits of the packed fields -------------------------------------------------
LIMIT_SIZES = ("G5", "G6", "G10")   # W = 2044 (quad 510), H = 2047, W = 2047: one level, 600 features


def dots_pair(width: int, height: int, margin: int = 19) -> np.ndarray:
    """Single 255 pixels on a flat 90 image, 16 apart along the long side and 8 along the short one,
    from (margin, margin) to exactly (W - margin - 1, H - margin - 1): every dot is one keypoint of
    score 165 (all 16 circle pixels darker), none of its neighbours is a corner, so the keypoints sit
    on the first and last legal column and row and all share one score.  Right = left moved 4
    columns to the left."""
    sx, sy = (16, 8) if width >= height else (8, 16)
    lx, ly = width - margin - 1, height - margin - 1   # the grid keeps 8 clear of the last column / row
    xs = [x for x in range(margin, lx, sx) if lx - x >= 8] + [lx]
    ys = [y for y in range(margin, ly, sy) if ly - y >= 8] + [ly]
    left = np.full((height, width + 4), 90, np.uint8)
    left[np.ix_(ys, xs)] = 255
    return np.stack([left[:, :width], left[:, 4:]])


@functools.lru_cache(maxsize=None)
def limit_scenario(gid: str) -> dict:
    """Three repeated frames of `dots` at one of LIMIT_SIZES (plain lens: the dots stay dots)."""
    w, h, levels, features, _ = GEOMETRIES[gid]
    cams = extract_cameras(rig_calibration(make_source(SEED, w, h, distorted=False)), 2)
    (li, ri), = stereo_pairs(cams)
    rect = stereo_rectify(cams[li], cams[ri])
    cfg = HipSlamConfig(n_features=features, n_levels=levels)
    frames = np.stack([dots_pair(w, h, cfg.edge_margin)] * N_FRAMES)
    frames.setflags(write=False)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": run_oracle(rect, cfg, frames)}


def level_survivors(image_result: dict, cfg) -> list[np.ndarray]:
    """Scores of the NMS survivors of every level of one oracle image (before the top-K cut)."""
    out = []
    for lev in image_result["levels"]:
        keys = O.nms_keys(O.fast_scores(lev), cfg.fast_threshold, cfg.edge_margin)
        out.append(O.decode_keys(keys)[2])
    return out


def quotas(cfg) -> list[int]:
    return level_quotas(cfg.n_features, cfg.n_levels)
