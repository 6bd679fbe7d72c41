"""k_describe's keypoint list in LDS and its stores, eight keypoints at a time, on the device.

A tile lists (xy, position, index) of its keypoints from the y-sorted records of its rows, at most
512 positions at a time (`tslam_describe_mode` caps that, so that small images run several chunks);
a wave collects eight descriptors and stores them, the y-sorted copies and the keypoint words
together, and what is left after its last keypoint; the level's first tile writes the padding zeros
behind its keypoints.  The cases (tests/describe_chain_cases.py; their preconditions are asserted
here on the oracle before the device is touched, and in tests/test_describe_chain_cpu.py) are at
256x128 (both levels on 16-byte rows) and 250x130 (neither: the byte staging):

  * level-0 tiles of exactly 1, 8, 9, 64, 65, 72 and 130 keypoints: waves of 0, 1, 8, 9 and 17;
  * the same images with list capacities 1, 8, 64 and the default: identical outputs;
  * noise at 336x244 with more than 512 records in a tile's rows: chunks without the hook;
  * a blanked second tile row and a first tile without a keypoint: padding zeros all the same;
  * three batches through one handle whose ring wraps (max_batch = 4).

Every case compares pyramids, keypoints (orientation included), descriptors, the y-sorted
descriptors and the padding zeros with the NumPy oracle bit for bit; `desc` and `desc_ys` are filled
with 0xFF before every run.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import describe_chain_cases as DC
from test_gpu_block_decode import _check_sorted
from test_gpu_geometry import _check_front_end

pytestmark = pytest.mark.gpu

CAPS = (0, 1, 8, 64)   # 0: the built-in capacity


def _run(sc: dict, batches: tuple, list_cap: int = 0, max_batch: int | None = None):
    """The frames through a fresh handle in the given batches; per frame what the feature checks
    read, plus the ring slots of every batch."""
    import torch

    from thor_slam_amd._lib import Handle

    cfg, frames = sc["cfg"], sc["frames"]
    h = Handle([sc["rect"]], cfg, max_batch=max_batch or max(batches))
    try:
        h.describe_mode(list_cap)
        for which in ("desc", "desc_ys"):   # the zeros of the padding slots must be written, not inherited
            h.copy_in(which, 0, np.full(h.buffer_info(which)[1], 0xFF, np.uint8))
        K = cfg.n_features
        dev = torch.from_numpy(np.array(frames)).cuda()   # a writable copy of the cached input
        s = torch.cuda.current_stream().cuda_stream
        per, slots, b0 = [], [], 0
        for nb in batches:
            h.submit(dev[b0:].data_ptr(), nb, s)
            h.read_poses(nb)
            slots.append([h.ring_slot(b0 + f) for f in range(nb)])
            for f in range(nb):
                g, slot = b0 + f, slots[-1][f]
                per.append({
                    "pyr": h.frame_block("pyramid", slot, np.uint8).reshape(2, h.pyr_bytes),
                    "kp": [h.keypoints(g, 0), h.keypoints(g, 1)],
                    "ys": h.frame_block("ysorted", slot, np.uint32).reshape(2, K, 4),
                    "desc_ys": h.frame_block("desc_ys", slot, np.uint32).reshape(2, K, 8),
                })
            b0 += nb
        assert b0 == len(frames)
    finally:
        h.close()
    return per, slots


def _check(sc: dict, per: list, what: str) -> None:
    w, h = sc["size"]
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, what, features_only=True)
    for i, (rec, o) in enumerate(zip(per, sc["oracle"])):
        _check_sorted(rec, [o["cur"]["left"], o["cur"]["right"]], f"{what} frame {i}")


def _assert_flush_counts(sc: dict) -> None:
    """The condition of the flush cases, from the oracle's keypoints alone."""
    tiles = [n for o in sc["oracle"] for side in ("left", "right") for n in DC.tile_counts(o["cur"][side]).values()]
    for n in DC.WANTED_COUNTS:
        assert n in tiles, f"no level-0 tile of exactly {n} keypoints: {sorted(set(tiles))}"
    assert max(tiles) >= 129, f"no level-0 tile of 129 keypoints or more: {max(tiles)}"
    waves = {k for n in tiles for k in DC.per_wave(n)}
    assert set(DC.WANTED_PER_WAVE) <= waves and max(waves) >= 17, f"keypoints per wave {sorted(waves)}"


@functools.lru_cache(maxsize=None)
def _flush_run(size: str, cap: int):
    sc = DC.flush_scenario(size)
    _assert_flush_counts(sc)
    return _run(sc, (len(sc["frames"]),), list_cap=cap)[0]


@pytest.mark.parametrize("size", sorted(DC.SIZES))
def test_flush_boundaries(size):
    _check(DC.flush_scenario(size), _flush_run(size, 0), f"flush {size}")


@pytest.mark.parametrize("cap", CAPS[1:])
@pytest.mark.parametrize("size", sorted(DC.SIZES))
def test_chunked_lists_agree(size, cap):
    """A tile of 130 keypoints among 202 records in its rows takes 202, 26 and 4 chunks."""
    sc = DC.flush_scenario(size)
    rows = max(n for o in sc["oracle"] for side in ("left", "right")
               for n in DC.row_range_positions(o["cur"][side], sc["size"][1]))
    assert rows > 3 * max(CAPS), f"at most {rows} records in a tile's rows: fewer than four chunks at {max(CAPS)}"
    per, ref = _flush_run(size, cap), _flush_run(size, 0)
    _check(sc, per, f"flush {size} cap {cap}")
    for i, (a, b) in enumerate(zip(per, ref)):
        for cam in range(2):
            np.testing.assert_array_equal(a["kp"][cam]["desc"], b["kp"][cam]["desc"], err_msg=f"frame {i} camera {cam} desc")
            np.testing.assert_array_equal(a["kp"][cam]["angle"], b["kp"][cam]["angle"], err_msg=f"frame {i} camera {cam} angle")
        np.testing.assert_array_equal(a["desc_ys"], b["desc_ys"], err_msg=f"frame {i} desc_ys")


def test_more_records_than_the_list_holds():
    sc = DC.overflow_scenario()
    rows = [n for o in sc["oracle"] for side in ("left", "right")
            for n in DC.row_range_positions(o["cur"][side], sc["size"][1])]
    assert max(rows) > DC.LIST_CAP, f"at most {max(rows)} records in a tile's rows: one chunk"
    assert min(rows) <= DC.LIST_CAP, "no tile row of one chunk beside them"
    _check(sc, _run(sc, (len(sc["frames"]),))[0], "overflow")


@pytest.mark.parametrize("cap", [0, 8])
@pytest.mark.parametrize("size", sorted(DC.SIZES))
def test_empty_tile_rows_and_first_tile_without_keypoints(size, cap):
    sc = DC.blank_scenario(size)
    for i, o in enumerate(sc["oracle"]):
        for side in ("left", "right"):
            img = o["cur"][side]
            tiles = DC.tile_counts(img)
            assert tiles and set(tiles) == {(1, 0)}, f"frame {i} {side}: level-0 keypoints in tiles {sorted(tiles)}"
            assert (~np.asarray(img["valid"], dtype=bool)).any(), f"frame {i} {side}: no padding slot"
    _check(sc, _run(sc, (len(sc["frames"]),), list_cap=cap)[0], f"blank {size} cap {cap}")


def test_batches_through_a_wrapping_ring():
    """Frame k + 1 differs from frame k in every tile, so a descriptor kept from the block's
    previous use of a register or of the list would show."""
    sc = DC.flush_scenario("w256", 11)
    per, slots = _run(sc, (4, 4, 3), max_batch=4)
    assert any(s[k + 1] < s[k] for s in slots for k in range(len(s) - 1)), f"no batch wraps inside the ring: {slots}"
    _check(sc, per, "ring")
