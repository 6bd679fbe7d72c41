"""The images of tests/describe_chain_cases.py do what they were chosen for (oracle only, no device)."""

from __future__ import annotations

import numpy as np
import pytest

import describe_chain_cases as DC


@pytest.mark.parametrize("size", sorted(DC.SIZES))
def test_tiles_hold_the_planned_keypoints(size):
    sc = DC.flush_scenario(size)
    for o, (left, right) in zip(sc["oracle"], DC.PLANS):
        assert DC.tile_counts(o["cur"]["left"]) == left and DC.tile_counts(o["cur"]["right"]) == right
    tiles = {n for plan in DC.PLANS for side in plan for n in side.values()}
    assert set(DC.WANTED_COUNTS) <= tiles and max(tiles) >= 129
    waves = {k for n in tiles for k in DC.per_wave(n)}
    assert set(DC.WANTED_PER_WAVE) <= waves and max(waves) >= 17
    assert sum(DC.per_wave(130)) == 130 and DC.per_wave(9) == [2, 1, 1, 1, 1, 1, 1, 1]


def test_keypoints_of_a_tile_differ():
    """A descriptor or an orientation stored for the wrong keypoint of a wave's eight must show."""
    img = DC.flush_scenario("w256")["oracle"][0]["cur"]["right"]
    kp, valid = img["kp"], np.asarray(img["valid"], dtype=bool)
    lv0 = valid & (kp["level"] == 0)
    assert len({d.tobytes() for d in img["desc"][lv0]}) == lv0.sum(), "two level-0 keypoints share a descriptor"
    assert len(set(kp["angle"][lv0].tolist())) >= 8, "fewer than 8 orientations among the level-0 keypoints"


def test_blank_rows_and_first_tile():
    sc = DC.blank_scenario("w256")
    img = sc["oracle"][0]["cur"]["left"]
    assert set(DC.tile_counts(img)) == {(1, 0)}
    assert DC.row_range_positions(img, sc["size"][1])[1] == 0


def test_noise_overflows_the_list():
    sc = DC.overflow_scenario()
    rows = DC.row_range_positions(sc["oracle"][0]["cur"]["left"], sc["size"][1])
    assert max(rows) > DC.LIST_CAP >= min(rows), rows
