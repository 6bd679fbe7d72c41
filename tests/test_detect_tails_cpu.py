"""The hand-made inputs of tests/detect_tail_cases.py do what they were chosen for (oracle and the
CPU restatement of detect's item dealing, tools/detect_tail_sim.py; no GPU)."""

from __future__ import annotations

import numpy as np
import pytest

import detect_tail_cases as DT
import frontend_cases as FC
from detect_tail_cases import SIM
from oracle import numpy_slam as O


def _level0_queues(gid: str, img: np.ndarray) -> list[dict]:
    w, h, levels, _ = DT.GEOMETRIES[gid]
    cfg = DT.cfg_for(gid)
    return SIM.level_queues(img, cfg.fast_threshold + 1, SIM.band_rows(w, h, levels)[0], cfg.edge_margin)


def test_band_rows_match_the_documented_geometry():
    """640 x 400, 4 levels: 32 / 68 / 100 / 50 rows, 18 band blocks per image (detect)."""
    br = SIM.band_rows(640, 400, 4)
    assert br == [32, 68, 100, 50]
    assert sum((h + b - 1) // b for (_, h), b in zip(O.level_shapes(640, 400, 4), br)) == 18
    assert [SIM.packed_levels(*DT.GEOMETRIES[g][:3]) for g in ("T336", "T332")] == [[True] * 3, [True, False, False]]
    for gid in ("T336", "T332"):
        w, h, levels, _ = DT.GEOMETRIES[gid]
        assert SIM.packed_levels(w, h, levels) == [lv[1] for lv in FC.level_paths(w, h, levels)["levels"]]


def test_both_sides_quads():
    """110 quads that are candidates on both sides, 220 survivors with scores 127 / 128, and the
    both-side quads lie in the tails of several waves."""
    gid = "T128"
    cfg = DT.cfg_for(gid)
    img = DT.both_image()
    te, m = cfg.fast_threshold + 1, cfg.edge_margin
    qb, qd = SIM.phase_a_quads(img, te)
    assert (qb & qd).sum() == 110 and (qb ^ qd).sum() == 0
    _, _, s = O.decode_keys(O.nms_keys(O.fast_scores(img), cfg.fast_threshold, m))
    assert sorted(np.unique(s, return_counts=True)[1]) == [110, 110] and set(s) == {127, 128}
    # restated dealing: the wave of every both-side quad inside its band block
    w, h, levels, _ = DT.GEOMETRIES[gid]
    br = SIM.band_rows(w, h, levels)[0]
    qa, nq = (m - 1) >> 2, ((w - m) >> 2) + 1 - ((m - 1) >> 2)
    blocks = _level0_queues(gid, img)
    tail_waves = set()
    for band, blk in enumerate(blocks):
        assert (blk["bright"] < 64).all() and (blk["dark"] < 64).all(), "every entry must stay in a tail"
        np.testing.assert_array_equal(blk["bright"], blk["dark"])
        y0 = band * br
        ra = max(0, m - y0)
        for y, q in zip(*np.nonzero(qb & qd)):
            r = y - y0 + 1
            if ra <= r < min(br + 2, h - m + 2 - y0):
                tail_waves.add((band, (((r - ra) * nq + (q - qa)) % 512) // 64))
    assert len({wv for _, wv in tail_waves}) >= 2 and len(tail_waves) >= 4


@pytest.mark.parametrize("stage", ["dark", "nms"])
def test_counts_around_the_round_size(stage):
    """Every planned wave of every planned band queues its planned number of entries of the stage:
    per-wave totals of 1 .. 128, tails of 0, 1, 63 next to full rounds, block tail totals of 0, 1,
    63, 64, 65 and 128; no other wave of those bands queues anything."""
    blocks = _level0_queues("T336", DT.plan_image(stage))
    for band, waves in DT.PLAN.items():
        want = np.zeros(8, np.int64)
        for wv, n in waves.items():
            want[wv] = n
        np.testing.assert_array_equal(blocks[band][stage], want, err_msg=f"band {band}")
        assert blocks[band]["bright"].sum() == 0
    per_wave = sorted({n for waves in DT.PLAN.values() for n in waves.values()})
    assert per_wave == [2, 32, 33, 63, 64, 65, 128]
    tails = sorted({sum(n % 64 for n in waves.values()) for waves in DT.PLAN.values()})
    assert tails == [0, 1, 63, 64, 65, 128]
    assert any(n % 64 == 0 for waves in DT.PLAN.values() for n in waves.values()), "a queue emptied exactly inside the loop"
    lev = SIM.level_rounds(DT.plan_image(stage), 21, 32, 19)[stage]
    assert lev["inloop"] == 4 and lev["lanes"] == 63 + 63 + 2 + 63 + 1 + 64 + 65 and lev["pooled"] == 2 + 1 + 0 + 1 + 0 + 1 + 2


def test_flat_image_queues_nothing():
    for gid in ("T64", "T336"):
        w, h, levels, _ = DT.GEOMETRIES[gid]
        cfg = DT.cfg_for(gid)
        got = SIM.image_rounds(DT.image(gid, "flat"), [cfg.fast_threshold + 1] * levels, levels, cfg.edge_margin)
        for lev in got:
            assert lev["blocks"] > 0
            assert all(v == 0 for s in SIM.STAGES for v in lev[s].values())


def test_one_row_of_dots_reaches_some_waves_only():
    blocks = _level0_queues("T336", DT.row_image())
    blk = blocks[1]   # y = 40
    assert (blk["dark"] > 0).sum() == 2 and (blk["dark"] == 0).sum() == 6
    assert 0 < blk["nms"].sum() and (blk["nms"] == 0).any()
    assert all(b["dark"].sum() == 0 for i, b in enumerate(blocks) if i != 1)


@pytest.mark.parametrize("gid", ["T64", "T128", "T336", "T332"])
def test_noise_at_the_first_threshold(gid):
    """te = t + 1 on noise: rounds inside the loops plus tails (64 x 64: fewer than 64 items per
    wave, so every round is a tail)."""
    w, h, levels, _ = DT.GEOMETRIES[gid]
    cfg = DT.cfg_for(gid)
    lev = SIM.image_rounds(DT.image(gid, "noise"), [cfg.fast_threshold + 1] * levels, levels, cfg.edge_margin)[0]
    for s in ("bright", "dark"):
        assert lev[s]["pooled"] > 0
        assert (lev[s]["inloop"] == 0) == (gid == "T64")
    assert lev["nms"]["partial"] > 0


@pytest.mark.parametrize("gid", ["T72", "T336", "T332"])
def test_edge_content_geometry(gid):
    """Texture in columns 0-7 and W-8 .. W-1 of every level; the last band of every packed level is short,
    and at T72 its second smoothing row group is empty."""
    w, h, levels, _ = DT.GEOMETRIES[gid]
    img = DT.edges_image(gid)
    br = SIM.band_rows(w, h, levels)
    for l, lev in enumerate(O.pyramid(img, levels)):
        lw = lev.shape[1]
        # uniform bytes have a standard deviation of 73.9; each level averages 2 x 2 and halves it
        lim = 60 / 2 ** l
        assert lev[:, :8].std() > lim and lev[:, lw - 8:].std() > lim, f"level {l} edge columns must hold texture"
        n = (8 << (levels - 1)) >> l
        assert (lev[:, n:lw - n] == DT.FLAT).all()
        last = lev.shape[0] - (lev.shape[0] - 1) // br[l] * br[l]
        if SIM.packed_levels(w, h, levels)[l]:
            assert last < br[l], f"level {l}: the last band must be short"
        sm = O.smooth(lev)
        assert (sm[:, :2] != lev[:, :2]).any() and (sm[:, lw - 2:] != lev[:, lw - 2:]).any()
    if gid == "T72":
        groups = max(2, br[0] // 16)
        sr = (br[0] + groups - 1) // groups
        last = h - (h - 1) // br[0] * br[0]
        assert sr * (groups - 1) >= last, "the last band's second row group must be empty"
