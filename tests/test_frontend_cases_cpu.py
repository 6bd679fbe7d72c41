"""Preconditions of tests/test_gpu_geometry.py, checked on the oracle alone, so that the device
tests cannot pass vacuously: each geometry of ``frontend_cases`` really flips the kernel path it was
chosen for, the rendered sequences track, and the hand-made images really overflow a score bucket,
cut inside a score bin, repeat their descriptors or hold nothing."""

from __future__ import annotations

import numpy as np
import pytest

import frontend_cases as FC


@pytest.mark.parametrize("gid", sorted(FC.EXPECTED_PATHS))
def test_geometry_flips_the_listed_paths(gid):
    w, h, levels, _, _ = FC.GEOMETRIES[gid]
    got = FC.level_paths(w, h, levels)
    want = FC.EXPECTED_PATHS[gid]
    assert got["rectify_wide"] == want["rectify_wide"], f"{gid}: rectify path"
    assert got["levels"] == want["levels"], f"{gid}: per level (dma, dword, describe_wide)"


def test_geometry_offsets_and_limits():
    assert 336 % 64 != 0 and 448 % 64 == 0                                  # G1 / G4: rectify's first test
    assert FC.pyramid_offsets(332, 250, 3)[2] % 4 == 2                      # G2
    off = FC.pyramid_offsets(329, 251, 3)
    assert off[1] % 4 == 3 and FC.level_shapes(329, 251, 3)[1][0] % 4 == 0   # G3: the offset guard alone
    assert FC.level_shapes(448, 330, 4)[3] == (56, 41)                      # G4
    assert (2044 - 4) // 4 == 510 and 32 * 2044 == 65408                    # G5: last quad, rectify band bytes
    assert FC.level_shapes(83, 82, 2)[1] == (41, 41)                        # G8: 2 * edge_margin + 3
    assert FC.hand_cfg().edge_margin == 19


@pytest.mark.parametrize("gid", ["G1", "G2", "G3", "G4"])
def test_rendered_geometries_track(gid):
    sc = FC.geometry_scenario(gid)
    for i, o in enumerate(sc["oracle"][1:], start=1):
        assert o["status"] == 0 and o["n_corr"] >= 200, f"{gid} frame {i}: status {o['status']}, {o['n_corr']} correspondences"


def test_edge_geometries_reach_their_edges():
    """G4's level 3 finds fewer keypoints than its quota of 7, G5 pads most of its 600 slots, G6's keys
    hold rows past 1023, G7 cannot track, G8's coarsest level has a 3 x 3 keypoint band."""
    left = [FC.geometry_scenario(g)["oracle"][0]["cur"]["left"] for g in ("G4", "G5", "G6", "G8")]
    assert left[0]["quotas"][3] == 7 and 1 <= left[0]["counts"][3] < 7
    assert 0 < left[1]["counts"][0] < 100 and int(left[1]["kp"]["x"].max()) > 1023
    assert int(left[2]["kp"]["y"].max()) > 1023
    assert all(o["status"] == 1 for o in FC.geometry_scenario("G7")["oracle"][1:])
    v = left[3]["valid"] & (left[3]["kp"]["level"] == 1)
    assert ((left[3]["kp"]["x"][v] >= 19) & (left[3]["kp"]["x"][v] <= 21)).all()


@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_noise_cuts_inside_a_score_bin(sid):
    sc = FC.hand_scenario(sid, "noise")
    quota = FC.quotas(sc["cfg"])[0]
    scores = np.sort(FC.level_survivors(sc["oracle"][0]["cur"]["left"], sc["cfg"])[0])[::-1]
    print(f"{sid}: {scores.size} level-0 survivors against a quota of {quota}")
    assert scores.size >= 10 * quota
    kth = scores[quota - 1]
    assert (scores == kth).sum() >= 2 and (scores > kth).sum() < quota < (scores >= kth).sum()


@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_blocks_overflow_a_score_bucket(sid):
    sc = FC.hand_scenario(sid, "blocks")
    surv = FC.level_survivors(sc["oracle"][0]["cur"]["left"], sc["cfg"])
    hits = [l for l, (s, q) in enumerate(zip(surv, FC.quotas(sc["cfg"])))
            if s.size > q and np.bincount(s, minlength=256).max() > 256]
    print(f"{sid} (squares of {FC.BLOCK_SQUARE[sid]}): survivors {[s.size for s in surv]}, levels over the bucket {hits}")
    assert hits


@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_periodic_repeats_its_descriptors(sid):
    sc = FC.hand_scenario(sid, "periodic")
    for i, o in enumerate(sc["oracle"]):
        left = o["cur"]["left"]
        desc = left["desc"][left["valid"]]
        distinct = len({d.tobytes() for d in desc})
        matches = int((o["cur"]["stereo"] >= 0).sum())
        print(f"{sid} frame {i}: {distinct} distinct of {len(desc)} descriptors, {matches} stereo matches")
        assert len(desc) > 0 and distinct < 0.25 * len(desc)
        assert matches >= 100


@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_flat_has_no_keypoints(sid):
    for o in FC.hand_scenario(sid, "flat")["oracle"]:
        assert o["cur"]["left"]["counts"] == [0, 0, 0] and o["cur"]["right"]["counts"] == [0, 0, 0]


@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_mixed_sequence_goes_through_every_state(sid):
    """rendered, rendered, blocks, flat, noise, rendered: full quotas, then nothing, then full again."""
    ora = FC.mixed_scenario(sid)["oracle"]
    full = FC.quotas(FC.hand_cfg())
    assert [o["cur"]["left"]["counts"][0] for o in ora] == [full[0], full[0], full[0], 0, full[0], full[0]]
    # level 0 of the rendered frames teaches a threshold above fast_threshold + 1 (the K-th score - 2)
    left = ora[1]["cur"]["left"]
    kth = int(left["kp"]["score"][: full[0]][left["valid"][: full[0]]].min())
    print(f"{sid}: K-th level-0 score of the second rendered frame {kth}")
    assert kth - 2 > FC.hand_cfg().fast_threshold + 1


@pytest.mark.parametrize("gid", FC.LIMIT_SIZES)
def test_dots_sit_on_the_first_and_last_legal_column_and_row(gid):
    """Every dot is a keypoint, all share one score (a bucket of more than 256 keys, none cut), and
    the keys hold x = W - 20 and y = H - 20: 2024 / 2027 in the 11-bit fields at the widest and
    tallest images."""
    w, h, _, _, _ = FC.GEOMETRIES[gid]
    sc = FC.limit_scenario(gid)
    left = sc["oracle"][0]["cur"]["left"]
    n = left["counts"][0]
    x, y, score = (left["kp"][k][:n] for k in ("x", "y", "score"))
    print(f"{gid}: {n} keypoints, x {x.min()}..{x.max()}, y {y.min()}..{y.max()}, scores {set(score.tolist())}")
    assert n == int((sc["frames"][0, 0] == 255).sum()) and 256 < n <= sc["cfg"].n_features
    assert (x.min(), x.max(), y.min(), y.max()) == (19, w - 20, 19, h - 20)
    assert set(score.tolist()) == {165}
