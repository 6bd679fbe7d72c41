"""k_detect's flush rounds and its smoothing edge columns on the device.

A wave of a detect block flushes its candidate queues 64 entries at a time inside its loops (phase
B of FAST per side, then the NMS); the phase-B tails of the block's 8 waves are pooled into rounds
of 64, an NMS tail is flushed by its wave.  The hand-made images of tests/detect_tail_cases.py put chosen numbers of entries into chosen
waves (tests/test_detect_tails_cpu.py checks that on the oracle).  Here they go through a handle in
batches of 3 (te = t + 1) and of 1 (a learnt te from the second frame on), with the t + 1 fallback
forced through the det_thr buffer where a case says so: pyramids, keypoints and descriptors are the
oracle's bit for bit (as tests/test_gpu_geometry.py compares them), the whole smoothed pyramid is
`oracle.smooth` of every level bit for bit (no other test reads it; its edge columns never reach a
descriptor), and `tslam_detect_counters` equals tools/detect_tail_sim.py's count for the same
images and thresholds, which also shows that the path a case is named for ran.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import detect_tail_cases as DT
import frontend_cases as FC
from detect_tail_cases import SIM
from oracle import numpy_slam as O
from test_gpu_geometry import _check_front_end

pytestmark = pytest.mark.gpu

KEYS = {"bright": ("inloop", "pooled", "lanes"), "dark": ("inloop", "pooled", "lanes"), "nms": ("inloop", "partial", "lanes")}


@functools.lru_cache(maxsize=None)
def _sim(gid: str, content: str, cam: int, te: tuple) -> list:
    """The simulation's rounds of one image of the case at thresholds te (frames repeat: cached)."""
    sc = DT.scenario(gid, content)
    side = ("left", "right")[cam]
    return SIM.pyramid_rounds(sc["oracle"][0]["cur"][side]["levels"], list(te), sc["cfg"].edge_margin)


def _run(gid: str, content: str, batch: int, force_fallback: bool):
    """The case's frames through a fresh counting handle: per frame the pyramid, the smoothed
    pyramid and the keypoints; the device counters; the simulation's counters for the thresholds
    and fallback flags the device used."""
    import torch

    from thor_slam_amd._lib import Handle

    sc = DT.scenario(gid, content)
    cfg, frames = sc["cfg"], sc["frames"]
    n, L, tfull = len(frames), cfg.n_levels, cfg.fast_threshold + 1
    h = Handle([sc["rect"]], cfg, max_batch=batch)
    try:
        first = h.detect_counters()   # switches counting on
        assert all(v == 0 for lev in first for s in SIM.STAGES for v in lev[s].values())
        dev = torch.from_numpy(np.array(frames)).cuda()
        s = torch.cuda.current_stream().cuda_stream
        per, want, fallbacks = [], None, 0
        for b0 in range(0, n, batch):
            nb = min(batch, n - b0)
            if force_fallback:   # no score reaches 255 + : every level comes short and runs again at t + 1
                h.copy_in("det_thr", 0, np.full(2 * L, 255, np.uint32))
            te = np.maximum(h.frame_block("det_thr", 0, np.uint32)[:2 * L].reshape(2, L), tfull)
            h.submit(dev[b0:].data_ptr(), nb, s)
            h.read_poses(nb)
            for f in range(nb):
                g = b0 + f
                slot = h.ring_slot(g)
                fail = h.frame_block("det_fail", f, np.uint32)[:2 * L].reshape(2, L)
                for cam in range(2):
                    want = SIM.add_rounds(want, _sim(gid, content, cam, tuple(int(t) for t in te[cam])))
                    flagged = [l for l in range(L) if fail[cam, l]]
                    fallbacks += len(flagged)
                    if flagged:
                        want = SIM.add_rounds(want, _sim(gid, content, cam, (tfull,) * L), levels=flagged)
                per.append({
                    "pyr": h.frame_block("pyramid", slot, np.uint8).reshape(2, h.pyr_bytes),
                    "smo": h.frame_block("smooth", f, np.uint8).reshape(2, h.pyr_bytes),
                    "kp": [h.keypoints(g, 0), h.keypoints(g, 1)],
                })
        got = h.detect_counters()
    finally:
        h.close()
    return sc, per, got, want, fallbacks


def _check_smoothed(sc: dict, per: list, gid: str, what: str) -> None:
    from test_gpu_parity import _levels
    from thor_slam_amd.params import level_shapes

    w, h, levels, _ = DT.GEOMETRIES[gid]
    wh, off = level_shapes(w, h, levels), FC.pyramid_offsets(w, h, levels)
    for i, (rec, o) in enumerate(zip(per, sc["oracle"])):
        for cam, side in enumerate(("left", "right")):
            for l, lev in enumerate(_levels(rec["smo"][cam], off, wh)):
                np.testing.assert_array_equal(lev, O.smooth(o["cur"][side]["levels"][l]),
                                              err_msg=f"{what} frame {i} {side} smoothed level {l}")


def _check_counters(got: list, want: list, what: str) -> dict:
    """Device counters == simulation, level by level; returns the totals per stage."""
    tot = {s: dict.fromkeys(KEYS[s], 0) for s in SIM.STAGES}
    tot["blocks0"] = got[0]["blocks"]
    for l, (g, w) in enumerate(zip(got, want)):
        print(what, "level", l, g)
        assert g["blocks"] == w["blocks"], f"{what} level {l}: blocks {g['blocks']} vs {w['blocks']}"
        for s in SIM.STAGES:
            for k in KEYS[s]:
                assert g[s][k] == w[s][k], f"{what} level {l} {s} {k}: device {g[s][k]}, simulation {w[s][k]}"
                tot[s][k] += g[s][k]
    return tot


def _check_paths(tot: dict, content: str, gid: str, what: str) -> None:
    """The path the case is named for ran."""
    b, d, n = tot["bright"], tot["dark"], tot["nms"]
    if content == "flat":
        assert all(v == 0 for s in SIM.STAGES for v in tot[s].values()), f"{what}: a flat image queues nothing"
        assert tot["blocks0"] > 0
    elif content == "both":
        assert b["pooled"] > 0 and d["pooled"] > 0 and b["lanes"] == d["lanes"] > 0 and n["partial"] > 0
    elif content == "plan_dark":
        assert d["inloop"] > 0 and d["pooled"] > 0 and n["partial"] > 0
    elif content == "plan_nms":
        assert n["inloop"] > 0 and n["partial"] > 0 and d["pooled"] > 0
    elif content == "row":
        assert d["pooled"] > 0 and n["partial"] > 0
    elif content == "noise":
        assert b["pooled"] > 0 and d["pooled"] > 0 and n["partial"] > 0
        assert (b["inloop"] > 0 and d["inloop"] > 0) == (gid != "T64"), f"{what}: rounds inside the loop"
    elif content == "edges":
        # named for the smoothing's edge columns (compared above); the texture lies outside the
        # margin at T72, so only the packed path itself is asserted: its blocks are counted
        assert tot["blocks0"] > 0
    else:
        raise KeyError(content)


@pytest.mark.parametrize("batch", [3, 1])
@pytest.mark.parametrize("gid,content", DT.CASES, ids=[f"{g}-{c}" for g, c in DT.CASES])
def test_pooled_rounds_bit_exact_and_counted(gid, content, batch):
    what = f"{gid} {content} batch {batch}"
    sc, per, got, want, _ = _run(gid, content, batch, force_fallback=False)
    w, h, _, _ = DT.GEOMETRIES[gid]
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, what, features_only=True)
    _check_smoothed(sc, per, gid, what)
    _check_paths(_check_counters(got, want, what), content, gid, what)


FALLBACK_CASES = [("T128", "both"), ("T336", "plan_dark"), ("T336", "noise"), ("T332", "edges"), ("T64", "flat")]


@pytest.mark.parametrize("batch", [3, 1])
@pytest.mark.parametrize("gid,content", FALLBACK_CASES, ids=[f"{g}-{c}" for g, c in FALLBACK_CASES])
def test_forced_fallback_bit_exact_and_counted(gid, content, batch):
    """det_thr = 255 before every batch: the speculative pass finds next to nothing, every level
    that has a quota comes short, and k_detect_fallback runs the same body at t + 1."""
    what = f"{gid} {content} batch {batch} fallback"
    sc, per, got, want, fallbacks = _run(gid, content, batch, force_fallback=True)
    w, h, levels, _ = DT.GEOMETRIES[gid]
    assert fallbacks == DT.N_FRAMES * 2 * levels, f"{what}: every image level must be flagged"
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, what, features_only=True)
    _check_smoothed(sc, per, gid, what)
    tot = _check_counters(got, want, what)
    _check_paths(tot, content, gid, what)
    per_image = sum(lev["blocks"] for lev in _sim(gid, content, 0, (sc["cfg"].fast_threshold + 1,) * levels))
    assert sum(g["blocks"] for g in got) == 2 * per_image * DT.N_FRAMES * 2, f"{what}: every band block ran twice"
