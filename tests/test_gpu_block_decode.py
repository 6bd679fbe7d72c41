"""Block decode, describe's prologue and the refinement's row loads on the device.

k_describe and the refinement kernels find their image from a grid (8, blocks per image, groups of 8
images) and their frame's ring slot from the batch's first slot; describe finds its tile in a table
and has both tile copies in flight when it learns whether its rows hold a keypoint; a refinement row
is one 16-byte load at the row's own byte address.  The cases here are small (256x128: 16-byte rows
on both levels; 250x130: neither level's rows are) and go at what those changes could break:

  * image counts around the grid's padding: 1 frame (2 images, 6 padding slots), 5 frames (10), a
    two-pair rig with 3 frames (12 images, 2 pairs), an RGB-D handle (1 camera) with 3 frames;
  * the ring: max_batch = 4 fed batches that wrap inside a batch and that start at slot 0 (the
    previous frame in the last slot); the very first frame has no previous frame;
  * a tile row with no keypoint (the image blanked from row 58 on): the block returns with its
    copies in flight, and the level's padding descriptors are still zeros (the descriptor buffers
    are filled with ones before every run);
  * matched keypoints next to the margin on all four sides of both levels, whose rows start at each
    of the four byte alignments.

Every frame of every batch is compared with the NumPy oracle bit for bit: pyramids, keypoints,
descriptors, stereo index and disparity, temporal index and position, correspondences and the
stats' counts; the y-sorted descriptors are the descriptors in the order of the device's y-sorted
records (zeros past them).  Poses meet the oracle at 1e-9 relative Frobenius, the bar of every
parity test here (the oracle is NumPy: its sums run in another order), and are bit for bit the same
between the two batchings of one sequence.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import frontend_cases as FC
from helpers import rel_frobenius, rig_scene, scenario
from oracle import numpy_slam as O
from test_gpu_geometry import _check_front_end, _check_poses
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

CFG_ITEMS = (("n_features", 300), ("n_levels", 2))
SIZES = {"w256": (256, 128), "w250": (250, 130)}
RING_BATCHES = (3, 3, 2, 3, 4, 3, 1)   # max_batch 4, ring 9: first frames 0 3 6 8 11 15 18
BLANK_FROM = 58                        # rows 58.. flat: no FAST circle of a row >= 64 meets texture
BORDER_ITEMS = (("n_features", 1200), ("n_levels", 2))


def _run(rects, cfg, frames, batches, max_batch=None, rig_E=None):
    """The frames through a fresh handle in the given batches; per frame and pair the blocks the
    parity checks read, plus the y-sorted records and descriptors of the pair's cameras."""
    import torch

    from thor_slam_amd._lib import Handle

    h = Handle(list(rects), cfg, max_batch=max_batch or max(batches))
    try:
        if rig_E is not None:
            h.set_rig(rig_E)
        for which in ("desc", "desc_ys"):   # the zeros of the padding slots must be written, not inherited
            h.copy_in(which, 0, np.full(h.buffer_info(which)[1], 0xFF, np.uint8))
        K, P, C, cpp = cfg.n_features, h.n_pairs, h.n_cams, h.cams_per_pair
        dev = torch.from_numpy(np.array(frames)).cuda()   # a writable copy of the cached input
        s = torch.cuda.current_stream().cuda_stream
        per, slots, b0 = [], [], 0
        for nb in batches:
            h.submit(dev[b0:].data_ptr(), nb, s)
            res = h.read_poses(nb)
            rig = h.read_rig_poses(nb) if rig_E is not None else None
            slots.append([h.ring_slot(b0 + f) for f in range(nb)])
            for f in range(nb):
                g, slot = b0 + f, slots[-1][f]
                pyr = h.frame_block("pyramid", slot, np.uint8).reshape(C, h.pyr_bytes)
                ys = h.frame_block("ysorted", slot, np.uint32).reshape(C, K, 4)
                dys = h.frame_block("desc_ys", slot, np.uint32).reshape(C, K, 8)
                kp = [h.keypoints(g, c) for c in range(C)]
                blk = {k: h.frame_block(k, slot, t).reshape(P, -1)[:, :K] for k, t in
                       (("stereo", np.int32), ("disp", np.float64), ("temporal", np.int32))}
                tuv = h.frame_block("temporal_uv", f, np.float64).reshape(P, -1)[:, :2 * K].reshape(P, K, 2)
                corr = h.frame_block("corr", f, np.float64).reshape(P, -1)[:, :8 * K].reshape(P, K, 8)
                pairs = []
                for p in range(P):
                    cams = range(cpp * p, cpp * p + cpp)
                    pairs.append({
                        "pyr": pyr[list(cams)], "kp": [kp[c] for c in cams], "ys": ys[list(cams)], "desc_ys": dys[list(cams)],
                        "stereo": blk["stereo"][p], "disp": blk["disp"][p], "temporal": blk["temporal"][p],
                        "tuv": tuv[p], "corr": corr[p], "T_rel": res["T_rel"][f, p], "T_abs": res["T_abs"][f, p],
                        "stats": res["stats"][f, p],
                    })
                per.append({"pairs": pairs, "rig": None if rig is None else {k: rig[k][f] for k in rig}})
            b0 += nb
        assert b0 == len(frames)
        quotas = list(h.quotas)
    finally:
        h.close()
    return per, slots, quotas


def _check_sorted(rec: dict, images: list, what: str) -> None:
    """Padding descriptors are zeros; the y-sorted descriptors are the descriptors in the order of
    the y-sorted records, zeros past the level's keypoints."""
    for cam, img in enumerate(images):
        valid = np.asarray(img["valid"], dtype=bool)
        desc, ys, dys = rec["kp"][cam]["desc"], rec["ys"][cam], rec["desc_ys"][cam]
        assert not desc[~valid].any(), f"{what} camera {cam}: a padding descriptor is not zero"
        live = ys[:, 3] != 0
        assert live.sum() == valid.sum(), f"{what} camera {cam}: {live.sum()} y-sorted records, {valid.sum()} keypoints"
        np.testing.assert_array_equal(dys[live], desc[ys[live, 2]], err_msg=f"{what} camera {cam}: y-sorted descriptors")
        assert not dys[~live].any(), f"{what} camera {cam}: a y-sorted padding descriptor is not zero"


def _check_stereo(oracle: list, per: list, cfg, width: int, height: int, what: str, pair: int = 0) -> None:
    recs = [r["pairs"][pair] for r in per]
    _check_front_end(oracle, recs, cfg, width, height, what)
    _check_poses(oracle, recs, what)
    for i, (rec, o) in enumerate(zip(recs, oracle)):
        _check_sorted(rec, [o["cur"]["left"], o["cur"]["right"]], f"{what} frame {i}")


@functools.lru_cache(maxsize=None)
def _scene(size: str):
    w, h = SIZES[size]
    return scenario(seed=0, n=5, width=w, height=h, cfg_items=CFG_ITEMS)


@functools.lru_cache(maxsize=None)
def _scene_run(size: str, batch: int):
    sc = _scene(size)
    return _run([sc["rect"]], sc["cfg"], sc["frames"], (batch,) * (5 // batch))[0]


# -- image counts around the grid's padding ---------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_stereo_bit_exact(size, batch):
    """2 images (6 padding slots of the group of 8) and 10 images (two groups, 6 padding slots)."""
    sc = _scene(size)
    w, h = SIZES[size]
    assert all(o["status"] == 0 for o in sc["oracle"][1:]), "the sequence must track"
    _check_stereo(sc["oracle"], _scene_run(size, batch), sc["cfg"], w, h, f"{size} batch {batch}")


@pytest.mark.parametrize("size", sorted(SIZES))
def test_batchings_agree_bitwise(size):
    """One frame per batch and five: every output, poses and covariances included, bit for bit."""
    for i, (a, b) in enumerate(zip(_scene_run(size, 1), _scene_run(size, 5))):
        ra, rb = a["pairs"][0], b["pairs"][0]
        for k in ("stereo", "temporal", "stats"):
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=f"frame {i} {k}")
        for k in ("disp", "tuv", "T_rel", "T_abs"):
            np.testing.assert_array_equal(ra[k].view(np.uint64), rb[k].view(np.uint64), err_msg=f"frame {i} {k} bits")
        n = int(ra["stats"][1])
        np.testing.assert_array_equal(ra["corr"][:n].view(np.uint64), rb["corr"][:n].view(np.uint64), err_msg=f"frame {i} corr")


# -- the ring ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ring_scene():
    return scenario(seed=0, n=sum(RING_BATCHES), width=256, height=128, cfg_items=CFG_ITEMS)


def test_ring_wraps_inside_a_batch_and_at_slot_zero():
    sc = _ring_scene()
    per, slots, _ = _run([sc["rect"]], sc["cfg"], sc["frames"], RING_BATCHES, max_batch=4)
    ring = max(max(s) for s in slots) + 1
    print("ring", ring, "slots per batch", slots)
    assert any(s[k + 1] < s[k] for s in slots for k in range(len(s) - 1)), "no batch wraps inside the ring"
    assert any(s[0] == 0 for s in slots[1:]), "no later batch starts at slot 0 (previous frame in the last slot)"
    assert slots[0][0] == 0 and (per[0]["pairs"][0]["temporal"] == -1).all(), "the first frame has no previous frame"
    _check_stereo(sc["oracle"], per, sc["cfg"], 256, 128, "ring")
    assert sum(o["status"] == 0 for o in sc["oracle"]) >= len(per) - 2, "the sequence must track"


# -- a tile row with no keypoint --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blank_scene():
    sc = _scene("w256")
    frames = sc["frames"][:3].copy()
    frames[:, :, BLANK_FROM:, :] = 90
    frames.setflags(write=False)
    cfg = HipSlamConfig(**dict(BORDER_ITEMS))   # quotas the 39 textured rows cannot fill
    return {"rect": sc["rect"], "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(sc["rect"], cfg, frames)}


@pytest.mark.parametrize("batch", [3, 1])
def test_tile_row_without_keypoints(batch):
    """Level 0 has two tile rows (rows 0..63, 64..127): no keypoint in the second, fewer keypoints
    than the quota in the first, so padding descriptors exist on both levels."""
    sc = _blank_scene()
    for i, o in enumerate(sc["oracle"]):
        for side in ("left", "right"):
            img = o["cur"][side]
            valid = np.asarray(img["valid"], dtype=bool)
            lv0 = valid & (img["kp"]["level"] == 0)
            assert lv0.any() and not (img["kp"]["y"][lv0] >= 64).any(), f"frame {i} {side}: a keypoint in tile row 1"
            assert (~valid).any(), f"frame {i} {side}: no padding slot"
    per = _run([sc["rect"]], sc["cfg"], sc["frames"], (batch,) * (3 // batch))[0]
    _check_stereo(sc["oracle"], per, sc["cfg"], 256, 128, f"blank batch {batch}")


# -- rows at every byte alignment, keypoints next to the margin ---------------------------------------


@functools.lru_cache(maxsize=None)
def _border_scene(size: str):
    """Noise moved one pixel right and down per frame; the right image sees it 5 columns further left."""
    w, h = SIZES[size]
    noise = np.random.default_rng(7).integers(0, 256, (h + 8, w + 16), dtype=np.uint8)
    # a 3x3 box keeps the noise's corners through the 2x2 level and the 5x5 smoothing
    pad = np.pad(noise.astype(np.uint32), 1, mode="edge")
    box = sum(pad[dy:dy + h + 8, dx:dx + w + 16] for dy in range(3) for dx in range(3)) // 9
    src = box.astype(np.uint8)
    frames = np.stack([np.stack([src[4 - i:4 - i + h, 8 - i:8 - i + w], src[4 - i:4 - i + h, 13 - i:13 - i + w]])
                       for i in range(3)])
    frames.setflags(write=False)
    sc = _scene(size)
    cfg = HipSlamConfig(**dict(BORDER_ITEMS))
    return {"rect": sc["rect"], "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(sc["rect"], cfg, frames)}


def border_coverage(size: str) -> dict:
    """Per level of frames >= 1: the byte alignments of the three kinds of rows the refinement loads
    (window at t, patch at t - 1, right window), x and y of the temporally matched keypoints and x
    of the stereo matches (whose right keypoint lies 5 columns further left, inside the margin too)."""
    sc = _border_scene(size)
    w, h = SIZES[size]
    off = FC.pyramid_offsets(w, h, 2)
    out = {}
    for i in (1, 2):
        cur, prev = sc["oracle"][i]["cur"], sc["oracle"][i - 1]["cur"]
        kp, pk, rk = cur["left"]["kp"], prev["left"]["kp"], cur["right"]["kp"]
        st, tm = np.asarray(cur["stereo"]), np.asarray(cur["temporal"])
        for l in range(2):
            wl = w >> l
            e = out.setdefault(l, {"window": set(), "patch": set(), "right": set(), "x": [], "y": [], "xs": []})
            for q in np.flatnonzero((kp["level"] == l) & np.asarray(cur["left"]["valid"], dtype=bool)):
                x, y = int(kp["x"][q]), int(kp["y"][q])
                if tm[q] >= 0:
                    e["x"].append(x), e["y"].append(y)
                    e["window"].add((off[l] + (y - 7) * wl + x - 7) % 4)
                    j = tm[q]
                    e["patch"].add((off[l] + (int(pk["y"][j]) - 5) * wl + int(pk["x"][j]) - 5) % 4)
                if st[q] >= 0:
                    e["xs"].append(x)
                    e["right"].add((off[l] + (y - 5) * wl + int(rk["x"][st[q]]) - 7) % 4)
    return out


@pytest.mark.parametrize("size", sorted(SIZES))
def test_rows_at_every_alignment_next_to_the_margin(size):
    sc = _border_scene(size)
    w, h = SIZES[size]
    m = sc["cfg"].edge_margin
    for l, e in border_coverage(size).items():
        wl, hl = w >> l, h >> l
        print(size, "level", l, {k: sorted(e[k]) for k in ("window", "patch", "right")}, "x", min(e["x"]), max(e["x"]),
              "of", m, wl - m - 1, "y", min(e["y"]), max(e["y"]), "of", m, hl - m - 1, "stereo x", min(e["xs"]), max(e["xs"]))
        for kind in ("window", "patch", "right"):
            assert e[kind] == {0, 1, 2, 3}, f"{size} level {l}: {kind} rows miss a byte alignment {sorted(e[kind])}"
        # frame t - 1 is frame t moved one pixel up and left, the right image 5 columns left: the
        # first column and row that can match are m + 1, and m + 5 for a stereo match
        assert min(e["x"]) <= m + 2 and max(e["x"]) >= wl - m - 2, f"{size} level {l}: no temporal match at a side margin"
        assert min(e["y"]) <= m + 2 and max(e["y"]) >= hl - m - 2, f"{size} level {l}: no temporal match at the top or bottom margin"
        assert min(e["xs"]) <= m + 9 and max(e["xs"]) >= wl - m - 5, f"{size} level {l}: no stereo match near a side margin"
    per = _run([sc["rect"]], sc["cfg"], sc["frames"], (3,))[0]
    recs = [r["pairs"][0] for r in per]
    _check_front_end(sc["oracle"], recs, sc["cfg"], w, h, f"border {size}")
    for i, (rec, o) in enumerate(zip(recs, sc["oracle"])):
        _check_sorted(rec, [o["cur"]["left"], o["cur"]["right"]], f"border {size} frame {i}")
        assert rec["stats"][0] == o["status"], f"border {size} frame {i}: status"


# -- a two-pair rig: 12 images, 2 pairs ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rig_scene():
    from oracle.numpy_rig import RigChain, rig_pose

    sc = rig_scene(n=3, width=256, height=128)
    cfg = HipSlamConfig(**dict(CFG_ITEMS))
    trks = [O.OracleTracker(cfg, dict(fx=r.fx, fy=r.fy, cx=r.cx, cy=r.cy, baseline=r.baseline, map_l=r.map_left,
                                      map_r=r.map_right)) for r in sc["rects"]]
    outs = [[trk.step(sc["frames"][i, 2 * q], sc["frames"][i, 2 * q + 1]) for q, trk in enumerate(trks)] for i in range(3)]
    chain, want = RigChain(), [{"status": 2}]
    for i in (1, 2):
        items = [{"status": o["status"], "T": o["T"], "corr": o.get("corr"), "intr": (r.fx, r.fy, r.cx, r.cy)}
                 for o, r in zip(outs[i], sc["rects"])]
        res = rig_pose(items, sc["E"], cfg)
        res["T_abs"] = chain.step(res)
        want.append(res)
    return {"frames": sc["frames"], "rects": sc["rects"], "E": sc["E"], "cfg": cfg, "outs": outs, "want": want}


def test_two_pair_rig_bit_exact():
    sc = _rig_scene()
    per = _run(sc["rects"], sc["cfg"], sc["frames"], (3,), rig_E=sc["E"])[0]
    for p in range(2):
        _check_stereo([o[p] for o in sc["outs"]], per, sc["cfg"], 256, 128, f"rig pair {p}", pair=p)
    for i, (rec, w) in enumerate(zip(per, sc["want"])):
        g = rec["rig"]
        assert g["stats"][0] == w["status"], f"rig frame {i}: status"
        if i and w["status"] == 0:
            assert g["stats"][4] == w["best"] and int(g["stats"][2]) == w["n_inliers"], (i, g["stats"])
            assert rel_frobenius(g["T_rel"], w["T"]) < 1e-9 and rel_frobenius(g["T_abs"], w["T_abs"]) < 1e-9, i


# -- RGB-D: one camera per pair ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rgbd_scene():
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=256, height=128)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rect = rgbd_undistort(cams[ci])
    cfg = HipSlamConfig(rgbd=True, **dict(CFG_ITEMS))
    trk = O.OracleTracker(cfg, dict(fx=rect.fx, fy=rect.fy, cx=rect.cx, cy=rect.cy, baseline=rect.baseline,
                                    map_l=rect.map_left, map_r=rect.map_right))
    oracle = [trk.step_rgbd(*src.render_rgbd(i)) for i in range(3)]
    return {"rect": rect, "cfg": cfg, "oracle": oracle, "records": src.render_rgbd_sequence(3)[:, None, :]}


@pytest.mark.parametrize("batch", [3, 1])
def test_rgbd_bit_exact(batch):
    sc = _rgbd_scene()
    per = _run([sc["rect"]], sc["cfg"], sc["records"], (batch,) * (3 // batch))[0]
    for i, (r, o) in enumerate(zip(per, sc["oracle"])):
        rec, left = r["pairs"][0], o["cur"]["left"]
        valid = left["valid"]
        np.testing.assert_array_equal(rec["kp"][0]["counts"], left["counts"], err_msg=f"frame {i} counts")
        for k in ("x", "y", "score", "angle", "level"):
            np.testing.assert_array_equal(rec["kp"][0][k][valid], left["kp"][k][valid], err_msg=f"frame {i} {k}")
        np.testing.assert_array_equal(rec["kp"][0]["desc"][valid], left["desc"][valid], err_msg=f"frame {i} descriptors")
        _check_sorted(rec, [left], f"rgbd frame {i}")
        np.testing.assert_array_equal(rec["disp"], o["cur"]["disp"], err_msg=f"frame {i} disparity")
        np.testing.assert_array_equal(rec["stereo"], o["cur"]["stereo"], err_msg=f"frame {i} stereo")
        np.testing.assert_array_equal(rec["temporal"], o["cur"]["temporal"], err_msg=f"frame {i} temporal")
        assert rec["stats"][0] == o["status"], f"frame {i}: status"
        if i and o["status"] == 0:
            assert rec["stats"][2] == o["n_inliers"] and rel_frobenius(rec["T_abs"], o["world_T_cam"]) < 1e-9, i
