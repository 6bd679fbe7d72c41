"""The fused stereo + temporal sub-pixel refinement (k_refine_pair, ``match_refine="auto"``) against
the two kernels it replaces (``match_refine="split"``) and against the NumPy oracle.

Cases: (a) 640x400, 3 frames in one batch; (b) the same frames one per submit, so the previous
frame comes from an earlier submit and the ring (3 slots) wraps; (c) distorted lenses; (d) 320x240
with 500 features: K is no multiple of the 32 queries of a block, so the last block is partly live.
(d) runs 3 pyramid levels, as every 320x240 test here: the library refuses a 4th level of 40x30,
smaller than 2 * edge_margin + 3, which could hold no keypoint anyway.
Every case first shows, from the oracle's matches, that the queries of frames >= 1 cover all four
classes the fused kernel stages differently (both matches, stereo only, temporal only, neither).
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from helpers import scenario

pytestmark = pytest.mark.gpu

N = 3
CASES = {
    "a": dict(batch=3),
    "b": dict(batch=1),
    "c": dict(batch=3, distorted=True),
    "d": dict(batch=3, width=320, height=240, cfg_items=(("n_features", 500), ("n_levels", 3))),
}


def _scene(case: str):
    kw = {k: v for k, v in CASES[case].items() if k != "batch"}
    return scenario(seed=0, n=N, **kw)


@functools.lru_cache(maxsize=None)
def _run(case: str, match_refine: str):
    import torch

    from thor_slam_amd._lib import Handle

    sc = _scene(case)
    cfg, batch = sc["cfg"], CASES[case]["batch"]
    K = cfg.n_features
    h = Handle([sc["rect"]], cfg, max_batch=batch, match_refine=match_refine)
    dev = torch.from_numpy(np.ascontiguousarray(sc["frames"])).cuda()
    per = []
    for b0 in range(0, N, batch):
        nb = min(batch, N - b0)
        h.submit(dev[b0:].data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
        h.read_poses(nb)
        for f in range(nb):
            slot = h.ring_slot(b0 + f)
            per.append({
                "kp": [h.keypoints(b0 + f, 0), h.keypoints(b0 + f, 1)],
                "stereo": h.frame_block("stereo", slot, np.int32)[:K].copy(),
                "disp": h.frame_block("disp", slot, np.float64)[:K].copy(),
                "temporal": h.frame_block("temporal", slot, np.int32)[:K].copy(),
                "tuv": h.frame_block("temporal_uv", f, np.float64)[: 2 * K].reshape(K, 2).copy(),
            })
    h.close()
    return per


def _assert_classes(case: str):
    """All four query classes in every frame >= 1, no temporal match in frame 0 (oracle data)."""
    sc = _scene(case)
    for i, res in enumerate(sc["oracle"]):
        o = res["cur"]
        valid = np.asarray(o["left"]["valid"], dtype=bool)
        s, t = np.asarray(o["stereo"])[valid] >= 0, np.asarray(o["temporal"])[valid] >= 0
        if i == 0:
            assert not t.any(), "frame 0 has a temporal match"
            continue
        counts = [int((s & t).sum()), int((s & ~t).sum()), int((~s & t).sum()), int((~s & ~t).sum())]
        print(f"case {case} frame {i}: both / stereo only / temporal only / neither = {counts}")
        assert min(counts) > 0, f"case {case} frame {i}: a query class is missing {counts}"


def _assert_oracle(case: str, per: list):
    sc = _scene(case)
    for i, rec in enumerate(per):
        o = sc["oracle"][i]["cur"]
        np.testing.assert_array_equal(rec["stereo"], o["stereo"], err_msg=f"frame {i} stereo matches")
        np.testing.assert_array_equal(np.isnan(rec["disp"]), np.isnan(o["disp"]), err_msg=f"frame {i} disparity validity")
        ok = ~np.isnan(o["disp"])
        np.testing.assert_array_equal(rec["disp"][ok], o["disp"][ok], err_msg=f"frame {i} refined disparity")
        np.testing.assert_array_equal(rec["temporal"], o["temporal"], err_msg=f"frame {i} temporal matches")
        if i == 0:
            assert (rec["temporal"] == -1).all()
            continue
        corr = sc["oracle"][i]["corr"]
        np.testing.assert_array_equal(rec["tuv"][corr["j"], 0], corr["u"], err_msg=f"frame {i} refined u")
        np.testing.assert_array_equal(rec["tuv"][corr["j"], 1], corr["v"], err_msg=f"frame {i} refined v")


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_equals_split(case):
    _assert_classes(case)
    fused, split = _run(case, "auto"), _run(case, "split")
    assert len(fused) == len(split) == N
    for i, (a, b) in enumerate(zip(fused, split)):
        np.testing.assert_array_equal(a["stereo"], b["stereo"], err_msg=f"frame {i} stereo")
        np.testing.assert_array_equal(a["temporal"], b["temporal"], err_msg=f"frame {i} temporal")
        for k in ("disp", "tuv"):
            np.testing.assert_array_equal(np.isnan(a[k]), np.isnan(b[k]), err_msg=f"frame {i} {k} NaN mask")
            np.testing.assert_array_equal(a[k].view(np.uint64), b[k].view(np.uint64), err_msg=f"frame {i} {k} bits")
        assert (a["stereo"] >= 0).any() and (i == 0 or (a["temporal"] >= 0).any())


@pytest.mark.parametrize("case", ["a", "d"])
def test_fused_equals_oracle(case):
    _assert_classes(case)
    _assert_oracle(case, _run(case, "auto"))


def test_descriptors_320x240():
    """Describe's tile grid at 320x240 / K = 500: the last tile row of level 0 (rows 192..239)
    still meets the keypoint band and must be described."""
    sc = _scene("d")
    saw_last_row = False
    for i, rec in enumerate(_run("d", "auto")):
        for cam, side in ((0, "left"), (1, "right")):
            o, got = sc["oracle"][i]["cur"][side], rec["kp"][cam]
            valid = o["valid"]
            np.testing.assert_array_equal(got["counts"], np.array(o["counts"]), err_msg=f"frame {i} {side} counts")
            for k in ("x", "y", "level", "angle"):
                np.testing.assert_array_equal(got[k][valid], o["kp"][k][valid], err_msg=f"frame {i} {side} {k}")
            np.testing.assert_array_equal(got["desc"][valid], o["desc"][valid], err_msg=f"frame {i} {side} descriptors")
            lv0 = valid & (o["kp"]["level"] == 0)
            saw_last_row |= bool((o["kp"]["y"][lv0] >= 192).any())
    assert saw_last_row, "no level-0 keypoint in tile rows 192..239"
