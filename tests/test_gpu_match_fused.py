"""k_match's two grid layouts: a block that matches both sides of its tile against one block per side.

By default a k_match block runs the query-side setup of its 128 queries once (load round, x-deal,
slot sort, A operand, column extent) and then matches the temporal and the stereo side one after
the other, reusing the ring, the reduction rows, the merge array and best / second.  The split
layout (`tslam_match_layout`, one block per side, each with its own setup) is the reference: the
words the matcher leaves (TSLAM_BUF_QBEST, _QSECOND, _QTPOS, _TBEST) are equal bit for bit, and the
block counters per side are equal too.  The merge counters of the stereo side may differ: a fused
block deals its queries to the waves by x for both sides, a stereo-only block by y.

Then the sides that differ inside one block, each against the oracle in the fused layout, with the
counters showing that the case reached what it is about.

All at 320 x 240, 600 features, 3 levels (quotas 458 / 114 / 28), as tests/test_gpu_match_mutual.py.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import frontend_cases as FC
from test_gpu_geometry import _check_front_end, _device_run
from test_gpu_match_mutual import (CFG_ITEMS, H, IDS, QTILES, SETTINGS, W, _check_paths, _hand, _rect, _rendered,
                                   _run_checked, match_path)  # noqa: F401 - match_path is a fixture

pytestmark = pytest.mark.gpu

WORDS = ("qbest", "qsecond", "qtpos", "tbest")
DTYPES = {"qbest": np.uint32, "qsecond": np.uint32, "qtpos": np.uint16, "tbest": np.uint32}


@pytest.fixture
def match_layout(monkeypatch):
    """match_layout(layout): every Handle created afterwards in this test uses that k_match grid
    (applied after match_path's settings when both fixtures are in use)."""
    from thor_slam_amd import _lib

    def use(layout: str) -> None:
        init = _lib.Handle.__init__

        def patched_init(self, *args, **kwargs):
            init(self, *args, **kwargs)
            self.match_layout(layout)

        monkeypatch.setattr(_lib.Handle, "__init__", patched_init)

    return use


def _match_words(sc: dict, layout: str, mode: str, cap: int) -> tuple[dict, dict]:
    """One batch of all frames through a fresh handle in `layout`: the matcher's words of every
    frame, [frame][side][K], and the counters."""
    import torch

    from thor_slam_amd._lib import Handle

    n, K = len(sc["frames"]), sc["cfg"].n_features
    h = Handle([sc["rect"]], sc["cfg"], max_batch=n)
    h.match_mode(mode, cap)
    h.match_layout(layout)
    h.match_counters()   # switches counting on
    dev = torch.from_numpy(np.array(sc["frames"])).cuda()
    h.submit(dev.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    h.read_poses(n)
    words = {k: np.stack([h.frame_block(k, f, DTYPES[k])[: 2 * K].reshape(2, K) for f in range(n)]) for k in WORDS}
    words["kcount"] = np.stack([h.frame_block("kcount", h.ring_slot(f), np.int32).reshape(2, -1)[0] for f in range(n)])
    cnt = h.match_counters()
    h.close()
    return words, cnt


def _written(kcount: np.ndarray, quotas: list[int], K: int) -> np.ndarray:
    """[frame][K]: the y-sorted positions below each level's count (qsecond is written nowhere else)."""
    mask = np.zeros((len(kcount), K), bool)
    off = 0
    for l, q in enumerate(quotas):
        for f in range(len(kcount)):
            mask[f, off:off + kcount[f, l]] = True
        off += q
    return mask


@pytest.mark.parametrize("kind", ["rendered", "periodic"])
@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_fused_equals_split(kind, mode, cap):
    sc = _rendered() if kind == "rendered" else _hand("periodic")
    K, quotas = sc["cfg"].n_features, FC.quotas(sc["cfg"])
    assert quotas[2] < 32, "level 2: one tile of fewer than 32 queries (waves 1..3 inactive on both sides)"
    split, cs = _match_words(sc, "split", mode, cap)
    fused, cf = _match_words(sc, "fused", mode, cap)
    print(kind, mode, cap, "split", cs, "fused", cf)
    np.testing.assert_array_equal(fused["kcount"], split["kcount"])
    assert (split["qbest"] != 0xFFFFFFFF).any(axis=(0, 2)).tolist() == [True, True], "both sides must match something"
    for k in ("qbest", "qtpos", "tbest"):
        np.testing.assert_array_equal(fused[k], split[k], err_msg=f"{kind} {mode} {cap}: {k}")
    w = _written(split["kcount"], quotas, K)[:, None, :].repeat(2, axis=1)
    np.testing.assert_array_equal(fused["qsecond"][w], split["qsecond"][w], err_msg=f"{kind} {mode} {cap}: qsecond")
    for c in (cs, cf):
        _check_paths(c, mode, cap)   # with the cap: direct > 0 on both sides, so the merge array was overrun twice per block
    for side in ("stereo", "temporal"):
        for k in ("empty_blocks", "walked_blocks"):
            assert cf[side][k] == cs[side][k], f"{side} {k}: fused {cf[side][k]} split {cs[side][k]}"
    n = len(sc["frames"])
    assert cf["temporal"]["empty_blocks"] + cf["temporal"]["walked_blocks"] == n * QTILES
    assert cf["stereo"]["empty_blocks"] + cf["stereo"]["walked_blocks"] == n * QTILES
    for k in ("merged", "direct", "flushed"):   # the temporal side is dealt by x in both layouts
        assert cf["temporal"][k] == cs["temporal"][k], f"temporal {k}"


# -- sides that differ inside one block (fused layout, against the oracle) -------------------------
def test_blank_right_stereo_has_no_train(match_path, match_layout):
    sc = _hand("blank_right")
    seen = match_path("auto", 0)
    match_layout("fused")
    cnt = _run_checked(sc, 3, "fused blank right", seen)
    _check_paths(cnt, "auto", 0, sides=("temporal",))
    assert cnt["stereo"]["walked_blocks"] == 0 and cnt["stereo"]["empty_blocks"] == 3 * QTILES
    assert cnt["temporal"]["walked_blocks"] > 0


def test_first_frame_temporal_empty_stereo_walks(match_path, match_layout):
    sc = _rendered()
    one = {"rect": sc["rect"], "cfg": sc["cfg"], "frames": sc["frames"][:1], "oracle": sc["oracle"][:1]}
    seen = match_path("auto", 0)
    match_layout("fused")
    cnt = _run_checked(one, 1, "fused first frame", seen)
    _check_paths(cnt, "auto", 0, sides=("stereo",))
    assert cnt["temporal"]["empty_blocks"] == QTILES and cnt["temporal"]["walked_blocks"] == 0
    assert cnt["stereo"]["walked_blocks"] == QTILES


def test_shrinking_tiles_past_the_count_return_for_both_sides(match_path, match_layout):
    sc = _hand("shrinking")
    short = np.array(sc["oracle"][2]["cur"]["left"]["counts"])
    assert short[0] <= 2 * 128
    seen = match_path("auto", 0)
    match_layout("fused")
    cnt = _run_checked(sc, 1, "fused shrinking", seen)
    _check_paths(cnt, "auto", 0)
    past = sum((q + 127) // 128 - (int(k) + 127) // 128 for q, k in zip(FC.quotas(sc["cfg"]), short))
    assert past >= 2
    # the sparse frame's tiles past its counts are empty on both sides (frame 0: temporal only)
    assert cnt["stereo"]["empty_blocks"] >= past
    assert cnt["temporal"]["empty_blocks"] >= QTILES + past


@functools.lru_cache(maxsize=None)
def _narrow() -> dict:
    """max_disparity 3 with 3 levels: 3 >> 2 == 0, so level 2 has no stereo range."""
    from thor_slam_amd.params import HipSlamConfig

    cfg = HipSlamConfig(max_disparity=3, **dict(CFG_ITEMS))
    frames = _rendered()["frames"]
    return {"rect": _rect(), "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(_rect(), cfg, frames)}


def test_empty_stereo_range_at_top_level(match_path, match_layout):
    sc = _narrow()
    quotas = FC.quotas(sc["cfg"])
    lo = quotas[0] + quotas[1]
    for o in sc["oracle"]:   # kp["level"] of the oracle: stereo has no match at level 2, temporal has
        lev = np.asarray(o["cur"]["left"]["kp"]["level"])
        assert (o["cur"]["stereo"][lev == 2] == -1).all()
    assert any((o["cur"]["temporal"][np.asarray(o["cur"]["left"]["kp"]["level"]) == 2] >= 0).any() for o in sc["oracle"][1:]), \
        "level 2 must have temporal matches"
    assert lo < sc["cfg"].n_features
    seen = match_path("auto", 0)
    match_layout("fused")
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=3)
    _check_front_end(sc["oracle"], per, sc["cfg"], W, H, "fused narrow disparity")
    cnt, = seen
    print(cnt)
    assert cnt["blocks_per_cu"] == 4
    # level 2's one tile per frame is empty on the stereo side and walks on the temporal side of frames 1, 2
    assert cnt["stereo"]["empty_blocks"] == 3 and cnt["stereo"]["walked_blocks"] == 3 * (QTILES - 1)
    assert cnt["temporal"]["empty_blocks"] == QTILES and cnt["temporal"]["walked_blocks"] == 2 * QTILES
