"""The top-K selection on each of its paths: candidates swept from global memory (generic), kept
in LDS after one read (resident), and the library's own choice (auto), at every block shape.

k_select runs one of four block shapes per level, chosen from the level's quota and size
(1024 / 512 / 256 / 64 threads), and inside a block either sweeps the level's candidates from
global memory for every pass or keeps them in LDS when they fit the shape's capacity
(`tslam_select_mode`).  Whatever ran, the output is the same bytes.  Same bar as
tests/test_gpu_parity.py and tests/test_gpu_geometry.py: pyramids, keypoints, descriptors, matches,
disparities, refined positions and correspondences bit-exact against the oracle.

Shapes the cases reach (thor-slam_amd/csrc/k_image.hip, launch_select): 640 x 400 with 2,000
features: 512 / 256 / 64 / 64 threads for levels 0..3; G4: 256 / 64 / 64 / 64; G3 and the hand sizes:
256 / 64 / 64; G6 (H = 2047) and a quota of 6,400 on one level: 1024.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import frontend_cases as FC
from helpers import make_source
from test_gpu_geometry import _check_front_end, _device_run
from test_gpu_parity import hip_run

pytestmark = pytest.mark.gpu

# test_gpu_parity.hip_run caches its result on its arguments, and the select path is no argument
# of it (it reaches the handle through the `select_path` fixture): every case here needs a run of
# its own on the device
_run = hip_run.__wrapped__

MODES = ("auto", "generic", "resident")
# resident capacities of the block shapes that the boundary cases below run in (k_image.hip:
# SelSmall holds G3's level 0, SelWave its coarsest level); a count above them would never be
# resident, and the capacity override would decide nothing
SMALL_RESIDENT, WAVE_RESIDENT = 1024, 256


@pytest.fixture
def select_path(monkeypatch):
    """select_path(mode, cap): every Handle created afterwards in this test selects on that path."""
    from thor_slam_amd import _lib

    def use(mode: str, cap: int = 0) -> None:
        init = _lib.Handle.__init__

        def patched(self, *args, **kwargs):
            init(self, *args, **kwargs)
            self.select_mode(mode, cap)

        monkeypatch.setattr(_lib.Handle, "__init__", patched)

    return use


# -- rendered sequences --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", [3, 1])
@pytest.mark.parametrize("gid", ["G4", "G3"])   # level rows on the 16-byte grid (but the last) / off it
def test_modes_bit_exact_per_geometry(select_path, gid, batch, mode):
    """batch = 3: every level at te = t + 1 (far more candidates than any resident capacity);
    batch = 1: frames 1 and 2 under the learnt threshold, where the candidates fit."""
    w, h, _, _, distorted = FC.GEOMETRIES[gid]
    select_path(mode)
    sc, per = _run(seed=FC.SEED, batch=batch, distorted=distorted, n=FC.N_FRAMES, cfg_items=FC.cfg_items(gid),
                      width=w, height=h)
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, f"{gid} batch {batch} select {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_modes_bit_exact_at_the_flagship_size(select_path, mode):
    """640 x 400, 2,000 features, batches of 1: level 0 in the 512-thread shape, level 1 in the
    256-thread one, levels 2 and 3 in one wave each."""
    select_path(mode)
    sc, per = _run(batch=1)
    _check_front_end(sc["oracle"], per, sc["cfg"], 640, 400, f"640x400 select {mode}")


@pytest.mark.parametrize("mode", MODES)
def test_modes_bit_exact_in_the_largest_shape(select_path, mode):
    """G6 (64 x 2047: more rows than any smaller shape has bins): the 1024-thread shape, all keys in
    one score bucket above the counting sort's capacity."""
    w, h, _, _, _ = FC.GEOMETRIES["G6"]
    select_path(mode)
    sc = FC.limit_scenario("G6")
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=1)
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, f"G6 dots select {mode}")


# -- hand-made images ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("content,fast_threshold", [("noise", 0), ("blocks", None), ("flat", None)])
@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_hand_made_content_under_each_mode(select_path, sid, content, fast_threshold, mode):
    """noise at t = 0: the cut falls inside a score bin and then inside a row, with far more
    candidates than any resident capacity; blocks: a score bucket above TS_SEL_BUCKET_MAX (the
    bitonic path); flat: no candidate at any level."""
    select_path(mode)
    sc = FC.hand_scenario(sid, content, fast_threshold)
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=FC.N_FRAMES)
    _check_front_end(sc["oracle"], per, sc["cfg"], *FC.HAND_SIZES[sid], f"{sid} {content} t={fast_threshold} select {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_mixed_sequence_under_each_mode(select_path, sid, mode):
    """Batches of 1 over rendered, rendered, blocks, flat, noise, rendered: learnt threshold,
    bucket overflow, nothing (the fallback finds nothing either), recovery."""
    select_path(mode)
    sc = FC.mixed_scenario(sid)
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=1)
    _check_front_end(sc["oracle"], per, sc["cfg"], *FC.HAND_SIZES[sid], f"{sid} mixed select {mode}", features_only=True)


@functools.lru_cache(maxsize=None)
def _large_quota_scenario() -> dict:
    """`noise` at t = 0 on one level with a quota of 6,400: more keys than the 6,144 words of
    s_keys below the row-fill region of the 1024-thread shape, so the collected keys reach into the
    region that held the x-radix histogram; the cut falls inside a score bin and inside a row.  One
    frame (te = t + 1): its ~6,600 candidates also fit that shape's resident capacity."""
    from thor_slam_amd.params import HipSlamConfig

    rect = FC.hand_rect("G1")
    cfg = HipSlamConfig(n_features=6400, n_levels=1, fast_threshold=0)
    frames = FC.content_frames("G1", "noise", 1)
    frames.setflags(write=False)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(rect, cfg, frames)}


@pytest.mark.parametrize("mode", MODES)
def test_quota_above_the_row_fill_offset(select_path, mode):
    sc = _large_quota_scenario()
    cfg = sc["cfg"]
    for side in ("left", "right"):
        n = len(FC.level_survivors(sc["oracle"][0]["cur"][side], cfg)[0])
        assert n > cfg.n_features > 6144, f"{side}: {n} survivors must exceed the quota, the quota 6144"
    select_path(mode)
    per = _device_run(sc["rect"], cfg, sc["frames"], batch=1)
    _check_front_end(sc["oracle"], per, cfg, *FC.HAND_SIZES["G1"], f"G1 noise K=6400 select {mode}", features_only=True)


# -- the capacity boundary -----------------------------------------------------------------------
BOUNDARY_GID = "G3"
# level -> (fast_threshold, resident capacity of the level's block shape).  Frame 0 of a fresh
# handle runs at te = t + 1, so its candidates are the oracle's NMS survivors; the threshold puts
# their number between the level's quota and that capacity (at t = 20 level 0 has ~3,900
# survivors, at t = 60 the coarsest level has fewer than its quota: one threshold cannot serve both)
BOUNDARY_LEVELS = {0: (60, SMALL_RESIDENT), 2: (20, WAVE_RESIDENT)}


@functools.lru_cache(maxsize=None)
def _boundary_scenario(level: int):
    w, h, _, _, distorted = FC.GEOMETRIES[BOUNDARY_GID]
    from helpers import scenario

    items = FC.cfg_items(BOUNDARY_GID) + (("fast_threshold", BOUNDARY_LEVELS[level][0]),)
    sc = scenario(seed=FC.SEED, n=FC.N_FRAMES, width=w, height=h, distorted=distorted, cfg_items=items)
    counts = [len(FC.level_survivors(sc["oracle"][0]["cur"][side], sc["cfg"])[level]) for side in ("left", "right")]
    return sc, items, counts


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("level", sorted(BOUNDARY_LEVELS))
def test_resident_capacity_boundary(select_path, level, side, delta):
    """The resident capacity one below, at and one above a level's candidate count on frame 0
    (that of the left, then of the right image): the level takes the global sweeps, then just
    fits, then fits with room.  Everything bit-exact each time."""
    w, h, levels, _, distorted = FC.GEOMETRIES[BOUNDARY_GID]
    assert level in (0, levels - 1)
    sc, items, counts = _boundary_scenario(level)
    count, quota = counts[side], FC.quotas(sc["cfg"])[level]
    print(f"level {level} side {side}: {count} candidates, quota {quota}, capacity {count + delta}")
    assert count > quota, "the cut must be real"
    assert count + 1 <= BOUNDARY_LEVELS[level][1], "the count must fit the shape's own capacity"
    select_path("resident", count + delta)
    sc2, per = _run(seed=FC.SEED, batch=FC.N_FRAMES, distorted=distorted, n=FC.N_FRAMES, cfg_items=items, width=w, height=h)
    _check_front_end(sc2["oracle"], per, sc["cfg"], w, h, f"{BOUNDARY_GID} level {level} capacity {count + delta}")


# -- a level shorter than its quota --------------------------------------------------------------
SHORT_HALF = 28   # half side of the textured square of the sparse frame


@functools.lru_cache(maxsize=None)
def _short_scenario(sid: str) -> dict:
    """Batches of 1: rendered, rendered, sparse, rendered.  `sparse` is the third rendered frame
    inside a central square on a flat image: its corners score like the frames before it, so the
    learnt threshold is high, but every level has fewer survivors than its quota even at t + 1."""
    w, h = FC.HAND_SIZES[sid]
    rect, cfg = FC.hand_rect(sid), FC.hand_cfg()
    ren = make_source(FC.SEED, w, h, distorted=False).render_stereo_sequence(3)
    sparse = FC.flat_pair(w, h).copy()
    y0, x0 = h // 2 - SHORT_HALF, w // 2 - SHORT_HALF
    sparse[:, y0:y0 + 2 * SHORT_HALF, x0:x0 + 2 * SHORT_HALF] = ren[2][:, y0:y0 + 2 * SHORT_HALF, x0:x0 + 2 * SHORT_HALF]
    frames = np.stack([ren[0], ren[1], sparse, ren[2]])
    frames.setflags(write=False)
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(rect, cfg, frames)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_level_shorter_than_its_quota(select_path, sid, mode):
    """The sparse frame comes short under the learnt threshold (det_fail), and short again in the
    fallback at t + 1: kcount below the quota, padding records after it, and the next threshold
    back at t + 1, which the keypoints of the following frame show."""
    sc = _short_scenario(sid)
    cfg, quotas = sc["cfg"], FC.quotas(sc["cfg"])
    sparse = sc["oracle"][2]["cur"]
    for side in ("left", "right"):
        counts = list(sparse[side]["counts"])
        assert all(0 < n < q for n, q in zip(counts, quotas)), f"{side}: every level must come short ({counts} of {quotas})"
    select_path(mode)
    per = _device_run(sc["rect"], cfg, sc["frames"], batch=1)
    for cam, side in enumerate(("left", "right")):
        np.testing.assert_array_equal(per[2]["kp"][cam]["counts"], np.array(sparse[side]["counts"]))
    _check_front_end(sc["oracle"], per, cfg, *FC.HAND_SIZES[sid], f"{sid} short level select {mode}", features_only=True)
