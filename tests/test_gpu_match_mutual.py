"""The matcher's train-side minima (the mutual check) on each of their paths.

k_match keeps, per train, the minimum of (distance << 16 | query index) over the queries that gate
it.  The waves of a block merge their minima in an LDS array indexed by the train's y-sorted
position inside the block's window and the block sends one global atomic per touched position
(merged); positions past the array's capacity, or every position (direct), go straight to the
global minimum.  tbest is indexed by that position (a lookup array from k_select leads from the
best train's keypoint index to it), so a block's flush is one contiguous range.  qbest is not
cleared before a launch: blocks with nothing to match and the padding slots of a tile write the
"no match" word themselves.  `tslam_match_mode` forces either path or
caps the capacity; whatever ran, `stereo`, `temporal` and the refined values are the oracle's, bit
for bit (same bar as tests/test_gpu_parity.py).  `tslam_match_counters` shows that each case
reached the path it is about.

All cases at 320 x 240, 600 features, 3 levels (quotas 458 / 114 / 28: four query tiles at level
0, one tile of fewer than 32 queries at level 2); every level's window holds fewer trains than the
built-in capacity, so the capacity cap (64) is what sends a launch down both paths.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import frontend_cases as FC
from helpers import make_source, rig_calibration, rig_scene, scenario
from test_gpu_geometry import _check_front_end, _device_run

pytestmark = pytest.mark.gpu

W, H, LEVELS, FEATURES = 320, 240, 3, 600
CFG_ITEMS = (("n_features", FEATURES), ("n_levels", LEVELS))
CAP = 64
# (mode, merge capacity): the library's choice, every wave's own atomics, merged, merged with overflow
SETTINGS = [("auto", 0), ("direct", 0), ("merged", 0), ("merged", CAP)]
IDS = ["auto", "direct", "merged", f"merged-cap{CAP}"]
QTILES = sum((q + 127) // 128 for q in (458, 114, 28))


@pytest.fixture
def match_path(monkeypatch):
    """match_path(mode, cap): every Handle created afterwards in this test matches on that path and
    counts; the counters of each handle are appended to the returned list when it is closed."""
    from thor_slam_amd import _lib

    def use(mode: str, cap: int = 0) -> list:
        seen: list = []
        init, close = _lib.Handle.__init__, _lib.Handle.close

        def patched_init(self, *args, **kwargs):
            init(self, *args, **kwargs)
            self.match_mode(mode, cap)
            self.match_counters()   # switches counting on

        def patched_close(self):
            if getattr(self, "h", None):
                seen.append(self.match_counters())
            close(self)

        monkeypatch.setattr(_lib.Handle, "__init__", patched_init)
        monkeypatch.setattr(_lib.Handle, "close", patched_close)
        return seen

    return use


def _check_paths(cnt: dict, mode: str, cap: int, sides=("stereo", "temporal")) -> None:
    """The counters of a run that matched something on each of `sides`."""
    print(mode, cap, cnt)
    assert cnt["blocks_per_cu"] == 4, "k_match must keep 4 blocks on a compute unit"
    for side in sides:
        c = cnt[side]
        assert c["walked_blocks"] > 0
        if mode == "direct":
            assert c["direct"] > 0 and c["merged"] == 0 and c["flushed"] == 0, f"{side}: direct path only"
        elif cap:
            assert c["merged"] > 0 and c["direct"] > 0, f"{side}: a window above the cap takes both paths"
            assert 0 < c["flushed"] <= c["merged"]
        else:
            assert c["merged"] > 0 and c["direct"] == 0, f"{side}: every window fits the built-in capacity"
            assert 0 < c["flushed"] <= c["merged"]


@functools.lru_cache(maxsize=None)
def _rect():
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify

    cams = extract_cameras(rig_calibration(make_source(FC.SEED, W, H, distorted=False)), 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


def _cfg():
    from thor_slam_amd.params import HipSlamConfig

    return HipSlamConfig(**dict(CFG_ITEMS))


@functools.lru_cache(maxsize=None)
def _hand(kind: str) -> dict:
    """Hand-made sequences with their oracle run (computed once, frames read-only)."""
    ren = make_source(FC.SEED, W, H, distorted=False).render_stereo_sequence(3)
    if kind == "periodic":      # repeated descriptors: equal distances on both sides of a match
        frames = np.stack([FC.periodic_pair(W, H, t) for t in range(3)])
    elif kind == "blank_right":  # no train on the stereo side of any frame
        frames = ren.copy()
        frames[:, 1] = 90
    elif kind == "shrinking":   # batches of 1: the third frame has fewer keypoints at every level
        sparse = FC.flat_pair(W, H).copy()
        half = 28
        y0, x0 = H // 2 - half, W // 2 - half
        sparse[:, y0:y0 + 2 * half, x0:x0 + 2 * half] = ren[2][:, y0:y0 + 2 * half, x0:x0 + 2 * half]
        frames = np.stack([ren[0], ren[1], sparse, ren[2]])
    else:
        raise KeyError(kind)
    frames.setflags(write=False)
    rect, cfg = _rect(), _cfg()
    return {"rect": rect, "cfg": cfg, "frames": frames, "oracle": FC.run_oracle(rect, cfg, frames)}


def _rendered() -> dict:
    return scenario(seed=FC.SEED, n=3, width=W, height=H, distorted=False, cfg_items=CFG_ITEMS)


def _run_checked(sc: dict, batch: int, what: str, seen: list, features_only: bool = False) -> dict:
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=batch)
    _check_front_end(sc["oracle"], per, sc["cfg"], W, H, what, features_only=features_only)
    assert len(seen) == 1
    return seen[0]


# -- rendered frames: the block structure --------------------------------------------------------
@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_cross_block_and_cross_wave_minima(match_path, mode, cap):
    """Level 0 holds four query tiles whose temporal windows (80 px of 240 rows) share trains, so a
    train's minimum is combined across blocks in tbest; inside a temporal block the x-quartile
    boxes overlap, so it is first combined across waves.  Counters: more block flushes than trains
    exist (some train was flushed by two blocks), and more LDS merges than flushes (some position
    was merged by two waves)."""
    sc = _rendered()
    counts = [np.array(o["cur"]["left"]["counts"]) for o in sc["oracle"]]
    assert all(c[0] > 2 * 128 for c in counts), "level 0 needs two query tiles or more"
    assert FC.quotas(sc["cfg"])[2] < 32 and all(c[2] > 0 for c in counts), "level 2: fewer than 32 queries"
    cnt = _run_checked(sc, 3, f"rendered {mode} {cap}", match_path(mode, cap))
    _check_paths(cnt, mode, cap)
    t = cnt["temporal"]
    trains = int(sum(c.sum() for c in counts[:-1]))   # the t-1 keypoints of frames 1 and 2
    if mode == "direct":
        assert t["direct"] > trains, "a train must be reached by more than one wave"
    elif not cap:
        assert t["flushed"] > trains, "a train must be flushed by more than one block"
        assert t["merged"] > t["flushed"], "a position must be merged by more than one wave of a block"
    # the first frame: its temporal blocks return early and write "no match" themselves
    assert t["empty_blocks"] >= QTILES
    assert (np.array([o["cur"]["temporal"] for o in sc["oracle"][:1]]) == -1).all()


@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_first_frame_alone(match_path, mode, cap):
    """One frame through a fresh handle: every temporal block is a first-frame block."""
    sc = _rendered()
    one = {"rect": sc["rect"], "cfg": sc["cfg"], "frames": sc["frames"][:1], "oracle": sc["oracle"][:1]}
    cnt = _run_checked(one, 1, f"first frame {mode} {cap}", match_path(mode, cap))
    _check_paths(cnt, mode, cap, sides=("stereo",))
    assert cnt["temporal"]["empty_blocks"] == QTILES and cnt["temporal"]["walked_blocks"] == 0


# -- hand-made frames ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_tie_heavy_descriptors(match_path, mode, cap):
    """`periodic`: the image repeats every 50 x 82 px, so descriptors repeat inside a window and a
    query meets equal distances: the best train is the lowest keypoint index, the mutual check's
    best query the lowest query index."""
    sc = _hand("periodic")
    for o in sc["oracle"]:
        left = o["cur"]["left"]
        d = left["desc"][left["valid"]]
        assert len(np.unique(d, axis=0)) < 0.8 * len(d), "descriptors must repeat"
    assert any((o["cur"]["temporal"] >= 0).any() for o in sc["oracle"][1:])
    cnt = _run_checked(sc, 3, f"periodic {mode} {cap}", match_path(mode, cap))
    _check_paths(cnt, mode, cap)


@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_blank_right_image(match_path, mode, cap):
    """No keypoint in the right image: every stereo block has tn == 0 and writes "no match"."""
    sc = _hand("blank_right")
    for o in sc["oracle"]:
        assert sum(o["cur"]["right"]["counts"]) == 0 and (o["cur"]["stereo"] == -1).all()
    assert any((o["cur"]["temporal"] >= 0).any() for o in sc["oracle"][1:])
    cnt = _run_checked(sc, 3, f"blank right {mode} {cap}", match_path(mode, cap))
    _check_paths(cnt, mode, cap, sides=("temporal",))
    assert cnt["stereo"]["walked_blocks"] == 0 and cnt["stereo"]["empty_blocks"] == 3 * QTILES


@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_second_batch_has_fewer_keypoints(match_path, mode, cap):
    """Batches of 1: rendered, rendered, sparse, rendered.  The sparse frame fills no level, so the
    positions past its counts hold the frame before's qbest unless k_match rewrites them; the next
    frame then matches against the short one."""
    sc = _hand("shrinking")
    full, short = (np.array(sc["oracle"][i]["cur"]["left"]["counts"]) for i in (1, 2))
    assert (short < full).all() and short[0] <= 2 * 128, f"the sparse frame must come short everywhere ({short} of {full})"
    cnt = _run_checked(sc, 1, f"shrinking {mode} {cap}", match_path(mode, cap))
    _check_paths(cnt, mode, cap)
    # frame 0 and the level-0 tiles past the sparse frame's count return early
    assert cnt["temporal"]["empty_blocks"] > QTILES


# -- the stereo-only launch of a sharded rig -----------------------------------------------------
@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_stereo_only_launch(match_path, mode, cap):
    """Two ranks, a pair each, one batch of 4 frames: rank 1 solves frames 2 and 3 and first runs
    launch_match_stereo on frame 1, so it launches more stereo blocks than temporal ones.  Rank 1's
    stereo matches and disparities of frames 1..3 and its temporal matches and refined positions of
    frames 2 and 3 are the oracle's for both pairs; poses identical to the unsharded rig's."""
    import torch

    from test_gpu_shard import TWO, assert_identical, unsharded
    from thor_slam_amd.shard import LocalShardedRig

    sc = rig_scene(TWO, 4, width=W, height=H)
    cfg = _cfg()
    seen = match_path(mode, cap)
    want, _ = unsharded(sc, cfg, 4, 1)
    rig = LocalShardedRig(sc["rects"], cfg, world=2, batch=4, base_T_rect=sc["E"])
    rig.step(torch.from_numpy(np.ascontiguousarray(sc["frames"])).cuda())
    for r in range(2):
        assert_identical(rig.read(r), want[0])
    assert (want[0]["rig"]["stats"][1:, 0] == 0).all()
    # against the oracle: rank 1's pre-pass frame (1: stereo only) and its range (2, 3), both pairs
    h1, K = rig.ranks[1].h, cfg.n_features
    for p, ora in enumerate(_rig_oracle()):
        for g in (1, 2, 3):
            slot, cur = h1.ring_slot(g), ora[g]["cur"]
            what = f"rank 1 pair {p} frame {g} {mode} {cap}"
            np.testing.assert_array_equal(h1.frame_block("stereo", slot, np.int32)[p * K:(p + 1) * K], cur["stereo"], err_msg=what)
            disp = h1.frame_block("disp", slot, np.float64)[p * K:(p + 1) * K]
            np.testing.assert_array_equal(np.isnan(disp), np.isnan(cur["disp"]), err_msg=what)
            ok = ~np.isnan(cur["disp"])
            np.testing.assert_array_equal(disp[ok], cur["disp"][ok], err_msg=what)
            if g > 1:
                np.testing.assert_array_equal(h1.frame_block("temporal", slot, np.int32)[p * K:(p + 1) * K], cur["temporal"], err_msg=what)
                corr = ora[g]["corr"]
                tuv = h1.frame_block("temporal_uv", g, np.float64).reshape(-1, K, 2)[p]
                np.testing.assert_array_equal(tuv[corr["j"], 0], corr["u"], err_msg=what)
                np.testing.assert_array_equal(tuv[corr["j"], 1], corr["v"], err_msg=what)
    rig.close()
    assert len(seen) == 3                      # the unsharded handle, then the ranks
    for cnt in seen:
        _check_paths(cnt, mode, cap)
    blocks = [{s: c[s]["walked_blocks"] + c[s]["empty_blocks"] for s in ("stereo", "temporal")} for c in seen]
    print(blocks)
    assert blocks[0]["stereo"] == blocks[0]["temporal"]
    assert blocks[2]["stereo"] > blocks[2]["temporal"] > 0, "rank 1 must have run a stereo-only launch"


@functools.lru_cache(maxsize=None)
def _rig_oracle() -> list:
    """The oracle's run of each pair of the two-pair rig scene (4 frames)."""
    sc = rig_scene(("192.168.2.21", "192.168.2.25"), 4, width=W, height=H)
    return [FC.run_oracle(rect, _cfg(), sc["frames"][:, 2 * p:2 * p + 2]) for p, rect in enumerate(sc["rects"])]


def test_imported_peer_image_has_selects_lookup_array():
    """tbest is indexed by the train's y-sorted position, found through the u16 lookup array
    (keypoint index -> position) that k_select writes beside the y-sorted records.  The stream
    block of the sharded exchange does not carry it: the unpack rebuilds it from the records.  Two
    ranks, a pair each: what rank 1 rebuilt for rank 0's cameras (and the reverse) is what the
    owner's select wrote, and it is the inverse of the records' index word."""
    import torch

    from test_gpu_shard import TWO
    from thor_slam_amd.shard import LocalShardedRig

    sc = rig_scene(TWO, 4, width=W, height=H)
    cfg = _cfg()
    K = cfg.n_features
    rig = LocalShardedRig(sc["rects"], cfg, world=2, batch=4, base_T_rect=sc["E"])
    rig.step(torch.from_numpy(np.ascontiguousarray(sc["frames"])).cuda())
    h = [rk.h for rk in rig.ranks]
    checked = 0
    # rank r solves frames [2r, 2r + 2) and imports the peer's cameras for frames 2r - 1 .. 2r + 1
    for r, frames in ((0, (0, 1)), (1, (1, 2, 3))):
        for g in frames:
            slot = h[r].ring_slot(g)
            for cam in range(4):
                owner = cam // 2
                got = h[r].frame_block("ypos", slot, np.uint16).reshape(4, K)[cam]
                want = h[owner].frame_block("ypos", h[owner].ring_slot(g), np.uint16).reshape(4, K)[cam]
                np.testing.assert_array_equal(got, want, err_msg=f"rank {r} frame {g} camera {cam}")
                z = h[r].frame_block("ysorted", slot, np.uint32).reshape(4, K, 4)[cam, :, 2]
                np.testing.assert_array_equal(got[z], np.arange(K), err_msg=f"rank {r} frame {g} camera {cam}: not the inverse")
                checked += owner != r
    assert checked == 2 * (2 + 3)
    assert not np.array_equal(got, np.arange(K)), "the lookup must be a real permutation"
    rig.close()


# -- RGB-D ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rgbd():
    from oracle import numpy_slam as O
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=W, height=H)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rect = rgbd_undistort(cams[ci])
    cfg = HipSlamConfig(rgbd=True, **dict(CFG_ITEMS))
    trk = O.OracleTracker(cfg, dict(fx=rect.fx, fy=rect.fy, cx=rect.cx, cy=rect.cy, baseline=rect.baseline,
                                    map_l=rect.map_left, map_r=rect.map_right))
    oracle = [trk.step_rgbd(*src.render_rgbd(i)) for i in range(3)]
    return {"src": src, "rect": rect, "cfg": cfg, "oracle": oracle, "records": src.render_rgbd_sequence(3)[:, None, :]}


@pytest.mark.parametrize("mode,cap", SETTINGS, ids=IDS)
def test_rgbd_handle(match_path, mode, cap):
    """Depth replaces stereo matching: every stereo block returns early, the temporal ones match."""
    from test_gpu_rgbd import _check, _hip

    sc = _rgbd()
    assert all(o["status"] == 0 for o in sc["oracle"][1:])
    seen = match_path(mode, cap)
    _check(sc, _hip(sc, 3))
    assert len(seen) == 1
    _check_paths(seen[0], mode, cap, sides=("temporal",))
    s = seen[0]["stereo"]
    assert s["walked_blocks"] == 0 and s["empty_blocks"] > 0 and s["merged"] == s["direct"] == 0
