"""The free-space layer without a device: the spec (thor_slam_amd/dense_freespace.py) against the
independent restatement (tests/ref_tsdf_freespace.py) on the scenes of tests/tsdf_freespace_cases.py,
the guard, the order of the frames, the resting object's figures, the configuration's checks and the
dense map's dispatch with the option on and off."""

from __future__ import annotations

import json

import numpy as np
import pytest

import ref_tsdf_freespace as RF
import test_dense_dispatch_cpu as D
import test_dense_dynamic_dispatch_cpu as DD
import tsdf_dynamic_cases as C
import tsdf_freespace_cases as F
from thor_slam_amd import dense_freespace as FS
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.slam._dense import DenseMap


# -- the spec equals the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("cam", [C.CAM, C.CAM2], ids=["67x77", "131x69"])
def test_spec_equals_reference(cam):
    frames, poses, obj, gap = F.call(cam)
    ref = F.call_reference(cam)
    t, w = C.volume()
    got = FS.dynamic(t, w, F.start_layer(2), C.ORIGIN, C.S, C.TRUNC, cam, frames, poses, 2, F.BAND_VOX, max_dist=C.MAX_D, **C.PRM)
    print(cam[:2], "nearest |sdf| to a gate", gap, "stats", ref["stats"].tolist())
    for k in ("mask", "depth", "stats", "words"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    # the call exercises every branch: words that grew, settled, saturated, were cleared, and stayed
    start = F.start_layer(2)
    r0, s0 = RF.unpack(start)
    r1, s1 = RF.unpack(ref["words"])
    assert (r1 > r0).any() and (s1 & ~s0).any() and (s0 & ~s1).any() and ((r0 == RF.SATURATED) & (r1 == RF.SATURATED)).any()
    assert ((r0 == RF.SATURATED) & (r1 == 0)).any() and (ref["words"] == start).any()
    assert not (ref["words"] >> 17).any()
    # the preset settled words take candidates away, and the layer is used as found: all frames alike
    plain = C.reference(frames[0], cam=cam)
    assert ref["stats"][0, 2] < plain["stats"][2] == obj.sum()
    np.testing.assert_array_equal(ref["mask"][0], ref["mask"][1])
    np.testing.assert_array_equal(ref["mask"][0], ref["mask"][3])
    assert ref["stats"][4].tolist() == [1, 0, 0, 0]


def test_a_nan_pose_and_an_empty_call_leave_the_layer():
    frames, poses, _, _ = F.call(C.CAM)
    start = F.start_layer(2)
    for mod in (FS, RF):
        got = mod.update(start, C.ORIGIN, C.S, C.CAM, frames[4:5], poses[4:5], C.MAX_D, F.BAND, 2)
        np.testing.assert_array_equal(got, start)
        np.testing.assert_array_equal(mod.update(start, C.ORIGIN, C.S, C.CAM, frames[:0], poses[:0], C.MAX_D, F.BAND, 2), start)


def test_table_lookup_matches():
    """A synthetic table that mirrors the image left to right: spec and restatement agree through it."""
    W, H = C.CAM[:2]
    frames, poses, _, _ = F.call(C.CAM)
    ys, xs = np.mgrid[0:H, 0:W]
    table = np.stack([(W - 1 - xs) * 32 + 5, ys * 32 - 7], axis=-1).astype(np.int32)
    ok, _ = RF.guarded(F.DIMS, C.ORIGIN, C.S, C.CAM, frames[0], poses[0], C.MAX_D, F.BAND, table)
    assert ok
    a = FS.update(F.start_layer(2), C.ORIGIN, C.S, C.CAM, frames[:2], poses[:2], C.MAX_D, F.BAND, 2, undistort=table)
    b = RF.update(F.start_layer(2), C.ORIGIN, C.S, C.CAM, frames[:2], poses[:2], C.MAX_D, F.BAND, 2, table=table)
    np.testing.assert_array_equal(a, b)
    assert not np.array_equal(a, RF.update(F.start_layer(2), C.ORIGIN, C.S, C.CAM, frames[:2], poses[:2], C.MAX_D, F.BAND, 2))


# -- the guard ---------------------------------------------------------------------------------------------
def test_guard_passes_the_scenes_and_catches_a_voxel_on_a_gate():
    frames, poses, _, gap = F.call(C.CAM)
    assert 0.0 < gap < F.BAND
    sdf = []
    RF.observations(F.DIMS, C.ORIGIN, C.S, C.CAM, frames[0], poses[0], C.MAX_D, F.BAND, sdf_out=sdf)
    sdf = np.array(sdf)
    for sign in (1.0, -1.0):   # a band that is exactly one voxel's |sdf|: the upper gate, then the lower one
        on = sdf[(sign * sdf > 0.5 * C.S) & (sign * sdf < C.TRUNC)]
        assert on.size
        ok, g = RF.guarded(F.DIMS, C.ORIGIN, C.S, C.CAM, frames[0], poses[0], C.MAX_D, float(abs(on[0])))
        assert not ok and g == 0.0


# -- frame order -------------------------------------------------------------------------------------------
def test_frame_order_matters():
    frames, poses, _, _ = F.call(C.CAM)
    zero = np.zeros(F.SHAPE, np.uint32)
    ball = F.ball_voxels()
    for mod in (FS, RF):
        # the whole call ends on the box frame, which sees the ball's voxels free; with the last
        # sphere frame moved to the end they end on a run of 1
        a = mod.update(zero, C.ORIGIN, C.S, C.CAM, frames, poses, C.MAX_D, F.BAND, 2)
        b = mod.update(zero, C.ORIGIN, C.S, C.CAM, frames[list(F.PERMUTED)], poses[list(F.PERMUTED)], C.MAX_D, F.BAND, 2)
        assert not np.array_equal(a, b) and not a[ball].any() and (b[ball] == 1).any()
        # its first four frames, the static frame first instead of third
        order = [2, 0, 1, 3]
        a = mod.update(zero, C.ORIGIN, C.S, C.CAM, frames[:4], poses[:4], C.MAX_D, F.BAND, 2)
        b = mod.update(zero, C.ORIGIN, C.S, C.CAM, frames[order], poses[order], C.MAX_D, F.BAND, 2)
        assert not np.array_equal(a, b)
        # in order: two occupied frames settle the ball, the static frame clears it, one more gives run 1
        # permuted: cleared first, then three occupied frames in a row: settled
        assert (a[ball] == 1).any() and (b[ball] == (RF.SETTLED_BIT | 3)).any()
        assert not (a[ball] & RF.SETTLED_BIT).any()


# -- the resting object: the figures re-derived -------------------------------------------------------------
def test_resting_object_is_released_and_taken_back():
    steps, frames, obj, gap = F.chain_reference()
    ball = F.ball_voxels()
    t0, w0 = C.volume()
    n_obj = int(obj.sum())
    masked = [int(st["mask"][obj].sum()) for st in steps]
    settled = [int((st["words"][ball] & RF.SETTLED_BIT != 0).sum()) for st in steps]
    changed = [int(((st["tsdf"] != t0) | (st["weight"] != w0))[ball].sum()) for st in steps]
    print("object pixels", n_obj, "masked per call", masked, "ball voxels", int(ball.sum()), "settled", settled,
          "changed", changed, "nearest |sdf| to a gate", gap)
    assert n_obj == 68 and ball.sum() == 59                           # the figures the documents quote, held here
    assert masked[:3] == [n_obj] * 3 and changed[:3] == [0] * 3        # calls 0..2: every object pixel masked, the ball untouched
    assert settled[:3] == [0, 0, 20]                                   # the third frame settles the ball's front, within the band
    assert masked[3] == 0 and changed[3] == 56                         # call 3: nothing of the object masked, 56 of 59 voxels written
    assert 2.5e-5 < gap < 2.6e-5                                       # the nearest |sdf| to a gate of the band
    # (candidates that remain in call 3 are the silhouette's rim, the spec's known limit: the opening removes them)
    print("candidates per call", [int(st["stats"][2]) for st in steps])
    assert steps[3]["stats"][2] < steps[2]["stats"][2] == n_obj and steps[3]["stats"][3] == 0
    # the same figures from the spec module
    t, w = C.volume()
    words = np.zeros(F.SHAPE, np.uint32)
    for c, name in enumerate(F.CHAIN[:4]):
        got = FS.dynamic(steps[c - 1]["tsdf"] if c else t, steps[c - 1]["weight"] if c else w, words, C.ORIGIN, C.S, C.TRUNC, C.CAM,
                         frames[name][None], C.T_STAR[None], F.CHAIN_SETTLE, F.BAND_VOX, max_dist=C.MAX_D, **C.PRM)
        words = got["words"]
        np.testing.assert_array_equal(got["mask"][0], steps[c]["mask"])
        np.testing.assert_array_equal(words, steps[c]["words"])
    # the static frames afterwards: the voxels the object occupied are seen free, the release is withdrawn
    was = (steps[4]["words"] & RF.SETTLED_BIT != 0) & ball
    assert was.any() and not (steps[-1]["words"][ball] & RF.SETTLED_BIT).any() and not steps[-1]["words"][was].any()


# -- configuration -------------------------------------------------------------------------------------------
def test_config_validation():
    base = dict(rgbd=True, dense_map=True, dense_color=False, dense_dynamic=True)
    assert HipSlamConfig().dense_dynamic_settle_frames == 0 and HipSlamConfig().dense_dynamic_band_vox == 1.5
    HipSlamConfig(**base).validate()
    HipSlamConfig(**base, dense_dynamic_settle_frames=1).validate()
    HipSlamConfig(**base, dense_dynamic_settle_frames=65535, dense_dynamic_band_vox=4.0).validate()   # the default truncation
    HipSlamConfig(**base, dense_dynamic_settle_frames=3, dense_follow=True).validate()
    with pytest.raises(ValueError, match="settle_frames needs dense_dynamic"):
        HipSlamConfig(rgbd=True, dense_map=True, dense_dynamic_settle_frames=3).validate()
    for bad in (dict(dense_dynamic_settle_frames=-1), dict(dense_dynamic_settle_frames=65536), dict(dense_dynamic_settle_frames=True),
                dict(dense_dynamic_settle_frames=2.0),
                dict(dense_dynamic_settle_frames=3, dense_dynamic_band_vox=0.0),
                dict(dense_dynamic_settle_frames=3, dense_dynamic_band_vox=-1.0),
                dict(dense_dynamic_settle_frames=3, dense_dynamic_band_vox=4.0000001),
                dict(dense_dynamic_settle_frames=3, dense_dynamic_band_vox=float("nan")),
                dict(dense_dynamic_settle_frames=3, dense_dynamic_band_vox=float("inf")),
                dict(dense_dynamic_settle_frames=3, dense_dynamic_band_vox=2.5, tsdf_integrator_truncation_distance_vox=2.0)):
        with pytest.raises(ValueError, match="settle_frames|band_vox"):
            HipSlamConfig(**{**base, **bad}).validate()
    # the band is not looked at while the option is off
    HipSlamConfig(**base, dense_dynamic_band_vox=99.0).validate()
    with pytest.raises(ValueError, match="bits above 16"):
        FS.check_words(np.array([1 << 17], np.uint32))
    FS.check_words(np.array([RF.SETTLED_BIT | RF.SATURATED], np.uint32))
    run, settled = FS.split(np.array([RF.SETTLED_BIT | 7, 65535], np.uint32))
    assert run.dtype == np.uint16 and run.tolist() == [7, 65535] and settled.tolist() == [True, False]


# -- the dense map's dispatch ----------------------------------------------------------------------------------
def _calls(kw, **extra):
    cfg = HipSlamConfig(**kw, dense_dynamic=True, batch_size=D.N, **extra)
    cfg.validate()
    h = DD._Recorder(4 + D.N)
    dm = DenseMap(cfg, h, [D.SimpleNamespace(width=D.W, height=D.H)], 2, ())
    dm.init_handle()
    n_init = len(h.calls)
    dm.integrate(D.RECORDS_PTR, D.N, D.STREAM, stamps=D.STAMPS)
    return h.calls[:n_init], h.calls[n_init:]


@pytest.mark.parametrize("kw", [D.RGBD, D.STEREO], ids=["records", "stereo"])
def test_dispatch_option_on_adds_one_init_call(kw):
    init_off, batch_off = _calls(kw)
    init_on, batch_on = _calls(kw, dense_dynamic_settle_frames=7, dense_dynamic_band_vox=2.0)
    assert "tsdf_freespace_init" not in [c[0] for c in init_off + batch_off]
    at = [c[0] for c in init_on].index("tsdf_freespace_init")
    assert init_on[at] == ["tsdf_freespace_init", [], {"settle_frames": 7, "occupied_band_vox": 2.0}]
    assert init_on[at - 1][0] == "tsdf_dynamic_init"
    assert init_on[:at] + init_on[at + 1:] == init_off          # one extra call, nothing else
    assert batch_on == batch_off                                # the per-batch calls do not change


def test_dispatch_option_off_is_the_golden_trace():
    golden = json.loads(D.GOLDEN.read_text())
    cases = D._cases()
    assert sorted(cases) == sorted(golden)
    for name, (cfg, dense, has_color, g0) in cases.items():
        assert cfg.dense_dynamic_settle_frames == 0
        got = json.loads(json.dumps(D._run(cfg, dense, has_color, g0)))
        assert got == golden[name], name
