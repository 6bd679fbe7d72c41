"""The rolling window's rule without a GPU: the decision, the layer move, the property that makes
the feature meaningful (a following window equals the crop of one large static volume, bit for
bit), and the config's checks.  ``tests/ref_tsdf_follow.py`` (the tests' restatement) and
``thor_slam_amd/dense_follow.py`` (the product's spec) are written apart and must agree."""

from __future__ import annotations

import numpy as np
import pytest

import ref_tsdf_follow as REF
from oracle.numpy_tsdf import integrate
from thor_slam_amd import dense_follow as DF
from thor_slam_amd.params import HipSlamConfig

S = 1.0 / 16.0
O0 = (-12 * S, -6 * S, -4 * S)          # on the voxel grid: every coordinate below is exact in f64
DIMS = (24, 12, 28)
ANCHOR = (12, 6, 4)


def _pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def _views(ts, use=None):
    use = [True] * len(ts) if use is None else use
    return [(REF.cam_T_world(_pose(t)), u) for t, u in zip(ts, use)]


def _table(views):
    """The device's pose table [n][13] of (cam_T_world, used) views."""
    return np.array([list(c[:3, :3].reshape(9)) + list(c[:3, 3]) + [1.0 if u else 0.0] for c, u in views])


def _both(views, shift, margin, step, anchor=ANCHOR):
    a = REF.decide(views, O0, S, shift, anchor, margin, step)
    b = DF.decide(_table(views), O0, S, shift, anchor, margin, step)
    assert tuple(a) == tuple(b)
    return a


# -- the decision ---------------------------------------------------------------------------------
def test_default_anchor_and_origin():
    assert DF.default_anchor(O0, S) == ANCHOR
    assert DF.default_anchor(HipSlamConfig().tsdf_origin, HipSlamConfig().voxel_size) == (100, 40, 20)
    assert REF.Window(O0, DIMS, S, 4 * S, 10.0, 100.0).anchor == ANCHOR
    for shift in ((0, 0, 0), (5, -3, 1000003)):
        np.testing.assert_array_equal(DF.effective_origin((-5.0, -2.0, -1.0), 0.05, shift),
                                      REF.origin_of((-5.0, -2.0, -1.0), 0.05, shift))
    assert REF.origin_of((-5.0, -2.0, -1.0), 0.05, (3, 0, 0))[0] == -5.0 + 0.05 * 3.0    # never accumulated


def test_no_move_inside_the_margin_and_hysteresis_after_one():
    margin, step = 3, 2
    for vox in range(-3, 4):                       # |e| <= margin: stays
        for a in range(3):
            t = [0.5 * S] * 3
            t[a] += vox * S
            assert _both(_views([t]), (0, 0, 0), margin, step) == (0, 0, 0)
    for margin, step in ((3, 2), (5, 5), (7, 1), (32, 16)):
        for vox in list(range(-70, 71, 3)) + [margin + 1, -margin - 1]:
            t = [(vox + 0.5) * S, 0.5 * S, 0.5 * S]
            d = _both(_views([t]), (0, 0, 0), margin, step)
            assert (d[0] != 0) == (abs(vox) > margin) and d[1] == d[2] == 0 and d[0] % step == 0
            if d[0]:
                e_after = vox - d[0]                # the camera's voxel against the anchor after the move
                assert abs(e_after) < step <= margin
                assert _both(_views([t]), d, margin, step) == (0, 0, 0)


def test_truncation_toward_zero():
    # e = -7, step 2: C division gives -3 -> delta -6 (floor division would give -8)
    t = [(-7 + 0.5) * S, 0.5 * S, (7 + 0.5) * S]
    assert _both(_views([t]), (0, 0, 0), 3, 2) == (-6, 0, 6)
    assert REF.trunc_div(-7, 2) == -3 and REF.trunc_div(7, 2) == 3 and REF.trunc_div(-8, 2) == -4


def test_first_used_view_decides_and_nothing_moves_without_one():
    far, near = [10.5 * S, 0.5 * S, 0.5 * S], [0.5 * S] * 3
    assert _both(_views([far, near]), (0, 0, 0), 3, 2) == (10, 0, 0)
    assert _both(_views([far, near], [False, True]), (0, 0, 0), 3, 2) == (0, 0, 0)
    assert _both(_views([far, far], [False, False]), (0, 0, 0), 3, 2) == (0, 0, 0)
    assert _both([], (0, 0, 0), 3, 2) == (0, 0, 0)
    # only the first chunk of 256 views is looked at
    many = _views([near] * 256 + [far], [False] * 256 + [True])
    assert _both(many, (0, 0, 0), 3, 2) == (0, 0, 0)
    assert _both(many[1:], (0, 0, 0), 3, 2) == (10, 0, 0)


def test_centre_that_is_not_finite_or_too_far_moves_nothing():
    for bad in (np.nan, np.inf, -np.inf):
        v = _views([[10.5 * S, 0.5 * S, 0.5 * S]])
        c = v[0][0].copy()
        c[1, 3] = bad                               # a used view whose translation is broken
        assert _both([(c, True)], (0, 0, 0), 3, 2) == (0, 0, 0)
    assert _both(_views([[2.0 ** 30 * S, 0.0, 0.0]]), (0, 0, 0), 3, 2) == (0, 0, 0)       # |c| reaches 2^30
    # the camera 13 voxels past the anchor of a window at shift 2^30 - 10: the new |shift| would reach 2^30
    assert _both(_views([[(2 ** 30 + 3.5) * S, 0.5 * S, 0.5 * S]]), (2 ** 30 - 10, 0, 0), 3, 2) == (0, 0, 0)
    assert _both(_views([[(2 ** 30 - 39.5) * S, 0.5 * S, 0.5 * S]]), (2 ** 30 - 60, 0, 0), 3, 2) == (20, 0, 0)


# -- the layer move ---------------------------------------------------------------------------------
def _brute(layer, delta):
    nz, ny, nx = layer.shape[:3]
    out = np.zeros_like(layer)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                kk, jj, ii = k + delta[2], j + delta[1], i + delta[0]
                if 0 <= kk < nz and 0 <= jj < ny and 0 <= ii < nx:
                    out[k, j, i] = layer[kk, jj, ii]
    return out


@pytest.mark.parametrize("delta", [(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 2), (-3, 2, -1), (6, 0, 0), (7, 0, 0), (0, -5, 0),
                                   (0, 0, -6), (-40, 20, 50)])
def test_layer_move_equals_the_triple_loop(delta):
    rng = np.random.default_rng(3)
    for shape in ((6, 5, 7), (6, 5, 7, 3)):       # [nz][ny][nx] and the colour layer
        layer = rng.normal(size=shape).astype(np.float32)
        want = _brute(layer, delta)
        np.testing.assert_array_equal(REF.move(layer, delta), want)
        np.testing.assert_array_equal(DF.move_layer(layer, delta), want)
        if any(abs(d) >= n for d, n in zip(delta, (7, 5, 6))):
            assert not want.any()


# -- a following window is the crop of one static volume ---------------------------------------------
def test_following_window_equals_crop_of_static_volume():
    """s = 1/16 and an origin on that grid: voxel centres of the window and of the static volume are
    the same doubles, so every voxel that has been inside the window since the first call holds,
    bit for bit, what the static volume holds.  Voxels that left and came back rightly differ."""
    W, H, PAD = 32, 24, 24
    intr = (20.0, 20.0, 15.5, 11.5)
    trunc, max_d, max_w = 4 * S, 10.0, 100.0
    steps = [(0, 0, 0), (0.3, 0, 0), (0.1, 0, 0), (0, 0, 0.4), (-0.9, 0, 0), (0, 0.3, 0), (0, 0, -0.5), (0.2, -0.35, 0.2)]
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    win = REF.Window(O0, DIMS, S, trunc, max_d, max_w, margin=3, step=2)
    big_dims = tuple(d + 2 * PAD for d in DIMS)
    big_o = tuple(o - PAD * S for o in O0)
    big_t, big_w = np.zeros(big_dims[::-1], np.float32), np.zeros(big_dims[::-1], np.float32)
    since_start = np.ones(DIMS[::-1], bool)         # in window coordinates of the CURRENT window
    pos = np.zeros(3)
    for call, st in enumerate(steps):
        pos = pos + np.array(st)
        views = []
        for f in range(2):                           # two frames per call, the second a little further
            depth = (900 + 150 * np.sin(0.3 * xx + call) + 100 * np.cos(0.4 * yy + f) + rng.integers(0, 30, (H, W))).astype(np.uint16)
            views.append({"cTw": REF.cam_T_world(_pose(pos + f * np.array([0.02, 0.01, 0.0]))), "used": True,
                          "depth": depth, "intr": intr})
        delta = win.call(views)
        assert delta == DF.decide(_table([(v["cTw"], True) for v in views]), O0, S,
                                  [a - b for a, b in zip(win.shift, delta)], ANCHOR, 3, 2)
        since_start = REF.move(since_start, delta)   # what the move brought in was not there before
        for v in views:
            integrate(big_t, big_w, v["depth"], v["cTw"], intr, big_o, S, trunc, max_d, max_w)
        lo = [PAD + k for k in win.shift]
        crop = tuple(slice(lo[a], lo[a] + DIMS[a]) for a in (2, 1, 0))
        assert win.origin == tuple(big_o[a] + S * lo[a] for a in range(3))
        np.testing.assert_array_equal(win.vol["weight"][since_start], big_w[crop][since_start])
        np.testing.assert_array_equal(win.vol["tsdf"][since_start], big_t[crop][since_start])
    moved = sum(any(d) for d in win.moves)
    observed = int((big_w[crop][since_start] > 0).sum())
    differ = int((win.vol["weight"][~since_start] != big_w[crop][~since_start]).sum())
    print("moves", win.moves, "final shift", win.shift, "compared observed", observed, "re-entered that differ", differ)
    assert win.shift == [-8, 0, -2]
    assert moved >= 4 and observed >= 1000
    axes = {(a, np.sign(d[a])) for d in win.moves for a in range(3) if d[a]}
    assert len(axes) == 6                            # all three axes, both directions
    assert differ > 0                                # the mask is not decoration


# -- config -----------------------------------------------------------------------------------------
def test_config_validation():
    ok = dict(rgbd=True, dense_map=True, dense_follow=True)
    HipSlamConfig(**ok).validate()
    HipSlamConfig(**ok, dense_follow_margin=2, dense_follow_step=2, dense_follow_anchor=(1, -2, 3)).validate()
    HipSlamConfig(dense_follow_margin=0).validate()          # off: its parameters are not looked at
    assert HipSlamConfig().dense_follow is False
    with pytest.raises(ValueError, match="dense_map"):
        HipSlamConfig(rgbd=True, dense_follow=True).validate()
    for kw in (dict(dense_follow_step=0), dict(dense_follow_step=33), dict(dense_follow_margin=0, dense_follow_step=1),
               dict(dense_follow_step=2.0)):
        with pytest.raises(ValueError, match="dense_follow_step"):
            HipSlamConfig(**ok, **kw).validate()
    for anchor in ((1, 2), (1, 2, 3.5), "abc", 7, (1, 2, 2 ** 30)):
        with pytest.raises(ValueError, match="dense_follow_anchor"):
            HipSlamConfig(**ok, dense_follow_anchor=anchor).validate()
    with pytest.raises(ValueError, match="sharded"):
        HipSlamConfig(**ok, devices=(0, 0), shard_transport="copy").validate()
