"""The brick store's rule without a GPU (``thor_slam_amd/dense_store.py`` is the product's spec,
``tests/ref_tsdf_store.py`` the tests' restatement; written apart, they must agree): out and back
is the identity, a following window with the store equals one static volume wherever the window
was present whenever the static volume changed, floor division below zero, a pool that is too small,
and the config's checks."""

from __future__ import annotations

import math

import numpy as np
import pytest

import ref_tsdf_follow as REF
import ref_tsdf_store as RS
from oracle.numpy_tsdf import integrate
from thor_slam_amd import dense_store as DS
from thor_slam_amd.params import HipSlamConfig

S = 1.0 / 16.0
O0 = (-12 * S, -6 * S, -4 * S)          # on the voxel grid: every coordinate below is exact in f64
DIMS = (24, 12, 28)
W, H = 32, 24
INTR = (20.0, 20.0, 15.5, 11.5)
TRUNC, MAX_D, MAX_W = 4 * S, 10.0, 100.0
COLOR = ("tsdf", "weight", "color_weight", "color")


def _pose(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def _views(call, pos, rng, color=True):
    yy, xx = np.mgrid[0:H, 0:W]
    views = []
    for f in range(2):                               # two frames per call, the second a little further
        depth = (900 + 150 * np.sin(0.3 * xx + call) + 100 * np.cos(0.4 * yy + f) + rng.integers(0, 30, (H, W))).astype(np.uint16)
        v = {"cTw": REF.cam_T_world(_pose(np.asarray(pos) + f * np.array([0.02, 0.01, 0.0]))), "used": True,
             "depth": depth, "intr": INTR}
        if color:
            v["bgr"] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        views.append(v)
    return views


def _window(**kw):
    return RS.StoreWindow(O0, DIMS, S, TRUNC, MAX_D, MAX_W, **kw)


def _product_move(layers, shift, delta, store):
    """The product's model on copies of the test model's layers."""
    vol = {k: v.copy() for k, v in layers.items()}
    return vol, store.move(vol, shift, delta)


# -- 1. out and back is the identity ------------------------------------------------------------------
def test_out_and_back_is_the_identity():
    rng = np.random.default_rng(11)
    views = _views(0, (0, 0, 0), rng)
    win, plain = _window(layers=COLOR), _window(layers=COLOR, store=False)
    for w in (win, plain):
        w.call(views)                                # margin None: the window does not follow
    before = {k: v.copy() for k, v in win.vol.items()}
    assert (before["weight"] > 0).sum() > 1000 and (before["color_weight"] > 0).sum() > 100
    product, pvol, pshift = DS.Store(), {k: before[k].copy() for k in COLOR}, (0, 0, 0)
    for delta in ((5, -3, 9), (-5, 3, -9)):
        for w in (win, plain):
            w.shift_by(delta)
        pshift = product.move(pvol, pshift, delta)
        for k in COLOR:                              # the product's model and the tests' agree after every move
            np.testing.assert_array_equal(pvol[k].view(np.uint32), win.vol[k].view(np.uint32), err_msg=k)
        got, want = product.content(), win.content()
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        if delta[0] > 0:
            st = win.stats()
            print("away:", st)
            assert st["bricks"] > 4 and st["voxels_stored"] == win.left_nonzero > 500 and st["voxels_dropped"] == 0
    assert win.shift == [0, 0, 0] and pshift == (0, 0, 0)
    for k in COLOR:
        np.testing.assert_array_equal(win.vol[k].view(np.uint32), before[k].view(np.uint32), err_msg=k)
    bricks, words = win.content()
    assert len(bricks) == 0 and words.shape == (0, 6, 8, 8, 8)
    st = win.stats()
    assert st["bricks"] == 0 and st["voxels_stored"] == 0 and st["bricks_allocated"] > 4 and st["moves"] == 2
    # without the store the same sequence loses what left
    assert not np.array_equal(plain.vol["weight"], before["weight"])
    assert int((plain.vol["weight"] != before["weight"]).sum()) > 500


# -- 2. a following window with the store against one static volume --------------------------------------
def test_following_window_with_store_equals_static_volume():
    """s = 1/16 and an origin on that grid: voxel centres of the window and of the static volume are
    the same doubles.  Every observed voxel that was inside the window at every call in which the
    static volume changed it holds, bit for bit, what the static volume holds, in the window or in
    the store: also the voxels that left the window and came back, which is what the store is for."""
    PAD = 24
    steps = [(0, 0, 0), (0.3, 0, 0), (0.1, 0, 0), (0, 0, 0.4), (-0.9, 0, 0), (0, 0.3, 0), (0, 0, -0.5), (0.2, -0.35, 0.2)]
    away = {2: (8, 0, 0), 4: (0, 5, -9), 6: (-7, -4, 6)}      # explicit moves before these calls: the decision comes back
    rng = np.random.default_rng(5)
    win = _window(margin=3, step=2)
    big_dims = tuple(d + 2 * PAD for d in DIMS)
    big_o = tuple(o - PAD * S for o in O0)
    big_t, big_w = np.zeros(big_dims[::-1], np.float32), np.zeros(big_dims[::-1], np.float32)
    lo, hi = (-PAD,) * 3, tuple(d + PAD for d in DIMS)

    def inside():
        m = np.zeros(big_dims[::-1], bool)
        m[tuple(slice(PAD + win.shift[a], PAD + win.shift[a] + DIMS[a]) for a in (2, 1, 0))] = True
        return m

    valid = np.ones(big_dims[::-1], bool)           # never changed by the static volume while outside the window
    left_with_data = np.zeros(big_dims[::-1], bool)   # was outside the window while the static volume had data for it
    pos = np.zeros(3)
    for call, st in enumerate(steps):
        pos = pos + np.array(st)
        if call in away:
            win.shift_by(away[call])
            left_with_data |= ~inside() & (big_w > 0)
        views = _views(call, pos, rng, color=False)
        win.call(views)
        assert all(abs(k) <= PAD for k in win.shift)
        now = inside()
        left_with_data |= ~now & (big_w > 0)
        t0, w0 = big_t.copy(), big_w.copy()
        for v in views:
            integrate(big_t, big_w, v["depth"], v["cTw"], INTR, big_o, S, TRUNC, MAX_D, MAX_W)
        changed = (big_t.view(np.uint32) != t0.view(np.uint32)) | (big_w.view(np.uint32) != w0.view(np.uint32))
        valid &= ~(changed & ~now)
        whole = win.assemble(lo, hi)
        cmp = valid & (big_w > 0)
        np.testing.assert_array_equal(whole["weight"][cmp], big_w[cmp], err_msg=f"call {call}")
        np.testing.assert_array_equal(whole["tsdf"][cmp].view(np.uint32), big_t[cmp].view(np.uint32), err_msg=f"call {call}")
    returned = int((cmp & left_with_data & now).sum())
    print("moves", win.moves, "final shift", win.shift, "compared", int(cmp.sum()), "left and came back", returned,
          "store", win.stats())
    assert returned >= 200
    assert sum(any(d) for d in win.moves) >= 4 and int(cmp.sum()) >= 1000
    # the same sequence without the store fails the same comparison
    plain = _window(margin=3, step=2, store=False)
    rng = np.random.default_rng(5)
    pos = np.zeros(3)
    for call, st in enumerate(steps):
        pos = pos + np.array(st)
        if call in away:
            plain.shift_by(away[call])
        plain.call(_views(call, pos, rng, color=False))
    assert plain.shift == win.shift
    assert int((plain.assemble(lo, hi)["weight"][cmp] != big_w[cmp]).sum()) > 0


# -- 3. floor division ------------------------------------------------------------------------------------
def test_floor_division_below_zero():
    rng = np.random.default_rng(3)
    win = _window(layers=COLOR)
    win.shift = [-13, -5, -17]                       # absolute x -13..10, y -5..6, z -17..10
    shape = DIMS[::-1]
    for k in COLOR:
        win.vol[k] = rng.normal(size=shape + ((3,) if k == "color" else ())).astype(np.float32)
    win.vol["tsdf"][::3, ::2, ::5] = 0.0
    brute = {}                                       # absolute voxel -> words, one entry per voxel
    W0 = win.words()
    for k in range(shape[0]):
        for j in range(shape[1]):
            for i in range(shape[2]):
                brute[(i - 13, j - 5, k - 17)] = W0[:, k, j, i]
    product, pvol = DS.Store(), {k: win.vol[k].copy() for k in COLOR}
    product.move(pvol, win.shift, (DIMS[0], 0, 0))
    win.shift_by((DIMS[0], 0, 0))                    # |delta| >= dim: every voxel leaves
    assert not win.words().any() and not DS.words_of(pvol).any()
    bricks, words = win.content()
    want_keys = {tuple(math.floor(c / 8.0) for c in a) for a in brute}
    assert {tuple(b) for b in bricks.tolist()} == want_keys and len(want_keys) == 4 * 2 * 5
    assert {b[0] for b in want_keys} == {-2, -1, 0, 1} and min(b[2] for b in want_keys) == -3
    assert bricks.tolist() == sorted(bricks.tolist(), key=lambda b: (b[2], b[1], b[0]))
    seen = 0
    for b, brick in zip(bricks.tolist(), words):
        for z in range(8):
            for y in range(8):
                for x in range(8):
                    a = (8 * b[0] + x, 8 * b[1] + y, 8 * b[2] + z)
                    if a in brute:
                        assert (brick[:, z, y, x] == brute[a]).all(), a
                        seen += 1
                    else:
                        assert not brick[:, z, y, x].any(), a
    assert seen == len(brute)
    got = product.content()
    np.testing.assert_array_equal(got[0], bricks)
    np.testing.assert_array_equal(got[1], words)
    for a in (-17, -9, -8, -1, 0, 7, 8):
        b, loc = DS.brick_of(a)
        assert (int(b), int(loc)) == (math.floor(a / 8.0), a - 8 * math.floor(a / 8.0))
    # and back: the identity through negative bricks
    win.shift_by((-DIMS[0], 0, 0))
    np.testing.assert_array_equal(win.words(), W0)
    assert len(win.content()[0]) == 0


# -- 4. capacity ------------------------------------------------------------------------------------------
def test_capacity_below_what_a_move_needs():
    rng = np.random.default_rng(11)
    views = _views(0, (0, 0, 0), rng, color=False)
    small, full = _window(capacity=5), _window()
    product = DS.Store(capacity=5)
    for w in (small, full):
        w.call(views)
    before = small.words()
    pvol = {k: small.vol[k].copy() for k in ("tsdf", "weight")}
    for w in (small, full):
        w.shift_by((5, -3, 9))
    product.move(pvol, (0, 0, 0), (5, -3, 9))
    st = small.stats()
    print("capacity 5:", st, "unbounded:", full.stats())
    assert full.stats()["bricks"] > 5 and st["bricks_allocated"] == 5 and st["voxels_dropped"] > 0
    assert st["voxels_stored"] + st["voxels_dropped"] == small.left_nonzero == full.stats()["voxels_stored"]
    # which bricks win the five slots is unspecified (the two models fill them in different orders)
    assert len(product.bricks) == 5 and product.dropped > 0
    assert product.dropped + int(sum(v.any(axis=0).sum() for v in product.bricks.values())) == small.left_nonzero
    want = dict(zip(map(tuple, full.content()[0].tolist()), full.content()[1]))
    for b, brick in zip(*small.content()):           # every brick that is stored is exact
        np.testing.assert_array_equal(brick, want[tuple(b.tolist())])
    for w in (small, full):
        w.shift_by((-5, 3, -9))
    np.testing.assert_array_equal(full.words(), before)
    back = small.words()
    same = (back == before).all(axis=0)
    assert (same | ~back.any(axis=0)).all()          # a returning voxel has its old words or is zero
    assert int((~same).sum()) == st["voxels_dropped"]
    # a brick coordinate outside [-2^20, 2^20) is dropped, one inside is kept
    far = _window()
    far.call(views)
    n = int(far.words().any(axis=0).sum())
    far.shift = [8 * 2 ** 20, 0, 0]
    far.shift_by((DIMS[0], 0, 0))
    assert far.dropped == n and not far.bricks
    near = _window()
    near.call(views)
    near.shift = [-8 * 2 ** 20, 0, 0]
    near.shift_by((DIMS[0], 0, 0))
    assert near.dropped == 0 and near.stats()["voxels_stored"] == n


# -- the whole map from the window and the store ---------------------------------------------------------
def test_assemble_matches_the_brute_force():
    rng = np.random.default_rng(2)
    win = _window(layers=COLOR + ("freespace",))
    win.call(_views(0, (0, 0, 0), rng))
    win.vol["freespace"] = rng.integers(0, 1 << 17, DIMS[::-1]).astype(np.uint32) * (win.vol["weight"] > 0)
    for delta in ((5, -3, 9), (-30, 0, 2), (9, 1, 0)):
        win.shift_by(delta)
    bricks, words = win.content()
    layers = DS.split_words(words, color=True, freespace=True)
    run = lambda w: (w & 0xffff).astype(np.uint16)   # noqa: E731
    store = {**layers, "bricks": bricks, "run": run(layers["freespace"]), "settled": (layers["freespace"] >> 16) != 0}
    window = {k: win.vol[k] for k in COLOR}
    window.update(window_shift=np.array(win.shift), run=run(win.vol["freespace"]), settled=(win.vol["freespace"] >> 16) != 0)
    lo, hi = (-40, -9, -3), (37, 20, 45)
    got, want = DS.assemble(window, store, lo, hi), win.assemble(lo, hi)
    assert set(got) == set(COLOR) | {"run", "settled"}
    for k in COLOR:
        np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(got["run"], run(want["freespace"]))
    np.testing.assert_array_equal(got["settled"], (want["freespace"] >> 16) != 0)
    assert (got["weight"] > 0).sum() == (win.words()[1].view(np.float32) > 0).sum() + (words[:, 1].view(np.float32) > 0).sum()
    with pytest.raises(ValueError, match="lo < hi"):
        DS.assemble(window, store, (0, 0, 0), (0, 4, 4))
    with pytest.raises(ValueError, match="words per voxel"):
        DS.split_words(words, color=False, freespace=True)


# -- config -------------------------------------------------------------------------------------------------
def test_config_validation():
    ok = dict(rgbd=True, dense_map=True, dense_follow=True, dense_store=True)
    HipSlamConfig(**ok).validate()
    HipSlamConfig(**ok, dense_store_bricks=1).validate()
    HipSlamConfig(dense_store_bricks=0).validate()            # off: its parameter is not looked at
    cfg = HipSlamConfig()
    assert cfg.dense_store is False and cfg.dense_store_bricks == 65536
    with pytest.raises(ValueError, match="dense_follow"):
        HipSlamConfig(rgbd=True, dense_map=True, dense_store=True).validate()
    for bad in (0, -1, 2.0, True, 2 ** 30 + 1):
        with pytest.raises(ValueError, match="dense_store_bricks"):
            HipSlamConfig(**ok, dense_store_bricks=bad).validate()
    with pytest.raises(ValueError, match="sharded"):
        HipSlamConfig(**ok, devices=(0, 0), shard_transport="copy").validate()
