"""The mesh of the whole dense map on the CPU: the model in ``thor_slam_amd/dense_store.py``
(``whole_mesh``) against tests/ref_tsdf_store_mesh.py and against ``oracle.numpy_dense.extract_mesh`` on
window-plus-store states that ``dense_store.Store.move`` produces.  Dims 13 x 9 x 11: off the 8-voxel
brick grid on every axis and narrower than two bricks, so every window edge cuts bricks; the shifts
go below zero on every axis.  s = 0.0625 with the origin a multiple of s, where every f64 step of a
vertex is exact, so the box's mesh with its own origin has the same bits."""

from __future__ import annotations

import numpy as np

import ref_tsdf_store_mesh as RM
from oracle import numpy_dense as OD
from thor_slam_amd import dense_store as DS

NX, NY, NZ = 13, 9, 11
S, O0, MINW = 0.0625, (-0.625, -0.375, 1.0), 1e-4
CENTRE, RADIUS, TRUNC = np.array([-0.29, -0.11, 1.33]), 0.27, 4 * 0.0625
MOVES = [(5, -3, 2), (-16, 4, -4), (3, -9, 0), (-2, 3, -13), (NX + 30, 0, 0), (-NX - 20, 5, 15)]


def _observe(layers: dict, shift) -> None:
    """What a sensor would add: every window voxel still unobserved and within the band of the
    analytic sphere takes its distance, weight and a colour that depends on its absolute place."""
    k, j, i = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    a = np.stack([i + shift[0], j + shift[1], k + shift[2]], axis=-1)
    d = np.linalg.norm(np.array(O0) + S * (a + 0.5) - CENTRE, axis=-1) - RADIUS
    new = (layers["weight"] == 0) & (np.abs(d) < TRUNC)
    layers["tsdf"][new] = np.clip(d, -TRUNC, TRUNC).astype(np.float32)[new]
    layers["weight"][new] = 1.0 + (a.sum(axis=-1) % 3)[new]
    layers["color_weight"][new] = 1.0
    layers["color"][new] = ((a * np.array([3, 5, 7])) % 251).astype(np.float32)[new]


def _states():
    """(window dict, store dict, Store) after every move of MOVES, observing on the way."""
    layers = {"tsdf": np.zeros((NZ, NY, NX), np.float32), "weight": np.zeros((NZ, NY, NX), np.float32),
              "color_weight": np.zeros((NZ, NY, NX), np.float32), "color": np.zeros((NZ, NY, NX, 3), np.float32)}
    store, shift, out = DS.Store(), (0, 0, 0), []

    def snap():
        bricks, words = store.content() if store.bricks else (np.zeros((0, 3), np.int32), np.zeros((0, 6, 8, 8, 8), np.uint32))
        window = {**{k: v.copy() for k, v in layers.items()}, "window_shift": np.array(shift)}
        out.append((window, {**DS.split_words(words, True, False), "bricks": bricks}))

    _observe(layers, shift)
    snap()
    for delta in MOVES:
        shift = store.move(layers, shift, delta)
        layers = {k: np.array(v) for k, v in layers.items()}
        if delta != MOVES[4]:                       # parked far away: nothing to see there
            _observe(layers, shift)
        snap()
    return out


STATES = _states()


def _box(window, store):
    lo, hi = RM.bounds(window["window_shift"], (NX, NY, NZ), store["bricks"])
    return DS.assemble(window, store, lo, hi), lo


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_states_are_what_the_test_needs():
    shifts = np.array([w["window_shift"] for w, _ in STATES])
    assert (shifts.min(axis=0) < 0).all()
    assert all(len(s["bricks"]) > 0 for _, s in STATES[1:]) and (np.concatenate([s["bricks"] for _, s in STATES]) < 0).any()
    assert not STATES[5][0]["weight"].any()         # the window is empty: everything is in the store


def test_model_equals_ref_bit_for_bit():
    seam = split = 0
    for n, (window, store) in enumerate(STATES):
        box, lo = _box(window, store)
        want_t, want_c, info = RM.mesh(box, lo, O0, S, MINW, window["window_shift"], (NX, NY, NZ), store["bricks"])
        got_t, got_c, bricks = DS.whole_mesh(window, store, O0, S, MINW, colors=True)
        assert len(want_t) > 100, n
        np.testing.assert_array_equal(_u32(got_t), _u32(want_t), err_msg=f"state {n}")
        np.testing.assert_array_equal(_u32(got_c), _u32(want_c), err_msg=f"state {n}")
        assert bricks == info["bricks"], n
        plain_t, plain_c, _ = DS.whole_mesh(window, store, O0, S, MINW)
        assert plain_c is None
        np.testing.assert_array_equal(_u32(plain_t), _u32(want_t))
        seam, split = seam + info["seam_cubes"], split + info["split_cubes"]
    assert seam > 20 and split > 20                 # cubes across the window's edge, and across store bricks


def test_exact_grid_equals_the_box_mesh():
    for n, (window, store) in enumerate(STATES):
        box, lo = _box(window, store)
        origin = tuple(O0[c] + S * lo[c] for c in range(3))
        want_t, want_c = OD.extract_mesh(box["tsdf"], box["weight"], origin, S, MINW, color=box["color"])
        want = RM.sorted_rows(want_t, want_c)
        ref_t, ref_c, _ = RM.mesh(box, lo, O0, S, MINW)
        got_t, got_c, _ = DS.whole_mesh(window, store, O0, S, MINW, colors=True)
        np.testing.assert_array_equal(_u32(RM.sorted_rows(ref_t, ref_c)), _u32(want), err_msg=f"ref, state {n}")
        np.testing.assert_array_equal(_u32(RM.sorted_rows(got_t, got_c)), _u32(want), err_msg=f"model, state {n}")


def test_output_does_not_depend_on_the_window():
    window, store = STATES[1]
    first = DS.whole_mesh(window, store, O0, S, MINW, colors=True)
    layers = {k: window[k].copy() for k in ("tsdf", "weight", "color_weight", "color")}
    st = DS.Store()
    for b, words in zip(store["bricks"], DS.words_of({k: store[k] for k in ("tsdf", "weight", "color_weight", "color")}).swapaxes(0, 1)):
        st.bricks[tuple(int(v) for v in b)] = words.copy()
    shift = tuple(int(v) for v in window["window_shift"])
    for delta in ((4, -6, 3), (-4, 6, -3), (1000, -2000, 3000), (-1000, 2000, -3000)):
        shift = st.move(layers, shift, delta)
        layers = {k: np.array(v) for k, v in layers.items()}
        bricks, words = st.content()
        got = DS.whole_mesh({**layers, "window_shift": np.array(shift)}, {**DS.split_words(words, True, False), "bricks": bricks},
                            O0, S, MINW, colors=True)
        np.testing.assert_array_equal(_u32(got[0]), _u32(first[0]), err_msg=str(delta))
        np.testing.assert_array_equal(_u32(got[1]), _u32(first[1]), err_msg=str(delta))
    assert st.dropped == 0
