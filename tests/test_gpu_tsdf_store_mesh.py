"""The mesh of the whole dense map on the device: ``tslam_mesh_extract_whole`` (``k_wmesh_list`` /
``k_wmesh_count`` / ``k_wmesh_emit`` in ``k_tsdf_store_mesh.hip``), ``Handle.mesh_whole`` and
``HipSlamEngine.get_mesh(whole=True)`` against tests/ref_tsdf_store_mesh.py.  Everything is bit-exact:
the vertices are f32 results of one fixed sequence of IEEE operations, and the output's order is
part of the rule.

The sphere's volume is 21 x 13 x 19: off the 8-voxel brick grid on every axis, more than one brick
along each, so window edges cut bricks and cubes reach across bricks; the depth sequences run at
test_gpu_tsdf_store.py's dims (37 x 13 x 41, and 40 x 13 x 41 with colour) and voxel size 0.05,
where no f64 step of a vertex is exact."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import ref_tsdf_store_mesh as RM
from test_gpu_tsdf_follow import MAX_D, MAX_W, ORIGIN, TRUNC_VOX, VOX, H, W, _pose, _records
from test_gpu_tsdf_store import DIMS, DIMS40, P0, _SCam
from thor_slam_amd import dense_store as DS
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

MINW = 1e-4
# -- the analytic sphere ------------------------------------------------------------------------------
SDIMS, SVOX, SORIGIN = (21, 13, 19), 0.0625, (-0.625, -0.375, 1.0)
CENTRE, RADIUS, BAND = np.array([0.031, 0.027, 1.59]), 0.33, 4
SHIFTS = [(5, -3, 9), (-16, 4, -4), (3, -9, 0), (SDIMS[0] + 30, 0, 0)]


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _sphere():
    """tsdf, weight, colour, colour weight of the window at shift 0."""
    nx, ny, nz = SDIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    a = np.stack([i, j, k], axis=-1)
    d = np.linalg.norm(np.array(SORIGIN) + SVOX * (a + 0.5) - CENTRE, axis=-1) - RADIUS
    seen = np.abs(d) < BAND * SVOX
    tsdf = np.where(seen, np.clip(d, -TRUNC_VOX * SVOX, TRUNC_VOX * SVOX), 0.0).astype(np.float32)
    weight = seen.astype(np.float32)
    color = np.where(seen[..., None], (a * np.array([3, 5, 7])) % 251, 0).astype(np.float32)
    return tsdf, weight, color, weight.copy()


class _Sphere:
    """A handle whose volume holds the sphere, with a store of 256 bricks."""

    def __init__(self, color: bool, capacity: int | None = 256, write: bool = True):
        from thor_slam_amd._lib import Handle

        _, rect, _ = _records(False, 2)
        self.h = Handle([rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=2)
        self.color = color
        if color:
            self.h.tsdf_color(True)
        self.h.tsdf_init(SORIGIN, SDIMS, SVOX, TRUNC_VOX, MAX_D, MAX_W)
        if capacity is not None:
            self.h.tsdf_store_init(capacity)
        if write:
            t, w, c, cw = _sphere()
            self.h.tsdf_write(t, w)
            if color:
                self.h.tsdf_write_color(c, cw)

    def whole(self):
        """(triangles, colours or None, bricks visited)"""
        if self.color:
            t, c = self.h.mesh_whole(MINW, colors=True)
            return t, c, self.h.mesh_whole_bricks
        return self.h.mesh_whole(MINW), None, self.h.mesh_whole_bricks

    def close(self):
        self.h.close()


def _device_map(h, color: bool, dims):
    """What the device holds, window and store, as the whole map over the box of the visited bricks:
    (box, lo, shift, store bricks)."""
    t, w = h.tsdf_read()
    window = {"tsdf": t, "weight": w}
    if color:
        window["color"], window["color_weight"] = h.tsdf_read_color()
    shift, _ = h.tsdf_window()
    window["window_shift"] = shift
    bricks, words = h.tsdf_store_read()
    store = {**DS.split_words(words[:, :6 if color else 2], color, False), "bricks": bricks}
    lo, hi = RM.bounds(shift, dims, bricks)
    return DS.assemble(window, store, lo, hi), lo, shift, bricks


def _ref(h, color: bool, dims, origin, vox):
    box, lo, shift, bricks = _device_map(h, color, dims)
    return RM.mesh(box, lo, origin, vox, MINW, shift, dims, bricks)


def _same(got, want, msg=""):
    np.testing.assert_array_equal(_u32(got[0]), _u32(want[0]), err_msg=f"triangles {msg}")
    if want[1] is not None:
        np.testing.assert_array_equal(_u32(got[1]), _u32(want[1]), err_msg=f"colours {msg}")


# -- 1. at shift 0 the whole mesh is the window's mesh; 2. and it stays where the window goes ------------
@pytest.mark.parametrize("color", [False, True])
def test_sphere_wherever_the_window_is(color):
    c = _Sphere(color)
    try:
        first = c.whole()
        want = _ref(c.h, color, SDIMS, SORIGIN, SVOX)
        print("sphere:", len(first[0]), "triangles,", first[2], "bricks", want[2])
        assert len(first[0]) > 500 and first[2] == want[2]["bricks"] == 3 * 2 * 3
        _same(first, want, "against the ref at shift 0")
        win = c.h.mesh(MINW, colors=True) if color else (c.h.mesh(MINW), None)
        assert len(win[0]) == len(first[0])
        np.testing.assert_array_equal(_u32(RM.sorted_rows(first[0], first[1])), _u32(RM.sorted_rows(*win)))
        seen = (_sphere()[1] > 0)
        cubes = np.ones(tuple(n - 1 for n in SDIMS[::-1]), bool)
        for n in range(8):
            cubes &= seen[tuple(slice(d, m - 1 + d) for d, m in zip((n >> 2 & 1, n >> 1 & 1, n & 1), SDIMS[::-1]))]
        assert 0 < cubes.sum() < cubes.size and want[2]["tri_bricks"] < want[2]["bricks"]   # unobserved cubes; bricks off the surface
        total = np.zeros(3, int)
        for n, delta in enumerate(SHIFTS + [None]):
            delta = tuple(-total) if delta is None else delta
            total += delta
            c.h.tsdf_shift(delta)
            got = c.whole()
            ref = _ref(c.h, color, SDIMS, SORIGIN, SVOX)
            assert c.h.tsdf_store_stats()["voxels_dropped"] == 0
            _same(got, first, f"after shift {n} to {total}")
            _same(ref, first, f"ref after shift {n}")
            assert got[2] == ref[2]["bricks"], n
            if n == 0:
                assert ref[2]["seam_cubes"] >= 1
            if n == 3:
                assert ref[2]["split_cubes"] >= 1 and not c.h.tsdf_read()[1].any()
        assert not total.any() and len(c.h.tsdf_store_read()[0]) == 0
    finally:
        c.close()


# -- 3. integrated depth at a voxel size off the exact grid ------------------------------------------------
@pytest.mark.parametrize("color,dims", [(False, DIMS), (True, DIMS40)])
def test_depth_sequence(color, dims):
    c = _SCam(n=4, color=color, dims=dims)
    win = c.window()
    big = dims[0] + 30
    steps = 0

    def check(msg):
        nonlocal steps
        want = _ref(c.h, color, dims, ORIGIN, VOX)      # c.both / c.shift have just checked the device's map against the model
        got = c.h.mesh_whole(MINW, colors=True) if color else (c.h.mesh_whole(MINW), None)
        _same(got, want, msg)
        assert c.h.mesh_whole_bricks == want[2]["bricks"], msg
        steps += 1
        return len(want[0]), want[2]

    try:
        c.both(win, 0, P0, "call 0")
        check("call 0")
        c.shift(win, (-16, 4, -4))
        check("x and z below zero")
        c.both(win, 1, [_pose((-0.7, 0.2, -0.2))], "call 1")
        c.shift(win, (3, -9, 0))
        n, info = check("y below zero")
        assert n > 1000 and info["seam_cubes"] > 0
        c.shift(win, (0, 0, 12))
        c.both(win, 2, [_pose((-0.6, -0.2, 0.4)), _pose((-0.6, -0.2, 0.42), (0.0, 0.03, 0.0))], "call 2")
        check("call 2")
        c.shift(win, (big, 0, 0))
        n, info = check("everything in the store")
        assert n > 1000 and info["split_cubes"] > 0 and info["seam_cubes"] == 0
        c.both(win, 3, [_pose((2.9, -0.2, 0.4))], "call 3, away")
        check("call 3, away")
        c.shift(win, (-big, 5, -8))
        c.both(win, 0, [_pose((-0.6, 0.0, 0.0))], "call 4, back")
        st = c.shift(win, (7, -1, 3))
        check("the end")
        assert win.shift == [-6, -1, 3] and st["voxels_dropped"] == 0 and steps == 7
    finally:
        c.close()


# -- 4. a pool that is too small: the holes are unobserved ---------------------------------------------------
def test_small_pool():
    c = _Sphere(True, capacity=4)
    try:
        first = c.whole()
        c.h.tsdf_shift((12, 0, 0))                   # a dozen bricks' worth leaves, a part of the sphere stays in the window
        st = c.h.tsdf_store_stats()
        assert st["voxels_dropped"] > 0 and st["bricks_allocated"] == 4
        got = c.whole()
        want = _ref(c.h, True, SDIMS, SORIGIN, SVOX)
        print("small pool:", len(got[0]), "of", len(first[0]), "triangles;", st)
        _same(got, want)
        assert 0 < len(got[0]) < len(first[0]) and got[2] == want[2]["bricks"]
    finally:
        c.close()


# -- 5. the shared buffer and the refusals ----------------------------------------------------------------------
def test_buffer_and_refusals():
    c = _Sphere(False)
    lib, h = c.h.lib, c.h.h
    try:
        c.h.tsdf_shift((5, -3, 9))
        whole = c.h.mesh_whole(MINW)
        head = np.zeros((7, 3, 3), np.float32)
        assert lib.tslam_mesh_read(h, head.ctypes.data, 7) == 0
        np.testing.assert_array_equal(_u32(head), _u32(whole[:7]))
        window = c.h.mesh(MINW)                                 # the two extracts share the buffer
        assert 0 < len(window) < len(whole)
        again = np.zeros_like(window)
        assert lib.tslam_mesh_read(h, again.ctypes.data, len(window)) == 0
        np.testing.assert_array_equal(_u32(again), _u32(window))
        assert lib.tslam_mesh_extract_whole(h, MINW, None, None, None) == 0   # null counts
        back = np.zeros_like(whole)
        assert lib.tslam_mesh_read(h, back.ctypes.data, len(whole)) == 0
        np.testing.assert_array_equal(_u32(back), _u32(whole))
        n = ctypes.c_int64(-1)
        assert lib.tslam_mesh_extract_whole(h, MINW, ctypes.byref(n), None, None) == 0 and n.value == len(whole)
        with pytest.raises(RuntimeError, match="error -1.*min_weight"):
            c.h.mesh_whole(-1.0)
        with pytest.raises(RuntimeError, match="error -1.*min_weight"):
            c.h.mesh_whole(float("nan"))
        c.h.tsdf_store_init(0)
        with pytest.raises(RuntimeError, match="error -4.*no brick store"):
            c.h.mesh_whole(MINW)
        np.testing.assert_array_equal(_u32(c.h.mesh(MINW)), _u32(window))
    finally:
        c.close()
    from thor_slam_amd._lib import Handle

    _, rect, _ = _records(False, 2)
    bare = Handle([rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=2)
    try:
        with pytest.raises(RuntimeError, match="error -4.*no TSDF volume"):
            bare.mesh_whole(MINW)
    finally:
        bare.close()


# -- 6. engine end to end ------------------------------------------------------------------------------------------
def test_engine_whole_mesh():
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    n, per, anchor = 18, 6, (8, 6, -46)              # test_gpu_tsdf_store.py's drive
    src = SyntheticRGBDSource(width=W, height=H)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    kw = dict(rgbd=True, dense_map=True, dense_follow=True, dense_follow_step=1, dense_follow_margin=1, batch_size=per,
              dense_follow_anchor=anchor, n_features=1000, n_levels=3, tsdf_origin=ORIGIN, tsdf_dims=DIMS, voxel_size=VOX,
              tsdf_integrator_max_integration_distance_m=MAX_D, tsdf_max_weight=MAX_W)
    cfg = HipSlamConfig(dense_store=True, dense_store_bricks=4096, **kw)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    try:
        for _ in range(n):
            eng.process_frames(rig.get_synchronized_frames())
        eng.flush()
        dm, st = eng.get_dense_map(), eng.get_dense_store()
        assert dm["window_shift"].any() and st["stats"]["voxels_stored"] > 500 and st["stats"]["voxels_dropped"] == 0
        lo, hi = RM.bounds(dm["window_shift"], DIMS, st["bricks"])
        want = RM.mesh(DS.assemble(dm, st, lo, hi), lo, ORIGIN, VOX, cfg.mesh_integrator_min_weight, dm["window_shift"], DIMS,
                       st["bricks"])
        before = eng.get_mesh()
        got = eng.get_mesh(whole=True)
        _same((got["triangles"], got["colors"]), want)
        assert got["bricks"] == want[2]["bricks"] and got["origin"].tolist() == list(ORIGIN) and len(got["triangles"]) > 1000
        np.testing.assert_array_equal(got["world_T_volume"], dm["world_T_volume"])
        after = eng.get_mesh()                       # the window's mesh is what it was
        assert set(after) == {"triangles", "colors", "world_T_volume"} and len(after["triangles"]) < len(got["triangles"])
        for k in ("triangles", "colors"):
            np.testing.assert_array_equal(_u32(after[k]), _u32(before[k]))
    finally:
        eng.shutdown()
    off = HipSlamEngine(num_cameras=2, config=HipSlamConfig(**kw))
    off.initialize(rig.calibration)
    try:
        assert off.get_mesh(whole=True) is None and off.get_mesh() is not None
    finally:
        off.shutdown()
