"""The median and speckle filters of the dense stereo matcher on the device (``k_sd_filter.hip``) vs
their restatement (``tests/ref_stereo_filter.py``) applied to the reference matcher's output: depth
and disp32 bit-exact.  Rendered pairs at the matcher's shapes, every window size, each filter
alone, after semi-global aggregation; hand-made planes through ``stereo_depth_filter_apply`` at the
shapes where the labelling can go wrong (a serpentine that crosses every tile border, checkerboards,
squares of exactly s and of more than s pixels across the tile borders, a random plane with
components on both sides of s, a component larger than any legal s, several frames per call, the
same call twice); the tracking handle's ring-resident images, the engine path, the life cycle and
the argument errors."""

from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import ref_stereo_depth as BOX
import ref_stereo_filter as FLT
import ref_stereo_sgm as SGM
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.camera.rig import CameraRig
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.synthetic import SyntheticStereoSource

pytestmark = pytest.mark.gpu

W0, H0 = 320, 240
ORIGIN = (-2.0, -1.5, 0.5)
DIMS = (80, 60, 100)
MAX_D, MAX_W = 10.0, 100.0
CFG = dict(n_features=1000, n_levels=3, max_disparity=48)   # 48 candidates keep the reference quick
SIZE, RANGE = 50, 32
FXB = 50.0


def _rect_of(src):
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


@functools.lru_cache(maxsize=None)
def _rendered(width, height, baseline=0.3, n=2):
    """n rendered pairs [n][2][H][W] and fx * baseline."""
    src = SyntheticStereoSource(width=width, height=height, baseline=baseline)
    frames = np.stack([np.stack([src.render_image(i, 0), src.render_image(i, 1)]) for i in range(n)])
    frames.setflags(write=False)
    return frames, float(src.get_intrinsics()[0].matrix[0, 0] * baseline)


@functools.lru_cache(maxsize=None)
def _matched(width, height, f, n_disp, sgm=False):
    """The reference matcher's unfiltered disp32 of frame f, computed once."""
    frames, fxb = _rendered(width, height)
    if sgm:
        d = SGM.stereo_depth_sgm(frames[f, 0], frames[f, 1], n_disp, fxb, 100, 1200)[1]
    else:
        d = BOX.stereo_depth(frames[f, 0], frames[f, 1], n_disp, fxb)[1]
    d.setflags(write=False)
    return d


@pytest.fixture(scope="module")
def handle():
    from thor_slam_amd._lib import Handle

    h = Handle([_rect_of(SyntheticStereoSource(width=W0, height=H0))], HipSlamConfig(**CFG), max_batch=4)
    yield h
    h.close()


def _run_images(h, frames, fxb, n_disp, flt=None, sgm=None, init=True):
    """The matcher on caller-supplied images; flt / sgm = keyword arguments of
    Handle.stereo_depth_filter / stereo_depth_sgm, or None to leave that setting alone."""
    import torch

    n, _, hh, ww = frames.shape
    dev = torch.from_numpy(np.array(frames)).cuda()      # a writable copy of the cached input
    if init:
        h.stereo_depth_init(max_frames=n, n_disp=n_disp)
    if sgm is not None:
        h.stereo_depth_sgm(**sgm)
    if flt is not None:
        h.stereo_depth_filter(**flt)
    h.stereo_depth_images(dev.data_ptr(), dev.data_ptr() + ww * hh, 2 * ww * hh, ww, hh, fxb, n,
                          torch.cuda.current_stream().cuda_stream)
    return [h.stereo_depth_read(f) for f in range(n)]


def _apply(h, planes, flt, fxb=FXB, init=True):
    """Hand-made disp32 planes [n][H][W] through stereo_depth_filter_apply."""
    import torch

    planes = np.ascontiguousarray(planes, dtype=np.uint16)
    n, hh, ww = planes.shape
    dev = torch.from_numpy(planes.view(np.int16)).cuda()
    if init:
        h.stereo_depth_init(max_frames=n, n_disp=24)
        h.stereo_depth_filter(**flt)
    h.stereo_depth_filter_apply(dev.data_ptr(), ww, hh, fxb, n, torch.cuda.current_stream().cuda_stream)
    return [h.stereo_depth_read(f) for f in range(n)]


def _assert_same(got, want, what=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"disp32 {what}")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"depth {what}")


def _check_apply(h, planes, m=0, size=0, rng=RANGE, what=""):
    planes = np.asarray(planes, np.uint16)
    planes = planes[None] if planes.ndim == 2 else planes
    got = _apply(h, planes, dict(median=m, speckle_size=size, speckle_range=rng))
    wants = [FLT.filtered(p, FXB, m, size, rng) for p in planes]
    for f, want in enumerate(wants):
        _assert_same(got[f], want, f"{what} frame {f}")
    return wants


# -- rendered pairs ------------------------------------------------------------------------------
# the matcher's shapes: below one step with a ragged band; off every tile size; the handle's size
SHAPES = [(72, 40, 24), (200, 136, 40), (320, 240, 64)]


@pytest.mark.parametrize("m", [3, 5, 7])
@pytest.mark.parametrize("width,height,n_disp", SHAPES)
def test_images_bit_exact(handle, width, height, n_disp, m):
    frames, fxb = _rendered(width, height)
    raw = _matched(width, height, 0, n_disp)
    med = FLT.median(raw, m)
    out = FLT.speckle(med, SIZE, RANGE)
    changed, removed = int((med != raw).sum()), int(((out == 0) & (med != 0)).sum())
    print(f"{width}x{height} m {m}: the median changes {changed} pixels, the speckle step removes {removed}")
    assert changed >= 100           # a kernel that does nothing cannot pass
    assert removed >= 10
    got = _run_images(handle, frames[:1], fxb, n_disp, flt=dict(median=m, speckle_size=SIZE, speckle_range=RANGE))
    _assert_same(got[0], (BOX.depth_from_disp32(out, fxb), out), f"{width}x{height} m {m}")


# widths and heights off every multiple of 8 (the filter's hand-made planes are 75 x 43; here the
# matcher feeds it at such shapes): odd both ways, one column past the matcher's 252-column step, a
# strip of 17 rows.  SIZE_ODD: components of up to 20 pixels, so that the small images lose some.
ODD_SHAPES = [(75, 43, 24), (101, 67, 40), (253, 41, 72), (257, 17, 24)]
SIZE_ODD = 20


@pytest.mark.parametrize("width,height,n_disp", ODD_SHAPES)
def test_images_odd_shapes_median_and_speckle(handle, width, height, n_disp):
    frames, fxb = _rendered(width, height)
    raw = _matched(width, height, 0, n_disp)
    med = FLT.median(raw, 5)
    out = FLT.speckle(med, SIZE_ODD, RANGE)
    changed, removed = int((med != raw).sum()), int(((out == 0) & (med != 0)).sum())
    print(f"{width}x{height}: the median changes {changed} pixels, the speckle step removes {removed}")
    assert changed >= 100 and removed >= 10        # a kernel that does nothing cannot pass
    got = _run_images(handle, frames[:1], fxb, n_disp, flt=dict(median=5, speckle_size=SIZE_ODD, speckle_range=RANGE))
    _assert_same(got[0], (BOX.depth_from_disp32(out, fxb), out), f"{width}x{height}")


def test_images_two_frames(handle):
    frames, fxb = _rendered(72, 40)
    got = _run_images(handle, frames, fxb, 24, flt=dict(median=5, speckle_size=SIZE, speckle_range=RANGE))
    for f in range(2):
        _assert_same(got[f], FLT.filtered(_matched(72, 40, f, 24), fxb, 5, SIZE, RANGE), f"frame {f}")


def test_images_median_only(handle):
    frames, fxb = _rendered(200, 136)
    raw = _matched(200, 136, 0, 40)
    want = FLT.filtered(raw, fxb, 5, 0)
    assert (want[1] != raw).sum() >= 100 and np.array_equal(want[1] != 0, raw != 0)
    _assert_same(_run_images(handle, frames[:1], fxb, 40, flt=dict(median=5, speckle_size=0))[0], want)


def test_images_speckle_only(handle):
    frames, fxb = _rendered(200, 136)
    raw = _matched(200, 136, 0, 40)
    want = FLT.filtered(raw, fxb, 0, SIZE, RANGE)
    assert ((want[1] == 0) & (raw != 0)).sum() >= 10
    _assert_same(_run_images(handle, frames[:1], fxb, 40, flt=dict(median=0, speckle_size=SIZE, speckle_range=RANGE))[0], want)


@pytest.mark.parametrize("order", ["sgm first", "filter first"])
def test_images_after_sgm(handle, order):
    """Semi-global aggregation and the filters, set in either order."""
    import torch

    frames, fxb = _rendered(200, 136)
    raw = _matched(200, 136, 0, 40, sgm=True)
    want = FLT.filtered(raw, fxb, 5, SIZE, RANGE)
    assert (want[1] != raw).sum() >= 100
    assert not np.array_equal(raw, _matched(200, 136, 0, 40))
    if order == "sgm first":
        got = _run_images(handle, frames[:1], fxb, 40, sgm={}, flt=dict(median=5, speckle_size=SIZE, speckle_range=RANGE))
    else:
        handle.stereo_depth_init(max_frames=1, n_disp=40)
        handle.stereo_depth_filter(median=5, speckle_size=SIZE, speckle_range=RANGE)
        got = _run_images(handle, frames[:1], fxb, 40, sgm={}, init=False)
    _assert_same(got[0], want, order)
    # semi-global aggregation off again: the filters stay
    handle.stereo_depth_sgm(enable=False)
    got = _run_images(handle, frames[:1], fxb, 40, init=False)
    _assert_same(got[0], FLT.filtered(_matched(200, 136, 0, 40), fxb, 5, SIZE, RANGE), "after SGM off")
    torch.cuda.synchronize()


# -- hand-made planes ----------------------------------------------------------------------------
def _serpentine(width, height, r):
    """A one-pixel path along every other row, joined at alternating ends, whose values form a
    triangle wave of step r along the path; (plane, length)."""
    path = []
    for k, y in enumerate(range(0, height, 2)):
        xs = range(width) if k % 2 == 0 else range(width - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 2 < height:
            path.append((y + 1, width - 1 if k % 2 == 0 else 0))
    i = np.arange(len(path))
    tri = np.abs((i % 200) - 100)                        # 100 .. 0 .. 100, steps of 1
    a = np.zeros((height, width), np.uint16)
    ys, xs = np.array(path).T
    a[ys, xs] = 64 + r * tri
    return a, len(path)


def test_serpentine_is_one_component(handle):
    a, n = _serpentine(200, 136, RANGE)
    assert n == 68 * 200 + 67 and n <= 65535 and int(a.max()) == 64 + 100 * RANGE <= 8191
    assert FLT.components(a, RANGE)[1] == [n]
    kept, = _check_apply(handle, a, size=n - 1, what="serpentine kept")
    np.testing.assert_array_equal(kept[1], a)
    gone, = _check_apply(handle, a, size=n, what="serpentine removed")
    assert not gone[1].any()
    # one unit less of range and every pixel stands alone
    alone, = _check_apply(handle, a, size=1, rng=RANGE - 1, what="serpentine, range r - 1")
    assert not alone[1].any()


def test_checkerboards(handle):
    yy, xx = np.mgrid[0:43, 0:75]
    odd = ((yy + xx) & 1).astype(np.uint16)
    holes = odd * 640                                            # valid / zero: every valid pixel alone
    steps_out = (640 + odd * (RANGE + 1)).astype(np.uint16)      # all valid, neighbours r + 1 apart
    steps_in = (640 + odd * RANGE).astype(np.uint16)             # neighbours r apart: one component
    assert set(FLT.components(holes, RANGE)[1]) == {1} and set(FLT.components(steps_out, RANGE)[1]) == {1}
    assert FLT.components(steps_in, RANGE)[1] == [43 * 75]
    for plane, name in ((holes, "holes"), (steps_out, "r + 1")):
        out, = _check_apply(handle, plane, size=1, what=name)
        assert not out[1].any()
    kept, = _check_apply(handle, steps_in, size=43 * 75 - 1, what="r, kept")
    np.testing.assert_array_equal(kept[1], steps_in)
    gone, = _check_apply(handle, steps_in, size=43 * 75, what="r, removed")
    assert not gone[1].any()


def _squares(k):
    """k x k squares on a zero background of the handle's size, each laid across a border of the
    kernels' tiles: x and y = 16, 32, 64 and x = 252 .. 256."""
    a = np.zeros((H0, W0), np.uint16)
    spots = [(xb - 3, yb - 3) for yb in (16, 32, 64) for xb in (16, 32, 64, 256)]
    spots += [(xb - 3, 100 + 20 * i) for i, xb in enumerate((252, 253, 254, 255, 256))]
    for x, y in spots:
        assert not a[y - 1:y + k + 1, x - 1:x + k + 1].any()     # squares do not touch
        a[y:y + k, x:x + k] = 320 + 8 * len(spots)
    return a, len(spots)


def test_squares_of_s_go_and_larger_ones_stay(handle):
    k = 7
    small, n = _squares(k)
    large, _ = _squares(k + 1)
    assert FLT.components(small, RANGE)[1] == [k * k] * n and FLT.components(large, RANGE)[1] == [(k + 1) ** 2] * n
    got_small, got_large = _check_apply(handle, np.stack([small, large]), size=k * k, what="squares")
    assert not got_small[1].any()
    np.testing.assert_array_equal(got_large[1], large)


def _random_plane(seed, shape=(43, 75)):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 40, 60, 200], np.uint16), size=shape, p=(0.4, 0.26, 0.26, 0.08))


def test_random_plane_components_on_both_sides_of_s(handle):
    """75 x 43, values {0, 40, 60, 200}, 60 % non-zero, r = 32: 40 and 60 link, 200 does not.  The
    reference's components have at least 20 distinct sizes on either side of s (seed 7: 40 distinct
    sizes, 1 .. 134; s is the 20th)."""
    a = _random_plane(7)
    sizes = sorted(set(FLT.components(a, RANGE)[1]))
    s = sizes[len(sizes) // 2 - 1]
    below, above = [v for v in sizes if v <= s], [v for v in sizes if v > s]
    print(f"{len(sizes)} distinct sizes, s = {s}: {len(below)} at or below, {len(above)} above; non-zero {(a != 0).mean():.3f}")
    assert len(below) >= 20 and len(above) >= 20
    assert 0.55 <= (a != 0).mean() <= 0.65
    out, = _check_apply(handle, a, size=s, what="random plane")
    assert out[1].any() and (out[1] != a).any()


def test_component_larger_than_any_size_stays(handle):
    big = np.full((H0, W0), 800, np.uint16)                  # 76,800 pixels > 65,535
    out, = _check_apply(handle, big, size=65535, what="constant 320x240")
    np.testing.assert_array_equal(out[1], big)
    small = np.full((40, 72), 800, np.uint16)
    out, = _check_apply(handle, small, size=65535, what="constant 72x40")
    assert not out[1].any()


def test_three_frames_and_the_same_call_twice(handle):
    planes = np.stack([_random_plane(seed) for seed in (2, 3, 4)])
    assert not np.array_equal(planes[0], planes[1]) and not np.array_equal(planes[1], planes[2])
    flt = dict(median=3, speckle_size=12, speckle_range=RANGE)
    first = _apply(handle, planes, flt)
    wants = [FLT.filtered(p, FXB, 3, 12, RANGE) for p in planes]
    assert len({w[1].tobytes() for w in wants}) == 3
    for f in range(3):
        _assert_same(first[f], wants[f], f"frame {f}")
    again = _apply(handle, planes, flt, init=False)          # the planes are initialised per call
    for f in range(3):
        _assert_same(again[f], first[f], f"second call, frame {f}")
    # another input in between leaves nothing behind
    _apply(handle, planes[::-1], flt, init=False)
    third = _apply(handle, planes, flt, init=False)
    for f in range(3):
        _assert_same(third[f], first[f], f"third call, frame {f}")


@pytest.mark.parametrize("m", [3, 5, 7])
def test_median_on_random_planes(handle, m):
    """Every 13-bit value, 30 % zeros: the selection has to be exact at every bit."""
    rng = np.random.default_rng(10 + m)
    a = rng.integers(1, 8192, (43, 75)).astype(np.uint16)
    a[rng.random(a.shape) < 0.3] = 0
    a[0, :8] = [8191, 8191, 1, 1, 8191, 0, 8191, 1]          # the extremes next to each other, on a border
    out, = _check_apply(handle, a, m=m, what=f"median {m}")
    assert np.array_equal(out[1] != 0, a != 0) and (out[1] != a).sum() >= 100


def test_values_above_8191_count_as_8191(handle):
    rng = np.random.default_rng(5)
    a = rng.choice(np.array([0, 8100, 8191, 8192, 9000, 40000, 65535], np.uint16), size=(43, 75))
    flt = dict(median=3, speckle_size=4, speckle_range=91)   # 8100 and 8191 link
    got = _apply(handle, a[None], flt)[0]
    clamped = np.minimum(a, 8191).astype(np.uint16)
    assert (clamped != a).sum() >= 100
    _assert_same(got, FLT.filtered(clamped, FXB, 3, 4, 91))
    assert got[1].max() == 8191


# -- tracking-handle path ------------------------------------------------------------------------
def _level0(h, g, cam):
    blk = h.frame_block("pyramid", h.ring_slot(g), np.uint8).reshape(h.n_cams, h.pyr_bytes)
    return blk[cam, h.pyr_off[0]:h.pyr_off[0] + h.width * h.height].reshape(h.height, h.width)


def test_tracking_handle_bit_exact():
    import torch

    from thor_slam_amd._lib import Handle

    n = 2
    src = SyntheticStereoSource(width=W0, height=H0)
    rect = _rect_of(src)
    dev = torch.from_numpy(np.ascontiguousarray(src.render_stereo_sequence(n))).cuda()
    s = torch.cuda.current_stream().cuda_stream
    res = []
    for on in (False, True):
        h = Handle([rect], HipSlamConfig(**CFG), max_batch=n)
        h.submit(dev.data_ptr(), n, s)
        h.stereo_depth_init(max_frames=n)           # n_disp = the handle's max_disparity
        if on:
            h.stereo_depth_filter()                 # median 5, speckle (50, 32)
        h.stereo_depth(0, n, pair=0, stream=s)
        if on:
            for f in range(n):
                raw = BOX.stereo_depth(_level0(h, f, 0), _level0(h, f, 1), CFG["max_disparity"], rect.fx * rect.baseline)[1]
                want = FLT.filtered(raw, rect.fx * rect.baseline, 5, SIZE, RANGE)
                assert (want[0] > 0).mean() > 0.5 and (want[1] != raw).sum() >= 100
                _assert_same(h.stereo_depth_read(f), want, f"of frame {f}")
        res.append(h.read_poses(n))
        h.close()
    for k in ("T_abs", "T_rel", "stats"):
        np.testing.assert_array_equal(res[0][k], res[1][k], err_msg=k)


# -- engine --------------------------------------------------------------------------------------
def _engine_run(n=4, **kw):
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.slam.hip_engine import HipSlamEngine

    src = SyntheticStereoSource(width=W0, height=H0)
    rig = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    rig.start()
    cfg = HipSlamConfig(**CFG, batch_size=2, tsdf_origin=ORIGIN, tsdf_dims=DIMS, tsdf_integrator_max_integration_distance_m=MAX_D,
                        tsdf_max_weight=MAX_W, enable_loop_closure=False, dense_map=True, stereo_depth=True, **kw)
    eng = HipSlamEngine(num_cameras=2, config=cfg)
    eng.initialize(rig.calibration)
    poses = []
    for _ in range(n):
        p = eng.process_frames(rig.get_synchronized_frames())
        poses.append(None if p is None else p.to_4x4_matrix())
    eng.flush()
    poses.append(eng._latest_pose.to_4x4_matrix())
    return eng, src, poses


def test_engine_depth_is_filtered_and_tracking_untouched():
    run = {}
    for on in (True, False):
        kw = dict(stereo_depth_median=5, stereo_depth_speckle_size=SIZE) if on else {}
        eng, src, poses = _engine_run(**kw)
        r = {"poses": poses, "depth": eng.get_depth_image()[0]}
        if on:
            h, rect = eng._handle, _rect_of(src)
            fxb = rect.fx * rect.baseline
            raw = BOX.stereo_depth(_level0(h, 3, 0), _level0(h, 3, 1), CFG["max_disparity"], fxb)[1]
            r["want"] = FLT.filtered(raw, fxb, 5, SIZE, RANGE)[0]
        eng.shutdown()
        run[on] = r
    np.testing.assert_array_equal(run[True]["depth"], run[True]["want"])
    assert not np.array_equal(run[True]["depth"], run[False]["depth"])
    n_on, n_off = int((run[True]["depth"] > 0).sum()), int((run[False]["depth"] > 0).sum())
    print(f"depth pixels: filtered {n_on}, unfiltered {n_off}")
    assert 0 < n_on <= n_off
    poses, raw_poses = run[True]["poses"], run[False]["poses"]
    assert len(poses) == len(raw_poses) == 5 and poses[-1] is not None
    for a, b in zip(poses, raw_poses):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_array_equal(a, b)


# -- life cycle and errors -----------------------------------------------------------------------
def test_switching_off(handle):
    frames, fxb = _rendered(72, 40)
    raw = _run_images(handle, frames, fxb, 24)
    flt = _run_images(handle, frames, fxb, 24, flt={})
    assert not np.array_equal(flt[0][1], raw[0][1])
    off = _run_images(handle, frames, fxb, 24, flt=dict(enable=False), init=False)
    for f in range(2):
        _assert_same(off[f], raw[f], f"after enable=False, frame {f}")
        _assert_same(off[f], BOX.stereo_depth(frames[f, 0], frames[f, 1], 24, fxb), f"vs the box reference, frame {f}")
    handle.stereo_depth_filter()
    again = _run_images(handle, frames, fxb, 24)      # stereo_depth_init alone: the filters are off again
    for f in range(2):
        _assert_same(again[f], raw[f], f"after a new init, frame {f}")


def test_errors_launch_nothing(handle):
    import torch

    from thor_slam_amd import _lib
    from thor_slam_amd._lib import Handle

    lib = _lib.load_library()
    EINVAL, ESTATE = -1, -4

    def flt(h, enable=1, median=5, size=50, rng=32, reserved=(0, 0, 0, 0)):
        prm = (ctypes.c_int32 * 8)(enable, median, size, rng, *reserved)
        return lib.tslam_stereo_depth_filter(h.h, ctypes.addressof(prm))

    def apply(h, dev, w=72, hh=40, fxb=FXB, n=1):
        return lib.tslam_stereo_depth_filter_apply(h.h, ctypes.c_void_p(dev.data_ptr() if dev is not None else None), w, hh,
                                                   ctypes.c_double(fxb), n, None)

    plane = torch.full((2, 40, 72), 640, dtype=torch.int16, device="cuda")
    fresh = Handle([_rect_of(SyntheticStereoSource(width=W0, height=H0))], HipSlamConfig(**CFG), max_batch=2)
    assert flt(fresh) == ESTATE                                   # before tslam_stereo_depth_init
    assert flt(fresh, enable=0) == ESTATE
    assert apply(fresh, plane) == ESTATE
    fresh.stereo_depth_init(max_frames=2, n_disp=24)
    assert apply(fresh, plane) == ESTATE                          # the filters are off
    dev = torch.zeros((1, 2, H0, W0), dtype=torch.uint8, device="cuda")
    fresh.begin_batch(dev.data_ptr(), 1)
    assert flt(fresh) == ESTATE                                   # inside a batch
    fresh.end_batch()
    assert flt(fresh) == 0
    fresh.begin_batch(dev.data_ptr(), 1)
    assert apply(fresh, plane) == ESTATE
    fresh.end_batch()
    assert apply(fresh, plane) == 0
    assert flt(fresh, enable=0) == 0
    assert apply(fresh, plane) == ESTATE                          # off again
    fresh.close()

    frames, fxb = _rendered(72, 40)
    setting = dict(median=3, speckle_size=20, speckle_range=RANGE)
    before = _run_images(handle, frames, fxb, 24, flt=setting)
    for median in (1, 2, 4, 6, 9, -3):
        assert flt(handle, median=median) == EINVAL
    assert flt(handle, size=-1) == EINVAL and flt(handle, size=65536) == EINVAL
    assert flt(handle, rng=-1) == EINVAL and flt(handle, rng=8192) == EINVAL
    assert flt(handle, median=0, size=0) == EINVAL                # enable with nothing to do
    for r in ((1, 0, 0, 0), (0, 0, 0, 7)):
        assert flt(handle, reserved=r) == EINVAL
        assert flt(handle, enable=0, reserved=r) == EINVAL
    assert lib.tslam_last_error()
    assert apply(handle, None) == EINVAL
    assert apply(handle, plane, w=15) == EINVAL and apply(handle, plane, hh=15) == EINVAL
    assert apply(handle, plane, w=W0 + 1) == EINVAL and apply(handle, plane, hh=H0 + 1) == EINVAL
    assert apply(handle, plane, n=3) == EINVAL and apply(handle, plane, n=-1) == EINVAL
    assert apply(handle, plane, fxb=0.0) == EINVAL
    for f in range(2):
        _assert_same(handle.stereo_depth_read(f), before[f], f"after the refused calls, frame {f}")
    # the setting survived them: the same call gives the same output
    after = _run_images(handle, frames, fxb, 24, init=False)
    for f in range(2):
        _assert_same(after[f], before[f], f"of a call after the refused ones, frame {f}")
        _assert_same(after[f], FLT.filtered(_matched(72, 40, f, 24), fxb, **dict(m=3, size=20, rng=RANGE)), f"frame {f}")
