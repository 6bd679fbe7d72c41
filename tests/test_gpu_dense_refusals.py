"""Every refusal of the dense-map entry points (tslam_tsdf_*, tslam_mesh_*, tslam_esdf_*,
tslam_stereo_depth_*): the return code and the full ``tslam_last_error()`` text, one fault at a
time, and the calls with two faults where the order of the opening checks decides which one is
reported.  Every case is refused on the host before anything is launched; the handles are the
smallest the dense tests build, the volume is 8 x 8 x 8, and one frame is submitted so that a
"last batch" exists.

Each table row is (name, call, return code, text); ``call`` gets the test's context ``c``.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from test_gpu_tsdf_render import H, W, _handle, _records, _stream
from thor_slam_amd._lib import (StereoDepthFilterParams, StereoDepthSgmParams, TsdfAlignParams, TsdfFollowParams,
                                TsdfRenderParams, TsdfRigCamera)
from thor_slam_amd.params import HipSlamConfig

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
S = 2 * W * H                      # bytes of one depth image
VOL = "no TSDF volume (tslam_tsdf_init)"
RND = "no render state (tslam_tsdf_render_init)"
ALN = "no align state (tslam_tsdf_align_init)"
SD = "no stereo depth buffers (tslam_stereo_depth_init)"
LAST = "device poses: frames must belong to the last batch"
DEPTH = "bad depth / stride"
NOCOL = "no colour layer (tslam_tsdf_color before tslam_tsdf_init)"


class Ctx:
    """A handle, a device buffer that stands for every image argument (no refused call reads it)
    and the host arguments the calls share."""

    def __init__(self, h):
        import torch

        self.hd = h
        self.lib = h.lib
        self.h = h.h
        self.buf = torch.zeros(16 * W * H, dtype=torch.uint8, device="cuda")
        self.D = self.buf.data_ptr()
        self.eye = np.ascontiguousarray(np.stack([np.eye(4)] * 4))
        self.E = self.eye.ctypes.data
        self.origin = np.zeros(3)
        self.dims = np.array([8, 8, 8], dtype=np.int32)
        self.host = np.zeros(16 * 8 * 8 * 8, dtype=np.float32)   # any host output / input
        self.P = self.host.ctypes.data
        self.keep = []

    def g0(self):
        """The first frame of the last batch (every batch of these tests has one frame)."""
        return max(self.hd.frames_done - 1, 0)

    def ptr(self, obj):
        """The address of a ctypes object or an array that stays alive with the context."""
        self.keep.append(obj)
        return obj.ctypes.data if isinstance(obj, np.ndarray) else ctypes.addressof(obj)

    def i32(self, *v):
        return self.ptr(np.array(v, dtype=np.int32))

    def f64(self, *v):
        return self.ptr(np.array(v, dtype=np.float64))

    def volume(self, dims=(8, 8, 8)):
        assert self.lib.tslam_tsdf_init(self.h, self.origin.ctypes.data, self.i32(*dims), 0.05, 4.0, 10.0, 100.0) == 0

    def follow(self, anchor=(0, 0, 0), margin=2, step=1):
        return self.ptr(TsdfFollowParams((ctypes.c_int32 * 3)(*anchor), margin, step))

    def render(self, **kw):
        p = dict(width=8, height=8, fx=8.0, fy=8.0, cx=3.5, cy=3.5, min_weight=1e-4, min_depth=0.0, max_depth=10.0,
                 step_scale=0.5, outputs=5, reserved=0)
        p.update(kw)
        return self.ptr(TsdfRenderParams(*[p[k] for k, _ in TsdfRenderParams._fields_]))

    def align(self, reserved=(0, 0, 0, 0), **kw):
        p = dict(iterations=2, min_inliers=6, max_distance=0.1, min_weight=1e-4, max_depth=10.0, step_scale=0.5,
                 max_translation=0.5, max_rotation=0.5, eps_translation=0.0, eps_rotation=0.0, min_pivot=1e-6)
        p.update(kw)
        return self.ptr(TsdfAlignParams(*[p[k] for k, _ in TsdfAlignParams._fields_[:-1]], (ctypes.c_int32 * 4)(*reserved)))

    def cams(self, *cams):
        """Cameras (pair, depth, color, stride) of tslam_tsdf_integrate_rig."""
        arr = (TsdfRigCamera * len(cams))(*[TsdfRigCamera(c[0], 0, c[1] or None, c[2] or None, c[3]) for c in cams])
        return self.ptr(arr)

    def sgm(self, enable=1, p1=100, p2=1200, paths=15, chunk=0, reserved=(0, 0, 0)):
        return self.ptr(StereoDepthSgmParams(enable, p1, p2, paths, chunk, (ctypes.c_int32 * 3)(*reserved)))

    def flt(self, enable=1, median=5, size=50, rng=32, reserved=(0, 0, 0, 0)):
        return self.ptr(StereoDepthFilterParams(enable, median, size, rng, (ctypes.c_int32 * 4)(*reserved)))


def _check(c, table):
    """Every row of the table against the library; the rows that differ, with what came back."""
    bad = []
    for name, call, rc, text in table:
        got = call(c)
        msg = c.lib.tslam_last_error().decode() if got != 0 else ""
        print(f"{name}: {got} {msg!r}")
        if (got, msg) != (rc, text):
            bad.append((name, got, msg))
    assert not bad, bad


def _integrate(fn, pair=0, depth=True, stride=S, n=1, first=0, host=True, h=True):
    """tslam_tsdf_integrate / _rect with one argument off."""
    return lambda c: getattr(c.lib, fn)(c.h if h else None, pair, c.D if depth else None, stride, n, c.g0() + first,
                                        c.E if host else None, None)


def _rgbd(pair=0, color=True, depth=True, host=True, h=True):
    return lambda c: c.lib.tslam_tsdf_integrate_rgbd(c.h if h else None, pair, c.D if color else None, c.D if depth else None,
                                                     S, 1, 0, c.E if host else None, None)


def _rig(cams=((0, 1, 0, S),), n_cams=None, n=1, first=0, host=True, h=True):
    def call(c):
        cm = [(p, c.D if d else 0, c.D if col else 0, st) for p, d, col, st in cams]
        return c.lib.tslam_tsdf_integrate_rig(c.h if h else None, c.cams(*cm) if cams else None,
                                              len(cams) if n_cams is None else n_cams, n, c.g0() + first, c.E if host else None, None)
    return call


def _render(pair=0, n=1, first=0, host=True, h=True):
    return lambda c: c.lib.tslam_tsdf_render(c.h if h else None, pair, c.E if host else None, n, c.g0() + first, None)


def _align(depth=True, stride=S, n=1, first=0, host=True, h=True):
    return lambda c: c.lib.tslam_tsdf_align(c.h if h else None, c.D if depth else None, stride, n, c.g0() + first,
                                            c.E if host else None, None)


def _aligned(color=False, depth=True, stride=S, n=1, h=True):
    return lambda c: c.lib.tslam_tsdf_integrate_aligned(c.h if h else None, c.D if color else None, c.D if depth else None,
                                                        stride, n, None)


def _align_init(pair=0, max_frames=1, prm=True, **kw):
    return lambda c: c.lib.tslam_tsdf_align_init(c.h, pair, 1, c.align(**kw) if prm else None, max_frames)


def _render_init(max_views=1, **kw):
    return lambda c: c.lib.tslam_tsdf_render_init(c.h, c.render(**kw), max_views)


INTEGRATE = ("tslam_tsdf_integrate", "tslam_tsdf_integrate_rect")

# -- a null handle -------------------------------------------------------------------------------------
NULL_HANDLE = [
    ("tsdf_init", lambda c: c.lib.tslam_tsdf_init(None, c.f64(0, 0, 0), c.i32(8, 8, 8), 0.05, 4.0, 10.0, 100.0), EINVAL, "bad argument"),
    ("integrate", _integrate(INTEGRATE[0], h=False), EINVAL, "bad handle or pair"),
    ("integrate_rect", _integrate(INTEGRATE[1], h=False), EINVAL, "bad handle or pair"),
    ("integrate_rgbd", _rgbd(h=False), EINVAL, "bad handle or pair"),
    ("integrate_rgbd, no colour either", _rgbd(h=False, color=False), EINVAL, "null colour images"),
    ("integrate_rig", _rig(h=False), EINVAL, "bad argument"),
    ("follow", lambda c: c.lib.tslam_tsdf_follow(None, c.follow()), EINVAL, "null handle"),
    ("shift", lambda c: c.lib.tslam_tsdf_shift(None, c.i32(1, 0, 0), None), EINVAL, "bad argument"),
    ("window", lambda c: c.lib.tslam_tsdf_window(None, c.P, c.P), ESTATE, VOL),
    ("color", lambda c: c.lib.tslam_tsdf_color(None, 1), EINVAL, "null handle"),
    ("render_init", lambda c: c.lib.tslam_tsdf_render_init(None, c.render(), 1), EINVAL, "bad argument"),
    ("render", _render(h=False), EINVAL, "bad handle or pair"),
    ("render_buffers", lambda c: c.lib.tslam_tsdf_render_buffers(None, None, None, None, None, None), EINVAL, "null handle"),
    ("render_read", lambda c: c.lib.tslam_tsdf_render_read(None, 0, c.P, None, None, None), EINVAL, "null handle"),
    ("align_init", lambda c: c.lib.tslam_tsdf_align_init(None, 0, 1, c.align(), 1), EINVAL, "null handle"),
    ("align", _align(h=False), EINVAL, "null handle"),
    ("align_read", lambda c: c.lib.tslam_tsdf_align_read(None, 1, c.P, None, None, None), EINVAL, "null handle"),
    ("align_buffers", lambda c: c.lib.tslam_tsdf_align_buffers(None, None, None), EINVAL, "null handle"),
    ("integrate_aligned", _aligned(h=False), EINVAL, "null handle"),
    ("read", lambda c: c.lib.tslam_tsdf_read(None, c.P, c.P), ESTATE, VOL),
    ("write", lambda c: c.lib.tslam_tsdf_write(None, c.P, c.P), ESTATE, VOL),
    ("read_color", lambda c: c.lib.tslam_tsdf_read_color(None, c.P, c.P), ESTATE, "no colour layer"),
    ("write_color", lambda c: c.lib.tslam_tsdf_write_color(None, c.P, c.P), ESTATE, "no colour layer"),
    ("mesh_extract", lambda c: c.lib.tslam_mesh_extract(None, 1e-4, None, None), ESTATE, VOL),
    ("mesh_read", lambda c: c.lib.tslam_mesh_read(None, c.P, 1), ESTATE, VOL),
    ("mesh_read_colors", lambda c: c.lib.tslam_mesh_read_colors(None, c.P, 1), ESTATE, "no colour layer mesh"),
    ("esdf_compute", lambda c: c.lib.tslam_esdf_compute(None, 0.2, 1.0, 1e-4, None), ESTATE, VOL),
    ("esdf_read", lambda c: c.lib.tslam_esdf_read(None, c.P), ESTATE, "no ESDF (tslam_esdf_compute)"),
    ("esdf_slice", lambda c: c.lib.tslam_esdf_slice(None, 0, 1, 0.2, 1.0, 1e-4, c.P), ESTATE, VOL),
    ("stereo_depth_init", lambda c: c.lib.tslam_stereo_depth_init(None, c.i32(0, 10, 1, 0), 1), EINVAL, "bad argument"),
    ("stereo_depth_sgm", lambda c: c.lib.tslam_stereo_depth_sgm(None, c.sgm()), EINVAL, "bad argument"),
    ("stereo_depth_filter", lambda c: c.lib.tslam_stereo_depth_filter(None, c.flt()), EINVAL, "bad argument"),
    ("stereo_depth_filter_apply", lambda c: c.lib.tslam_stereo_depth_filter_apply(None, c.D, 16, 16, 1.0, 1, None), EINVAL, "bad argument"),
    ("stereo_depth", lambda c: c.lib.tslam_stereo_depth(None, 0, 0, 1, None), EINVAL, "bad handle or pair"),
    ("stereo_depth_slots", lambda c: c.lib.tslam_stereo_depth_slots(None, 0, 0, 1, 0, None), EINVAL, "bad handle or pair"),
    ("stereo_depth_images", lambda c: c.lib.tslam_stereo_depth_images(None, c.D, c.D, W * H, 16, 16, 1.0, 1, None), EINVAL, "bad argument"),
    ("stereo_depth_buffers", lambda c: c.lib.tslam_stereo_depth_buffers(None, None, None, None), EINVAL, "null handle"),
    ("stereo_depth_read", lambda c: c.lib.tslam_stereo_depth_read(None, 0, c.P, c.P), EINVAL, "null handle"),
]

# -- an RGB-D handle before tslam_tsdf_init ------------------------------------------------------------
NO_VOLUME = [
    ("tsdf_init, null origin", lambda c: c.lib.tslam_tsdf_init(c.h, None, c.i32(8, 8, 8), 0.05, 4.0, 10.0, 100.0), EINVAL, "bad argument"),
    ("tsdf_init, null dims", lambda c: c.lib.tslam_tsdf_init(c.h, c.f64(0, 0, 0), None, 0.05, 4.0, 10.0, 100.0), EINVAL, "bad argument"),
    ("tsdf_init, dims 0", lambda c: c.lib.tslam_tsdf_init(c.h, c.f64(0, 0, 0), c.i32(8, 0, 8), 0.05, 4.0, 10.0, 100.0), EINVAL,
     "dims must be >= 1 with at most 2^31 voxels"),
    ("tsdf_init, too many voxels", lambda c: c.lib.tslam_tsdf_init(c.h, c.f64(0, 0, 0), c.i32(2048, 2048, 513), 0.05, 4.0, 10.0, 100.0),
     EINVAL, "dims must be >= 1 with at most 2^31 voxels"),
    ("tsdf_init, voxel size 0", lambda c: c.lib.tslam_tsdf_init(c.h, c.f64(0, 0, 0), c.i32(8, 8, 8), 0.0, 4.0, 10.0, 100.0), EINVAL,
     "voxel_size, trunc_vox, max_dist must be > 0 and max_weight >= 1"),
    ("tsdf_init, max_weight below 1", lambda c: c.lib.tslam_tsdf_init(c.h, c.f64(0, 0, 0), c.i32(8, 8, 8), 0.05, 4.0, 10.0, 0.5), EINVAL,
     "voxel_size, trunc_vox, max_dist must be > 0 and max_weight >= 1"),
    ("integrate", _integrate(INTEGRATE[0]), ESTATE, VOL),
    ("integrate_rect", _integrate(INTEGRATE[1]), ESTATE, VOL),
    ("integrate_rgbd", _rgbd(), ESTATE, NOCOL),
    ("integrate, and a bad pair", _integrate(INTEGRATE[0], pair=1), EINVAL, "bad handle or pair"),
    ("integrate, and null depth", _integrate(INTEGRATE[0], depth=False), ESTATE, VOL),
    ("integrate_rig", _rig(), ESTATE, "no rig set (tslam_set_rig)"),
    ("follow", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow()), ESTATE, VOL),
    ("follow off", lambda c: c.lib.tslam_tsdf_follow(c.h, None), ESTATE, VOL),
    ("shift", lambda c: c.lib.tslam_tsdf_shift(c.h, c.i32(1, 0, 0), None), ESTATE, VOL),
    ("shift, null delta", lambda c: c.lib.tslam_tsdf_shift(c.h, None, None), EINVAL, "bad argument"),
    ("window", lambda c: c.lib.tslam_tsdf_window(c.h, c.P, c.P), ESTATE, VOL),
    ("render_init", _render_init(), ESTATE, VOL),
    ("render_init, null params", lambda c: c.lib.tslam_tsdf_render_init(c.h, None, 1), EINVAL, "bad argument"),
    ("render_init, and a bad width", _render_init(width=0), ESTATE, VOL),
    ("render", _render(), ESTATE, VOL),
    ("render, and a bad pair", _render(pair=1), EINVAL, "bad handle or pair"),
    ("render_buffers", lambda c: c.lib.tslam_tsdf_render_buffers(c.h, None, None, None, None, None), ESTATE, RND),
    ("render_read", lambda c: c.lib.tslam_tsdf_render_read(c.h, 0, None, None, None, None), ESTATE, RND),
    ("align_init", _align_init(), ESTATE, VOL),
    ("align_init off", _align_init(prm=False), ESTATE, VOL),
    ("align_init, and a bad pair", _align_init(pair=1), ESTATE, VOL),
    ("align", _align(), ESTATE, VOL),
    ("align, and null depth", _align(depth=False), ESTATE, VOL),
    ("align_read", lambda c: c.lib.tslam_tsdf_align_read(c.h, 1, c.P, None, None, None), ESTATE, ALN),
    ("align_buffers", lambda c: c.lib.tslam_tsdf_align_buffers(c.h, None, None), ESTATE, ALN),
    ("integrate_aligned", _aligned(), ESTATE, VOL),
    ("read", lambda c: c.lib.tslam_tsdf_read(c.h, c.P, c.P), ESTATE, VOL),
    ("write", lambda c: c.lib.tslam_tsdf_write(c.h, c.P, c.P), ESTATE, VOL),
    ("write, and null volumes", lambda c: c.lib.tslam_tsdf_write(c.h, None, None), ESTATE, VOL),
    ("read_color", lambda c: c.lib.tslam_tsdf_read_color(c.h, c.P, c.P), ESTATE, "no colour layer"),
    ("write_color", lambda c: c.lib.tslam_tsdf_write_color(c.h, c.P, c.P), ESTATE, "no colour layer"),
    ("mesh_extract", lambda c: c.lib.tslam_mesh_extract(c.h, 1e-4, None, None), ESTATE, VOL),
    ("mesh_extract, and a bad weight", lambda c: c.lib.tslam_mesh_extract(c.h, -1.0, None, None), ESTATE, VOL),
    ("mesh_read", lambda c: c.lib.tslam_mesh_read(c.h, c.P, 1), ESTATE, VOL),
    ("mesh_read_colors", lambda c: c.lib.tslam_mesh_read_colors(c.h, c.P, 1), ESTATE, "no colour layer mesh"),
    ("esdf_compute", lambda c: c.lib.tslam_esdf_compute(c.h, 0.2, 1.0, 1e-4, None), ESTATE, VOL),
    ("esdf_read", lambda c: c.lib.tslam_esdf_read(c.h, c.P), ESTATE, "no ESDF (tslam_esdf_compute)"),
    ("esdf_slice", lambda c: c.lib.tslam_esdf_slice(c.h, 0, 1, 0.2, 1.0, 1e-4, c.P), ESTATE, VOL),
    ("stereo_depth_init", lambda c: c.lib.tslam_stereo_depth_init(c.h, c.i32(0, 10, 1, 0), 1), ESTATE,
     "dense stereo depth needs a stereo handle (this one is RGB-D)"),
]

# -- the same handle inside a batch, still without a volume: the volume is asked for first ----------------
NO_VOLUME_IN_BATCH = [
    ("integrate", _integrate(INTEGRATE[0]), ESTATE, VOL),
    ("integrate_rig", _rig(), ESTATE, "no rig set (tslam_set_rig)"),
    ("follow", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow()), ESTATE, VOL),
    ("shift", lambda c: c.lib.tslam_tsdf_shift(c.h, c.i32(1, 0, 0), None), ESTATE, VOL),
    ("render_init", _render_init(), ESTATE, VOL),
    ("render", _render(), ESTATE, VOL),
    ("align_init", _align_init(), ESTATE, VOL),
    ("align", _align(), ESTATE, VOL),
    ("integrate_aligned", _aligned(), ESTATE, VOL),
    ("stereo_depth_init", lambda c: c.lib.tslam_stereo_depth_init(c.h, c.i32(0, 10, 1, 0), 1), ESTATE,
     "dense stereo depth needs a stereo handle (this one is RGB-D)"),
]

# -- an 8 x 8 x 8 volume, no render or align state; the last batch is one frame -------------------
VOLUME = [
    ("color after init", lambda c: c.lib.tslam_tsdf_color(c.h, 1), ESTATE, "tslam_tsdf_color before tslam_tsdf_init"),
    ("integrate_rig", _rig(), ESTATE, "no rig set (tslam_set_rig)"),
    ("integrate_rgbd", _rgbd(), ESTATE, NOCOL),
    ("integrate_rgbd, null colour", _rgbd(color=False), EINVAL, "null colour images"),
    ("follow, step 0", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow(step=0)), EINVAL, "need 1 <= step <= margin < 2^30"),
    ("follow, margin below step", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow(margin=1, step=2)), EINVAL, "need 1 <= step <= margin < 2^30"),
    ("follow, margin 2^30", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow(margin=1 << 30)), EINVAL, "need 1 <= step <= margin < 2^30"),
    ("follow, anchor 2^30", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow(anchor=(0, 1 << 30, 0))), EINVAL, "|anchor| must be below 2^30"),
    ("shift, null delta", lambda c: c.lib.tslam_tsdf_shift(c.h, None, None), EINVAL, "bad argument"),
    ("shift, delta -2^30", lambda c: c.lib.tslam_tsdf_shift(c.h, c.i32(0, 0, -(1 << 30)), None), EINVAL, "|delta| must be below 2^30"),
    ("render_init, null params", lambda c: c.lib.tslam_tsdf_render_init(c.h, None, 1), EINVAL, "bad argument"),
    ("render_init, width 0", _render_init(width=0), EINVAL, "width and height must be 1..16384"),
    ("render_init, height 16385", _render_init(height=16385), EINVAL, "width and height must be 1..16384"),
    ("render_init, cx NaN", _render_init(cx=float("nan")), EINVAL, "camera and render parameters must be finite"),
    ("render_init, max_depth inf", _render_init(max_depth=float("inf")), EINVAL, "camera and render parameters must be finite"),
    ("render_init, fx 0", _render_init(fx=0.0), EINVAL, "fx and fy must be > 0"),
    ("render_init, min_weight < 0", _render_init(min_weight=-1.0), EINVAL, "min_weight must be >= 0"),
    ("render_init, min_depth < 0", _render_init(min_depth=-1.0), EINVAL, "need 0 <= min_depth < max_depth"),
    ("render_init, max_depth = min_depth", _render_init(min_depth=1.0, max_depth=1.0), EINVAL, "need 0 <= min_depth < max_depth"),
    ("render_init, step_scale 0", _render_init(step_scale=0.0), EINVAL, "step_scale must be in (0, 1]"),
    ("render_init, step_scale 2", _render_init(step_scale=2.0), EINVAL, "step_scale must be in (0, 1]"),
    ("render_init, outputs 0", _render_init(outputs=0), EINVAL, "outputs must be a bit mask 1..15 and reserved 0"),
    ("render_init, outputs 16", _render_init(outputs=16), EINVAL, "outputs must be a bit mask 1..15 and reserved 0"),
    ("render_init, reserved 1", _render_init(reserved=1), EINVAL, "outputs must be a bit mask 1..15 and reserved 0"),
    ("render_init, max_views 0", _render_init(max_views=0), EINVAL, "max_views must be 1..256"),
    ("render_init, max_views 257", _render_init(max_views=257), EINVAL, "max_views must be 1..256"),
    ("render", _render(), ESTATE, RND),
    ("render, and a bad pair", _render(pair=-1), EINVAL, "bad handle or pair"),
    ("render_buffers", lambda c: c.lib.tslam_tsdf_render_buffers(c.h, None, None, None, None, None), ESTATE, RND),
    ("render_read", lambda c: c.lib.tslam_tsdf_render_read(c.h, 0, None, None, None, None), ESTATE, RND),
    ("align_init, pair -1", _align_init(pair=-1), EINVAL, "bad pair"),
    ("align_init, pair 1", _align_init(pair=1), EINVAL, "bad pair"),
    ("align_init, iterations 0", _align_init(iterations=0), EINVAL, "iterations must be 1..64"),
    ("align_init, iterations 65", _align_init(iterations=65), EINVAL, "iterations must be 1..64"),
    ("align_init, min_inliers 5", _align_init(min_inliers=5), EINVAL, "min_inliers must be >= 6"),
    ("align_init, max_frames 0", _align_init(max_frames=0), EINVAL, "max_frames must be 1..256"),
    ("align_init, max_frames 257", _align_init(max_frames=257), EINVAL, "max_frames must be 1..256"),
    ("align_init, max_translation NaN", _align_init(max_translation=float("nan")), EINVAL, "align parameters must be finite"),
    ("align_init, max_depth inf", _align_init(max_depth=float("inf")), EINVAL, "align parameters must be finite"),
    ("align_init, max_distance 0", _align_init(max_distance=0.0), EINVAL, "max_distance, max_depth and max_translation must be > 0"),
    ("align_init, min_weight < 0", _align_init(min_weight=-1.0), EINVAL, "min_weight must be >= 0"),
    ("align_init, step_scale 0", _align_init(step_scale=0.0), EINVAL, "step_scale must be in (0, 1]"),
    ("align_init, max_rotation 4", _align_init(max_rotation=4.0), EINVAL, "max_rotation must be in (0, pi]"),
    ("align_init, eps_translation < 0", _align_init(eps_translation=-1.0), EINVAL, "eps_translation and eps_rotation must be >= 0"),
    ("align_init, min_pivot 1", _align_init(min_pivot=1.0), EINVAL, "min_pivot must be in (0, 1)"),
    ("align_init, reserved", _align_init(reserved=(0, 0, 1, 0)), EINVAL, "reserved must be 0"),
    ("align", _align(), ESTATE, ALN),
    ("align, and null depth", _align(depth=False), ESTATE, ALN),
    ("align_read", lambda c: c.lib.tslam_tsdf_align_read(c.h, 1, c.P, None, None, None), ESTATE, ALN),
    ("align_buffers", lambda c: c.lib.tslam_tsdf_align_buffers(c.h, None, None), ESTATE, ALN),
    ("integrate_aligned", _aligned(), ESTATE, ALN),
    ("integrate_aligned, and colour without the layer", _aligned(color=True), ESTATE, ALN),
    ("write, null tsdf", lambda c: c.lib.tslam_tsdf_write(c.h, None, c.P), EINVAL, "null volume"),
    ("write, null weight", lambda c: c.lib.tslam_tsdf_write(c.h, c.P, None), EINVAL, "null volume"),
    ("read_color", lambda c: c.lib.tslam_tsdf_read_color(c.h, c.P, c.P), ESTATE, "no colour layer"),
    ("write_color", lambda c: c.lib.tslam_tsdf_write_color(c.h, c.P, c.P), ESTATE, "no colour layer"),
    ("mesh_extract, min_weight < 0", lambda c: c.lib.tslam_mesh_extract(c.h, -1.0, None, None), EINVAL, "min_weight must be >= 0"),
    ("mesh_extract, min_weight NaN", lambda c: c.lib.tslam_mesh_extract(c.h, float("nan"), None, None), EINVAL, "min_weight must be >= 0"),
    ("mesh_read, max_tris < 0", lambda c: c.lib.tslam_mesh_read(c.h, c.P, -1), EINVAL, "bad buffer"),
    ("mesh_read, null buffer", lambda c: c.lib.tslam_mesh_read(c.h, None, 1), EINVAL, "bad buffer"),
    ("mesh_read_colors", lambda c: c.lib.tslam_mesh_read_colors(c.h, c.P, 1), ESTATE, "no colour layer mesh"),
    ("esdf_compute, max_dist 0", lambda c: c.lib.tslam_esdf_compute(c.h, 0.0, 1.0, 1e-4, None), EINVAL,
     "max_dist must be > 0, site_vox and min_weight >= 0"),
    ("esdf_compute, site_vox < 0", lambda c: c.lib.tslam_esdf_compute(c.h, 0.2, -1.0, 1e-4, None), EINVAL,
     "max_dist must be > 0, site_vox and min_weight >= 0"),
    ("esdf_compute, too far", lambda c: c.lib.tslam_esdf_compute(c.h, 0.05 * 2050, 1.0, 1e-4, None), EINVAL,
     "max_dist / voxel_size must be at most 2048 voxels"),
    ("esdf_read", lambda c: c.lib.tslam_esdf_read(c.h, c.P), ESTATE, "no ESDF (tslam_esdf_compute)"),
    ("esdf_slice, null buffer", lambda c: c.lib.tslam_esdf_slice(c.h, 0, 1, 0.2, 1.0, 1e-4, None), EINVAL,
     "need 0 <= y0 < y1 <= ny and a buffer"),
    ("esdf_slice, y1 = y0", lambda c: c.lib.tslam_esdf_slice(c.h, 2, 2, 0.2, 1.0, 1e-4, c.P), EINVAL, "need 0 <= y0 < y1 <= ny and a buffer"),
    ("esdf_slice, y1 > ny", lambda c: c.lib.tslam_esdf_slice(c.h, 0, 9, 0.2, 1.0, 1e-4, c.P), EINVAL, "need 0 <= y0 < y1 <= ny and a buffer"),
    ("esdf_slice, max_dist 0", lambda c: c.lib.tslam_esdf_slice(c.h, 0, 1, 0.0, 1.0, 1e-4, c.P), EINVAL,
     "max_dist must be > 0, site_vox and min_weight >= 0"),
    ("esdf_slice, too far", lambda c: c.lib.tslam_esdf_slice(c.h, 0, 1, 0.05 * 2050, 1.0, 1e-4, c.P), EINVAL,
     "max_dist / voxel_size must be at most 2048 voxels"),
]
for _fn in INTEGRATE:   # tslam_tsdf_integrate and _rect share every refusal
    VOLUME += [
        (f"{_fn}, pair -1", _integrate(_fn, pair=-1), EINVAL, "bad handle or pair"),
        (f"{_fn}, pair 1", _integrate(_fn, pair=1), EINVAL, "bad handle or pair"),
        (f"{_fn}, null depth", _integrate(_fn, depth=False), EINVAL, DEPTH),
        (f"{_fn}, n_frames < 0", _integrate(_fn, n=-1), EINVAL, DEPTH),
        (f"{_fn}, short stride", _integrate(_fn, n=2, stride=S - 1), EINVAL, DEPTH),
        (f"{_fn}, device poses past the batch", _integrate(_fn, host=False, n=2), EINVAL, LAST),
        (f"{_fn}, device poses after the batch", _integrate(_fn, host=False, first=1), EINVAL, LAST),
        (f"{_fn}, device poses before the batch", _integrate(_fn, host=False, first=-1), EINVAL, LAST),
    ]

# -- the same, inside a batch ------------------------------------------------------------------------------
VOLUME_IN_BATCH = [
    ("integrate", _integrate(INTEGRATE[0]), ESTATE, "tslam_tsdf_integrate inside a batch"),
    ("integrate_rect", _integrate(INTEGRATE[1]), ESTATE, "tslam_tsdf_integrate inside a batch"),
    ("integrate, and null depth", _integrate(INTEGRATE[0], depth=False), EINVAL, DEPTH),
    ("integrate, and device poses out of range", _integrate(INTEGRATE[0], host=False, first=-1), ESTATE,
     "tslam_tsdf_integrate inside a batch"),
    ("follow", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow()), ESTATE, "tslam_tsdf_follow inside a batch"),
    ("follow off", lambda c: c.lib.tslam_tsdf_follow(c.h, None), ESTATE, "tslam_tsdf_follow inside a batch"),
    ("follow, and step 0", lambda c: c.lib.tslam_tsdf_follow(c.h, c.follow(step=0)), ESTATE, "tslam_tsdf_follow inside a batch"),
    ("shift", lambda c: c.lib.tslam_tsdf_shift(c.h, c.i32(1, 0, 0), None), ESTATE, "tslam_tsdf_shift inside a batch"),
    ("shift, and delta 2^30", lambda c: c.lib.tslam_tsdf_shift(c.h, c.i32(1 << 30, 0, 0), None), ESTATE, "tslam_tsdf_shift inside a batch"),
    ("render_init", _render_init(), ESTATE, "tslam_tsdf_render_init inside a batch"),
    ("render_init, and width 0", _render_init(width=0), ESTATE, "tslam_tsdf_render_init inside a batch"),
    ("render, and no render state", _render(), ESTATE, RND),
    ("align_init", _align_init(), ESTATE, "tslam_tsdf_align_init inside a batch"),
    ("align_init off", _align_init(prm=False), ESTATE, "tslam_tsdf_align_init inside a batch"),
    ("align_init, and a bad pair", _align_init(pair=1), ESTATE, "tslam_tsdf_align_init inside a batch"),
    ("align, and no align state", _align(), ESTATE, ALN),
    ("integrate_aligned, and no align state", _aligned(), ESTATE, ALN),
]

# -- render and align states made (2 views of 8 x 8 with depth_m and normals; 2 frames) --------------------
STATES = [
    ("render, n_views < 0", _render(n=-1), EINVAL, "n_views must be 0..max_views"),
    ("render, n_views 3", _render(n=3), EINVAL, "n_views must be 0..max_views"),
    ("render, device poses past the batch", _render(host=False, n=2), EINVAL, LAST),
    ("render, device poses after the batch", _render(host=False, first=1), EINVAL, LAST),
    ("render, device poses before the batch", _render(host=False, first=-1), EINVAL, LAST),
    ("render, no views before the batch", _render(host=False, n=0, first=-1), EINVAL, LAST),
    ("render_read, view -1", lambda c: c.lib.tslam_tsdf_render_read(c.h, -1, c.P, None, None, None), EINVAL, "view out of range"),
    ("render_read, view 2", lambda c: c.lib.tslam_tsdf_render_read(c.h, 2, c.P, None, None, None), EINVAL, "view out of range"),
    ("render_read, depth_mm not asked for", lambda c: c.lib.tslam_tsdf_render_read(c.h, 0, None, c.P, None, None), EINVAL,
     "an output that tslam_tsdf_render_init was not asked for"),
    ("render_read, colour not asked for", lambda c: c.lib.tslam_tsdf_render_read(c.h, 0, c.P, None, None, c.P), EINVAL,
     "an output that tslam_tsdf_render_init was not asked for"),
    ("align, null depth", _align(depth=False), EINVAL, DEPTH),
    ("align, short stride", _align(n=2, stride=S - 1), EINVAL, DEPTH),
    ("align, n_frames < 0", _align(n=-1), EINVAL, "n_frames must be 0..max_frames"),
    ("align, n_frames 3", _align(n=3), EINVAL, "n_frames must be 0..max_frames"),
    ("align, device poses past the batch", _align(host=False, n=2), EINVAL, LAST),
    ("align, device poses after the batch", _align(host=False, first=1), EINVAL, LAST),
    ("align, device poses before the batch", _align(host=False, first=-1), EINVAL, LAST),
    ("align_read, max_frames < 0", lambda c: c.lib.tslam_tsdf_align_read(c.h, -1, c.P, None, None, None), EINVAL, "max_frames must be >= 0"),
    ("integrate_aligned, colour without the layer", _aligned(color=True), ESTATE, NOCOL),
    ("integrate_aligned, null depth", _aligned(depth=False), EINVAL, DEPTH),
    ("integrate_aligned, short stride", _aligned(n=2, stride=S - 1), EINVAL, DEPTH),
    ("integrate_aligned, n_frames < 0", _aligned(n=-1), EINVAL, "n_frames must be 0 .. the frames of the last tslam_tsdf_align"),
    ("integrate_aligned, before any tslam_tsdf_align", _aligned(), EINVAL, "n_frames must be 0 .. the frames of the last tslam_tsdf_align"),
]

STATES_IN_BATCH = [
    ("render", _render(), ESTATE, "tslam_tsdf_render inside a batch"),
    ("render, and n_views 3", _render(n=3), ESTATE, "tslam_tsdf_render inside a batch"),
    ("render, and a bad pair", _render(pair=1), EINVAL, "bad handle or pair"),
    ("align", _align(), ESTATE, "tslam_tsdf_align inside a batch"),
    ("align, and null depth", _align(depth=False), ESTATE, "tslam_tsdf_align inside a batch"),
    ("integrate_aligned", _aligned(), ESTATE, "tslam_tsdf_integrate_aligned inside a batch"),
    ("integrate_aligned, and colour without the layer", _aligned(color=True), ESTATE, "tslam_tsdf_integrate_aligned inside a batch"),
    ("integrate_aligned, and null depth", _aligned(depth=False), ESTATE, "tslam_tsdf_integrate_aligned inside a batch"),
]

# -- the states kept, the volume made again with one dimension of 1 -----------------------------------------
FLAT_VOLUME = [
    ("render_init", _render_init(), EINVAL, "rendering needs volume dims >= 2"),
    ("render", _render(), EINVAL, "rendering needs volume dims >= 2"),
    ("render, and n_views 3", _render(n=3), EINVAL, "rendering needs volume dims >= 2"),
    ("align_init", _align_init(), EINVAL, "alignment needs volume dims >= 2"),
    ("align_init, and a bad pair", _align_init(pair=1), EINVAL, "bad pair"),
    ("align_init, and iterations 0", _align_init(iterations=0), EINVAL, "alignment needs volume dims >= 2"),
    ("align: the state went with its volume", _align(), ESTATE, ALN),
]

# -- a handle with the colour layer ----------------------------------------------------------------------------
COLOR = [
    ("color off after init", lambda c: c.lib.tslam_tsdf_color(c.h, 0), ESTATE, "tslam_tsdf_color before tslam_tsdf_init"),
    ("integrate_rgbd, null colour", _rgbd(color=False), EINVAL, "null colour images"),
    ("integrate_rgbd, pair 1", _rgbd(pair=1), EINVAL, "bad handle or pair"),
    ("integrate_rgbd, null depth", _rgbd(depth=False), EINVAL, DEPTH),
    ("integrate_rgbd, device poses without a batch", _rgbd(host=False), EINVAL, LAST),
    ("write_color, null rgb", lambda c: c.lib.tslam_tsdf_write_color(c.h, None, c.P), EINVAL, "null colour volume"),
    ("write_color, null weight", lambda c: c.lib.tslam_tsdf_write_color(c.h, c.P, None), EINVAL, "null colour volume"),
    ("mesh_read_colors before a mesh", lambda c: c.lib.tslam_mesh_read_colors(c.h, c.P, 1), ESTATE, "no colour layer mesh"),
]
COLOR_IN_BATCH = [
    ("integrate_rgbd", _rgbd(), ESTATE, "tslam_tsdf_integrate inside a batch"),
    ("integrate_rgbd, and null depth", _rgbd(depth=False), EINVAL, DEPTH),
]
COLOR_MESH = [   # after a mesh of the empty volume and its ESDF
    ("mesh_read_colors, max_tris < 0", lambda c: c.lib.tslam_mesh_read_colors(c.h, c.P, -1), EINVAL, "bad buffer"),
    ("mesh_read_colors, null buffer", lambda c: c.lib.tslam_mesh_read_colors(c.h, None, 1), EINVAL, "bad buffer"),
    ("esdf_read, null buffer", lambda c: c.lib.tslam_esdf_read(c.h, None), EINVAL, "null buffer"),
]

# -- two RGB-D pairs as a rig ----------------------------------------------------------------------------------
RIG_NO_VOLUME = [
    ("integrate_rig", _rig(), ESTATE, VOL),
    ("integrate_rig, and n_cams 0", _rig(n_cams=0), ESTATE, VOL),
]
RIG = [
    ("null cameras", _rig(cams=()), EINVAL, "bad argument"),
    ("n_cams 0", _rig(n_cams=0), EINVAL, "n_cams must be 1..8"),
    ("n_cams 9", _rig(n_cams=9), EINVAL, "n_cams must be 1..8"),
    ("n_frames < 0", _rig(n=-1), EINVAL, "n_frames must be >= 0"),
    ("pair -1", _rig(cams=((-1, 1, 0, S),)), EINVAL, "pairs must be strictly ascending and in range"),
    ("pair 2", _rig(cams=((2, 1, 0, S),)), EINVAL, "pairs must be strictly ascending and in range"),
    ("pairs not ascending", _rig(cams=((1, 1, 0, S), (0, 1, 0, S))), EINVAL, "pairs must be strictly ascending and in range"),
    ("a pair twice", _rig(cams=((0, 1, 0, S), (0, 1, 0, S))), EINVAL, "pairs must be strictly ascending and in range"),
    ("null depth", _rig(cams=((0, 1, 0, S), (1, 0, 0, S))), EINVAL, DEPTH),
    ("short stride", _rig(cams=((0, 1, 0, S), (1, 1, 0, S - 1)), n=2), EINVAL, DEPTH),
    ("colour for one camera", _rig(cams=((0, 1, 0, S), (1, 1, 1, S))), EINVAL, "colour for all cameras or for none"),
    ("colour without the layer", _rig(cams=((0, 1, 1, S), (1, 1, 1, S))), EINVAL, "colour without the colour layer (tslam_tsdf_color)"),
    ("device poses without a batch", _rig(host=False), EINVAL, LAST),
    ("device poses before the batch", _rig(host=False, n=0, first=-1), EINVAL, LAST),
]
RIG_IN_BATCH = [
    ("integrate_rig", _rig(), ESTATE, "tslam_tsdf_integrate_rig inside a batch"),
    ("integrate_rig, and n_cams 0", _rig(n_cams=0), ESTATE, "tslam_tsdf_integrate_rig inside a batch"),
]

# -- a stereo handle --------------------------------------------------------------------------------------------
SW, SH = 320, 240


def _sd_init(prm=(0, 10, 1, 0), max_frames=2):
    return lambda c: c.lib.tslam_stereo_depth_init(c.h, c.i32(*prm) if prm else None, max_frames)


def _apply(disp=True, w=16, hh=16, fxb=1.0, n=1):
    return lambda c: c.lib.tslam_stereo_depth_filter_apply(c.h, c.D if disp else None, w, hh, fxb, n, None)


def _slots(pair=0, first=0, n=1, slot=0):
    return lambda c: c.lib.tslam_stereo_depth_slots(c.h, pair, c.g0() + first, n, slot, None)


def _images(left=True, right=True, stride=SW * SH, w=16, hh=16, fxb=1.0, n=1):
    return lambda c: c.lib.tslam_stereo_depth_images(c.h, c.D if left else None, c.D if right else None, stride, w, hh, fxb, n, None)


STEREO_FRESH = [
    ("init, null params", _sd_init(prm=None), EINVAL, "bad argument"),
    ("init, n_disp 3", _sd_init(prm=(3, 10, 1, 0)), EINVAL, "n_disp must be 4..256 (0 = max_disparity)"),
    ("init, n_disp 257", _sd_init(prm=(257, 10, 1, 0)), EINVAL, "n_disp must be 4..256 (0 = max_disparity)"),
    ("init, uniqueness 100", _sd_init(prm=(0, 100, 1, 0)), EINVAL, "uniqueness must be 0..99"),
    ("init, lr_tol < 0", _sd_init(prm=(0, 10, -1, 0)), EINVAL, "lr_tol must be >= 0 and reserved 0"),
    ("init, reserved", _sd_init(prm=(0, 10, 1, 1)), EINVAL, "lr_tol must be >= 0 and reserved 0"),
    ("init, max_frames 0", _sd_init(max_frames=0), EINVAL, "max_frames must be 1..65535"),
    ("init, max_frames 65536", _sd_init(max_frames=65536), EINVAL, "max_frames must be 1..65535"),
    ("sgm", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm()), ESTATE, SD),
    ("filter", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt()), ESTATE, SD),
    ("filter_apply", _apply(), ESTATE, SD),
    ("stereo_depth", lambda c: c.lib.tslam_stereo_depth(c.h, 0, 0, 1, None), ESTATE, SD),
    ("slots", _slots(), ESTATE, SD),
    ("slots, and a bad pair", _slots(pair=1), EINVAL, "bad handle or pair"),
    ("images", _images(), ESTATE, SD),
    ("buffers", lambda c: c.lib.tslam_stereo_depth_buffers(c.h, None, None, None), ESTATE, SD),
    ("read", lambda c: c.lib.tslam_stereo_depth_read(c.h, 0, c.P, c.P), ESTATE, SD),
]
STEREO_FRESH_IN_BATCH = [
    ("init", _sd_init(), ESTATE, "tslam_stereo_depth_init inside a batch"),
    ("init, and n_disp 3", _sd_init(prm=(3, 10, 1, 0)), ESTATE, "tslam_stereo_depth_init inside a batch"),
    ("sgm, and no buffers", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm()), ESTATE, SD),
    ("slots, and no buffers", _slots(), ESTATE, SD),
]
STEREO = [   # 2 slots, the filters off
    ("sgm, null params", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, None), EINVAL, "bad argument"),
    ("sgm, reserved", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(reserved=(0, 1, 0))), EINVAL, "reserved must be 0"),
    ("sgm off, reserved", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(enable=0, reserved=(0, 0, 1))), EINVAL, "reserved must be 0"),
    ("sgm, p1 < 0", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(p1=-1)), EINVAL, "penalties must satisfy 0 <= p1 <= p2 <= 2400"),
    ("sgm, p1 > p2", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(p1=200, p2=100)), EINVAL, "penalties must satisfy 0 <= p1 <= p2 <= 2400"),
    ("sgm, p2 2401", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(p2=2401)), EINVAL, "penalties must satisfy 0 <= p1 <= p2 <= 2400"),
    ("sgm, paths 0", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(paths=0)), EINVAL, "paths must be a bit mask 1..15"),
    ("sgm, paths 16", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(paths=16)), EINVAL, "paths must be a bit mask 1..15"),
    ("sgm, chunk_frames < 0", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(chunk=-1)), EINVAL, "chunk_frames must be >= 0"),
    ("filter, null params", lambda c: c.lib.tslam_stereo_depth_filter(c.h, None), EINVAL, "bad argument"),
    ("filter, reserved", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt(reserved=(0, 0, 0, 1))), EINVAL, "reserved must be 0"),
    ("filter, median 4", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt(median=4)), EINVAL, "median must be 0, 3, 5 or 7"),
    ("filter, speckle_size 65536", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt(size=65536)), EINVAL, "speckle_size must be 0..65535"),
    ("filter, speckle_range 8192", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt(rng=8192)), EINVAL, "speckle_range must be 0..8191"),
    ("filter, nothing to do", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt(median=0, size=0)), EINVAL,
     "enable needs a median or a speckle size"),
    ("filter_apply, null plane", _apply(disp=False), EINVAL, "bad argument"),
    ("filter_apply, filters off", _apply(), ESTATE, "the filters are off (tslam_stereo_depth_filter)"),
    ("filter_apply, filters off and n_frames 3", _apply(n=3), ESTATE, "the filters are off (tslam_stereo_depth_filter)"),
    ("slots, pair 1", _slots(pair=1), EINVAL, "bad handle or pair"),
    ("slots, n_frames < 0", _slots(n=-1), EINVAL, "n_frames must be 0..max_frames"),
    ("slots, n_frames 3", _slots(n=3), EINVAL, "n_frames must be 0..max_frames"),
    ("slots, first_slot < 0", _slots(slot=-1), EINVAL, "first_slot + n_frames must be within max_frames"),
    ("slots, past the last slot", _slots(slot=1, n=2), EINVAL, "first_slot + n_frames must be within max_frames"),
    ("slots, after the batch", _slots(first=1), EINVAL, "frames must belong to the last batch"),
    ("slots, before the batch", _slots(first=-1, n=0), EINVAL, "frames must belong to the last batch"),
    ("stereo_depth, after the batch", lambda c: c.lib.tslam_stereo_depth(c.h, 0, c.g0() + 1, 1, None), EINVAL, "frames must belong to the last batch"),
    ("stereo_depth, n_frames 3", lambda c: c.lib.tslam_stereo_depth(c.h, 0, c.g0(), 3, None), EINVAL, "n_frames must be 0..max_frames"),
    ("images, null left", _images(left=False), EINVAL, "bad argument"),
    ("images, null right", _images(right=False), EINVAL, "bad argument"),
    ("images, n_frames < 0", _images(n=-1), EINVAL, "n_frames must be 0..max_frames"),
    ("images, n_frames 3", _images(n=3), EINVAL, "n_frames must be 0..max_frames"),
    ("images, width 15", _images(w=15), EINVAL, "width / height must be 16 .. the handle's size"),
    ("images, height above the handle's", _images(hh=SH + 1), EINVAL, "width / height must be 16 .. the handle's size"),
    ("images, short stride", _images(n=2, stride=255), EINVAL, "frame_stride below one image"),
    ("images, fxb 0", _images(fxb=0.0), EINVAL, "fxb must be > 0"),
    ("images, fxb NaN", _images(fxb=float("nan")), EINVAL, "fxb must be > 0"),
    ("read, slot -1", lambda c: c.lib.tslam_stereo_depth_read(c.h, -1, c.P, c.P), EINVAL, "slot out of range"),
    ("read, slot 2", lambda c: c.lib.tslam_stereo_depth_read(c.h, 2, c.P, c.P), EINVAL, "slot out of range"),
]
STEREO_FILTERS_ON = [   # the median alone: no planes of its own
    ("filter_apply, n_frames < 0", _apply(n=-1), EINVAL, "n_frames must be 0..max_frames"),
    ("filter_apply, n_frames 3", _apply(n=3), EINVAL, "n_frames must be 0..max_frames"),
    ("filter_apply, width 15", _apply(w=15), EINVAL, "width / height must be 16 .. the handle's size"),
    ("filter_apply, width above the handle's", _apply(w=SW + 1), EINVAL, "width / height must be 16 .. the handle's size"),
    ("filter_apply, fxb 0", _apply(fxb=0.0), EINVAL, "fxb must be > 0"),
]
STEREO_IN_BATCH = [
    ("sgm", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm()), ESTATE, "tslam_stereo_depth_sgm inside a batch"),
    ("sgm, and reserved", lambda c: c.lib.tslam_stereo_depth_sgm(c.h, c.sgm(reserved=(1, 0, 0))), ESTATE, "tslam_stereo_depth_sgm inside a batch"),
    ("filter", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt()), ESTATE, "tslam_stereo_depth_filter inside a batch"),
    ("filter, and median 4", lambda c: c.lib.tslam_stereo_depth_filter(c.h, c.flt(median=4)), ESTATE, "tslam_stereo_depth_filter inside a batch"),
    ("filter_apply", _apply(), ESTATE, "tslam_stereo_depth_filter_apply inside a batch"),
    ("filter_apply, and n_frames 3", _apply(n=3), ESTATE, "tslam_stereo_depth_filter_apply inside a batch"),
    ("stereo_depth", lambda c: c.lib.tslam_stereo_depth(c.h, 0, 0, 1, None), ESTATE, "tslam_stereo_depth inside a batch"),
    ("slots", _slots(), ESTATE, "tslam_stereo_depth inside a batch"),
    ("slots, and n_frames 3", _slots(n=3), ESTATE, "tslam_stereo_depth inside a batch"),
    ("images", _images(), ESTATE, "tslam_stereo_depth_images inside a batch"),
    ("images, and width 15", _images(w=15), ESTATE, "tslam_stereo_depth_images inside a batch"),
]


def _batch(c, table):
    """The table between tslam_begin_batch and tslam_end_batch (nothing is launched)."""
    c.hd.begin_batch(c.D, 1)
    try:
        _check(c, table)
    finally:
        c.hd.end_batch()


def test_rgbd_handle():
    _, rec = _records(4)
    h = _handle()
    try:
        import torch

        c = Ctx(h)
        dev = torch.from_numpy(rec[:1].copy()).cuda()
        h.submit(dev.data_ptr(), 1, _stream())            # a last batch exists from here on
        _check(c, NULL_HANDLE)
        _check(c, NO_VOLUME)
        _batch(c, NO_VOLUME_IN_BATCH)
        c.volume()
        _check(c, VOLUME)
        _batch(c, VOLUME_IN_BATCH)
        assert c.lib.tslam_tsdf_render_init(c.h, c.render(), 2) == 0
        assert c.lib.tslam_tsdf_align_init(c.h, 0, 1, c.align(), 2) == 0
        _check(c, STATES)
        _batch(c, STATES_IN_BATCH)
        c.volume((8, 1, 8))
        _check(c, FLAT_VOLUME)
        t, w = np.zeros((8, 1, 8), np.float32), np.zeros((8, 1, 8), np.float32)
        assert c.lib.tslam_tsdf_read(c.h, t.ctypes.data, w.ctypes.data) == 0
        assert not t.any() and not w.any()               # no refused call wrote to the volume
    finally:
        h.close()


def test_colour_layer():
    h = _handle()
    try:
        c = Ctx(h)
        assert c.lib.tslam_tsdf_color(c.h, 1) == 0
        c.volume()
        _check(c, COLOR)
        _batch(c, COLOR_IN_BATCH)
        assert c.lib.tslam_mesh_extract(c.h, 1e-4, None, None) == 0
        assert c.lib.tslam_esdf_compute(c.h, 0.2, 1.0, 1e-4, None) == 0
        _check(c, COLOR_MESH)
    finally:
        h.close()


def test_rig():
    from thor_slam_amd._lib import Handle

    rect, _ = _records(4)
    h = Handle([rect, rect], HipSlamConfig(rgbd=True, n_features=1000, n_levels=3), max_batch=1)
    try:
        c = Ctx(h)
        h.set_rig([np.eye(4), np.eye(4)])
        _check(c, RIG_NO_VOLUME)
        c.volume()
        _check(c, RIG)
        _batch(c, RIG_IN_BATCH)
    finally:
        h.close()


def test_stereo_handle():
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.synthetic import SyntheticStereoSource

    cams = extract_cameras(CameraRig([SyntheticStereoSource(width=SW, height=SH)]).calibration, 2)
    (li, ri), = stereo_pairs(cams)
    h = Handle([stereo_rectify(cams[li], cams[ri])], HipSlamConfig(n_features=256, n_levels=1, max_disparity=48), max_batch=1)
    try:
        c = Ctx(h)
        _check(c, STEREO_FRESH)
        _batch(c, STEREO_FRESH_IN_BATCH)
        assert _sd_init()(c) == 0
        _check(c, STEREO)
        assert c.lib.tslam_stereo_depth_filter(c.h, c.flt(median=3, size=0)) == 0
        _check(c, STEREO_FILTERS_ON)
        _batch(c, STEREO_IN_BATCH)
    finally:
        h.close()
