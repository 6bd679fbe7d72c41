"""The dense map's dispatch with ``dense_dynamic``, pinned call by call with the recording stand-in of
tests/test_dense_dispatch_cpu.py: a batch's depth goes through ``tsdf_dynamic`` and the filtered
copy, in the mask state's slots, through ``tsdf_integrate_rect`` with the same frames, for records,
stereo runs, and stereo at interval 2.  No device is needed."""

from __future__ import annotations

import test_dense_dispatch_cpu as D
from thor_slam_amd.params import HipSlamConfig
from thor_slam_amd.slam._dense import DenseMap

N, W, H, STREAM, PTR = D.N, D.W, D.H, D.STREAM, D.RECORDS_PTR
HW = W * H
DYN_DEPTH, DYN_MASK, DYN_STATS = 0x60000000, 0x61000000, 0x62000000
SD_DEPTH, SD_BYTES = 0x20000000, 2 * HW          # what the stand-in's stereo_depth_buffers returns


class _Recorder(D._Recorder):
    def tsdf_dynamic_buffers(self):
        self._note("tsdf_dynamic_buffers", (), {})
        return {"depth": DYN_DEPTH, "mask": DYN_MASK, "stats": DYN_STATS}, {"depth": 2 * HW, "mask": HW}


def _run(g0=4, **kw):
    cfg = HipSlamConfig(**kw, dense_dynamic=True, batch_size=N)
    cfg.validate()
    h = _Recorder(g0 + N)
    dm = DenseMap(cfg, h, [D.SimpleNamespace(width=W, height=H)], 2, ())
    dm.integrate(PTR, N, STREAM, stamps=D.STAMPS)
    return h.calls, dm


def _pair(depth, stride, n, g):
    """The two calls of n frames from frame g, and the buffers looked up between them."""
    return [["tsdf_dynamic", [depth, stride, n], {"first_frame": g, "stream": STREAM}],
            ["tsdf_dynamic_buffers", [], {}],
            ["tsdf_integrate_rect", [DYN_DEPTH, 2 * HW, n], {"first_frame": g, "pair": 0, "stream": STREAM}]]


def test_records():
    calls, dm = _run(**D.RGBD)
    assert calls == _pair(PTR + 3 * HW, 5 * HW * 2, N, 4)
    assert dm.dyn_last == (N - 1, D.STAMPS[-1]) and dm.sd_last == {}


def test_stereo():
    calls, dm = _run(**D.STEREO)
    assert calls == [["stereo_depth_buffers", [], {}], ["stereo_depth", [4, N], {"pair": 0, "stream": STREAM}]] \
        + _pair(SD_DEPTH, SD_BYTES, N, 4)
    assert dm.dyn_last == (N - 1, D.STAMPS[-1]) and dm.sd_last == {0: (N - 1, D.STAMPS[-1])}


def test_stereo_interval_2():
    calls, dm = _run(**D.STEREO, stereo_depth_interval=2)
    want = [["stereo_depth_buffers", [], {}]]
    for g in (4, 6):
        want += [["stereo_depth", [g, 1], {"pair": 0, "stream": STREAM}]] + _pair(SD_DEPTH, SD_BYTES, 1, g)
    assert calls == want
    assert dm.dyn_last == (0, D.STAMPS[2]) and dm.sd_last == {0: (0, D.STAMPS[2])}


def test_init_handle_sets_the_state_up():
    for kw, rect in ((D.RGBD, False), (D.STEREO, True)):
        cfg = HipSlamConfig(**kw, dense_dynamic=True, batch_size=N, dense_dynamic_open_px=2)
        h = _Recorder(0)
        DenseMap(cfg, h, [D.SimpleNamespace(width=W, height=H)], 1, ()).init_handle()
        got = [c for c in h.calls if c[0] == "tsdf_dynamic_init"]
        assert got == [["tsdf_dynamic_init", [], {"pair": 0, "rect": rect, "max_frames": N, "min_free_weight": 5.0,
                                                  "free_fraction": 0.75, "open_radius": 2, "dilate_radius": 2}]]
        assert [c[0] for c in h.calls].index("tsdf_init") < [c[0] for c in h.calls].index("tsdf_dynamic_init")


def test_option_off_makes_none_of_the_calls():
    h = D._Recorder(4 + N)
    cfg = HipSlamConfig(**D.RGBD, batch_size=N)
    DenseMap(cfg, h, [D.SimpleNamespace(width=W, height=H)], 2, ()).integrate(PTR, N, STREAM, stamps=D.STAMPS)
    assert [c[0] for c in h.calls] == ["tsdf_integrate"]
