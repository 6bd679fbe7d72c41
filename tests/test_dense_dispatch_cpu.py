"""The dense map's dispatch, pinned call by call: which handle calls a batch's depth turns into, with
every argument, and the newest-frame bookkeeping it leaves (stereo depth and registered depth), over
the depth sources (records, stereo runs) and their options.  A recording stand-in takes the
handle's place, so no device is needed.

``tests/golden/dense_dispatch_trace.json`` was recorded by this module (``PYTHONPATH=thor-slam_amd
python tests/test_dense_dispatch_cpu.py``) from ``HipSlamEngine._integrate_depth`` as it stood before the
engine's dense-map code moved into ``slam/_dense.py``; the recorder drives whichever of the two the
checkout has."""

from __future__ import annotations

import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from thor_slam_amd.params import HipSlamConfig

GOLDEN = Path(__file__).parent / "golden" / "dense_dispatch_trace.json"
N, RECORDS_PTR, STREAM = 4, 0x10000000, 0x5EED
W, H = 16, 8
COLOR_SHAPE = (6, 10, 3)   # the colour camera's image, another size than the rectified one

RGBD = dict(rgbd=True, dense_map=True, dense_color=False)
STEREO = dict(dense_map=True, stereo_depth=True)
LOOP = dict(enable_loop_closure=True, dense_loop=True, dense_color=False, loop_kf_interval=2)
# name -> (config, has_color, first frame of the batch); every one with dense_cameras () and (0, 1).
# validate() refuses dense_align and dense_loop with dense_cameras: those four rows are dropped.
CONFIGS = {
    "records": (RGBD, None, 4),
    "records_color": ({**RGBD, "dense_color": True}, None, 4),
    "records_align": ({**RGBD, "dense_align": True}, None, 4),
    "records_loop": ({**RGBD, **LOOP}, None, 4),
    "records_loop_from0": ({**RGBD, **LOOP}, None, 0),
    "stereo": (STEREO, None, 4),
    "stereo_interval2": ({**STEREO, "stereo_depth_interval": 2}, None, 4),
    "stereo_align": ({**STEREO, "dense_align": True}, None, 4),
    "stereo_loop": ({**STEREO, **LOOP}, None, 4),
    "stereo_loop_from0": ({**STEREO, **LOOP}, None, 0),
    "stereo_color": ({**STEREO, "stereo_color": True}, {0: [True, True, False, True]}, 4),
    "stereo_color_device_batch": ({**STEREO, "stereo_color": True}, "none", 4),   # process_batch: has_color=None
}
STAMPS = [0.5, 0.6, 0.7, 0.8]


def _cases():
    out = {}
    for name, (kw, has_color, g0) in CONFIGS.items():
        for dense in ((), (0, 1)):
            cfg = HipSlamConfig(**kw, dense_cameras=dense, batch_size=N)
            try:
                cfg.validate()
            except ValueError:
                continue
            out[f"{name}-{'rig' if dense else 'pair0'}"] = (cfg, dense, has_color, g0)
    return out


class _Ptr:
    """A colour tensor's stand-in."""

    def __init__(self, ptr: int) -> None:
        self._ptr = ptr

    def data_ptr(self) -> int:
        return self._ptr


def _plain(v):
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.ndarray):
        return _plain(v.tolist())
    if isinstance(v, np.generic):
        return v.item()
    return v


class _Recorder:
    """Stands in for the handle: every call is appended to ``calls`` as (name, args, sorted kwargs)."""

    def __init__(self, frames_done: int) -> None:
        self.frames_done = frames_done
        self.calls: list = []

    def _note(self, name, args, kwargs):
        self.calls.append([name, _plain(args), _plain(kwargs)])

    def stereo_depth_buffers(self):
        self._note("stereo_depth_buffers", (), {})
        return 0x20000000, 0x28000000, 2 * W * H

    def depth_register_buffers(self, p):
        self._note("depth_register_buffers", (p,), {})
        base = 0x30000000 + p * 0x1000000
        return ({"depth": base, "bgr": base + 0x100000, "mask": base + 0x200000},
                {"depth": 2 * 60, "bgr": 3 * W * H, "mask": W * H})

    def __getattr__(self, name):
        return lambda *a, **kw: self._note(name, a, kw)


def _run(cfg, dense, has_color, g0) -> dict:
    """One batch of N frames starting at frame g0 through the dense dispatch; the handle calls and
    the bookkeeping it leaves."""
    try:
        from thor_slam_amd.slam._dense import ColorCamera, DenseMap
    except ImportError:   # before the split: the engine itself
        from thor_slam_amd.slam.hip_engine import HipSlamEngine
        DenseMap = None

    h = _Recorder(g0 + N)
    rects = [SimpleNamespace(width=W, height=H)] * 2
    colour = cfg.stereo_color
    dev, zero = _Ptr(0x40000000), {"mask": _Ptr(0x50000000), "bgr": _Ptr(0x51000000)}
    hc = None if has_color == "none" else has_color
    if DenseMap is None:
        eng = HipSlamEngine.__new__(HipSlamEngine)
        eng._config, eng._handle, eng._dense_pairs, eng._rects, eng._pairs = cfg, h, dense, rects[:1], [(0, 1), (2, 3)]
        eng._loop, eng._sd_last, eng._reg_last = None, {}, {}
        eng._color_cams = {0: {"shape": COLOR_SHAPE, "dev": dev}} if colour else {}
        eng._color_zero = zero if colour else None
        eng._integrate_depth(RECORDS_PTR, N, STREAM, stamps=STAMPS, has_color=hc)
        sd, reg = eng._sd_last, eng._reg_last
    else:
        dm = DenseMap(cfg, h, rects[:1], 2, dense)
        if colour:
            dm.color_cams[0] = ColorCamera(COLOR_SHAPE, None, dev, [False] * N)
            dm.color_zero = zero
        dm.integrate(RECORDS_PTR, N, STREAM, stamps=STAMPS, has_color=hc)
        sd, reg = dm.sd_last, dm.reg_last
    return {"calls": h.calls, "sd_last": _plain(sd), "reg_last": _plain(reg)}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_every_case_recorded(golden):
    assert sorted(golden) == sorted(_cases()) and len(golden) == 18


@pytest.mark.parametrize("name", sorted(_cases()))
def test_dispatch_matches_recording(golden, name):
    got = json.loads(json.dumps(_run(*_cases()[name])))
    want = golden[name]
    assert len(got["calls"]) == len(want["calls"])
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {i}"
    assert got["sd_last"] == want["sd_last"] and got["reg_last"] == want["reg_last"]


def test_loop_batch_from_frame_zero_skips_it(golden):
    """Frame 0 initialises and has no pose-graph node: the archive never gets it."""
    rec = golden["records_loop_from0-pair0"]["calls"]
    assert [c[0] for c in rec] == ["tsdf_archive_integrate"] and rec[0][1][2] == N - 1 and rec[0][2]["first_frame"] == 1
    assert all(c[1][0] != 0 for c in golden["stereo_loop_from0-pair0"]["calls"] if c[0] == "stereo_depth")


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps({name: _run(*case) for name, case in _cases().items()}, indent=1, sort_keys=True) + "\n")
    print(f"{len(_cases())} cases -> {GOLDEN}")
