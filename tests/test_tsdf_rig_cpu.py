"""The dense map from every camera of a rig, without a GPU: what the rule (tests/ref_tsdf_rig.py,
thor_slam_amd/dense_rig.py) covers on the bracket RGB-D rig, that its order matters, and
``HipSlamConfig.dense_cameras``."""

from __future__ import annotations

import numpy as np
import pytest

import ref_tsdf_rig as REF
import tsdf_rig_cases as C
from oracle import numpy_rig
from thor_slam_amd import dense_rig
from thor_slam_amd.params import HipSlamConfig

W, H, N = 160, 120, 3


def _observed(vol) -> int:
    return int((vol["weight"] > 0).sum())


def test_reference_coverage():
    """Every camera sees part of the room, all four see at least twice what pair 0 sees, and
    views overlap (a weight above the frame count)."""
    alone = [_observed(C.host_reference(W, H, N, False, (p,))) for p in range(4)]
    allc = C.host_reference(W, H, N, False, (0, 1, 2, 3))
    print("observed voxels per camera", alone, "all four", _observed(allc), "max weight", float(allc["weight"].max()))
    assert min(alone) >= 1000
    assert _observed(allc) >= 2 * alone[0]
    assert allc["weight"].max() > N
    # the colour layer lives inside the truncation band of what was observed
    assert 0 < (allc["color_weight"] > 0).sum() < _observed(allc)


def test_order_discriminates():
    """With max_weight = 2 the frame-major, camera-minor result differs from the camera-major one
    (one launch per camera): the order check on the device means something."""
    a = C.host_reference(W, H, N, False, (0, 1, 2, 3), 2.0, "frame")
    b = C.host_reference(W, H, N, False, (0, 1, 2, 3), 2.0, "camera")
    np.testing.assert_array_equal(a["weight"], b["weight"])     # the same voxels, the same counts
    # far beyond rounding: past the cap the newest observations win, and the two orders end on different ones
    assert (np.abs(a["tsdf"] - b["tsdf"]) > 1e-3).sum() > 100


def test_batch_equals_one_call_per_frame():
    sc = C.rgbd_scene(W, H, N)
    vol = REF.new_volume(C.DIMS)
    for f in range(N):
        one = {k: (v[f:f + 1] if k in ("depth", "bgr") else v) for k, v in sc.items()}
        C.reference(one, (0, 1, 2, 3), world_T_base=sc["world_T_base"][f:f + 1], vol=vol)
    want = C.host_reference(W, H, N, False, (0, 1, 2, 3))
    for k in want:
        np.testing.assert_array_equal(vol[k], want[k], err_msg=k)


def test_spec_matches_the_oracle_helpers():
    """dense_rig's products and inverse are oracle/numpy_rig's, bit for bit; the use rule."""
    rng = np.random.default_rng(5)
    sc = C.rgbd_scene(W, H, N)
    for _ in range(4):
        a, b = rng.normal(size=(4, 4)), rng.normal(size=(4, 4))
        np.testing.assert_array_equal(dense_rig.mul4(a, b), numpy_rig.mul4(a, b))
        np.testing.assert_array_equal(dense_rig.inv_rigid(a), numpy_rig.inv_rigid(a))
    for p in range(4):
        np.testing.assert_array_equal(dense_rig.rig_world_T_cam(sc["E"], sc["world_T_base"][2], p),
                                      REF.world_T_cam(sc["E"], sc["world_T_base"][2], p))
    # pair 0 at frame 0 sits at the volume's origin, to rounding
    np.testing.assert_allclose(REF.world_T_cam(sc["E"], np.eye(4), 0), np.eye(4), atol=1e-12)
    assert [dense_rig.frame_used(s, g) for s, g in ((0, 0), (0, 5), (2, 0), (2, 5), (1, 0), (1, 5))] == \
        [True, True, True, False, False, False]
    assert REF.used_device([2, 0, 1, 0], 0) == [True, True, False, True]
    assert REF.used_device([2, 0], 4) == [False, True]
    assert dense_rig.chunk_frames(3) == 85 and dense_rig.chunk_frames(4) == 64 and dense_rig.chunk_frames(1) == 256
    assert dense_rig.view_order(2, 2) == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_config_validation():
    ok = dict(rgbd=True, dense_map=True)
    HipSlamConfig(**ok, dense_cameras="all").validate()
    HipSlamConfig(**ok, dense_cameras=(1, "192.168.2.25")).validate()
    HipSlamConfig(**ok).validate()
    assert HipSlamConfig().dense_cameras == ()
    for kw in (dict(rgbd=True, dense_cameras="all"),                               # no dense_map
               dict(**ok, dense_cameras=(1, 1)),                                   # a duplicate entry
               dict(**ok, dense_cameras="every"),
               dict(**ok, dense_cameras="all", devices=(0, 0, 0, 0), shard_transport="copy")):
        with pytest.raises(ValueError, match="dense_cameras"):
            HipSlamConfig(**kw).validate()


def test_name_resolution():
    names = list(C.NAMES)
    r = dense_rig.resolve_dense_cameras
    assert r((), names) == () and r((), names[:1]) == ()
    assert r("all", names) == (0, 1, 2, 3)
    assert r(("192.168.2.25", 1), names) == (1, 3)           # ascending pair order, names and indices mixed
    assert r((np.int64(2),), names) == (2,)
    for spec, nm in ((("192.168.2.99",), names), ((4,), names), ((-1,), names), ((1, "192.168.2.22"), names),
                     ("all", names[:1]), ((0,), names[:1]), ((1.5,), names), ((True,), names)):
        with pytest.raises(ValueError, match="dense_cameras"):
            r(spec, nm)


def test_engine_initialize_refuses():
    """The refusals reach the caller of ``initialize`` as ValueError, before any device is touched."""
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.slam.hip_engine import HipSlamEngine
    from thor_slam_amd.synthetic import SyntheticRGBDSource, synthetic_rgbd_rig

    _, rig = synthetic_rgbd_rig(C.joints(), C.NAMES, 160, 120)
    base = dict(rgbd=True, n_features=1000, n_levels=3)
    for kw in (dict(dense_map=True, dense_cameras=("192.168.2.99",)),             # an unknown name
               dict(dense_map=True, dense_cameras=(0, "192.168.2.21")),           # the same camera twice
               dict(dense_map=True, dense_cameras=(7,)),
               dict(dense_cameras="all"),                                          # no dense_map
               dict(dense_map=True, dense_cameras="all", devices=(0, 0, 0, 0), shard_transport="copy")):
        eng = HipSlamEngine(num_cameras=8, config=HipSlamConfig(**base, **kw))
        with pytest.raises(ValueError, match="dense_cameras"):
            eng.initialize(rig.calibration)
    src = SyntheticRGBDSource(width=160, height=120)
    one = CameraRig([src], rig_extrinsics={src.name: Extrinsics.from_4x4_matrix(src.rig_T_source)})
    eng = HipSlamEngine(num_cameras=2, config=HipSlamConfig(**base, dense_map=True, dense_cameras="all"))
    with pytest.raises(ValueError, match="several pairs"):
        eng.initialize(one.calibration)
