"""Front-end parity at image sizes off the 16-byte grid and on tie-heavy images (the cases and
their preconditions: tests/frontend_cases.py, tests/test_frontend_cases_cpu.py).

Every parity test elsewhere runs at 640x400, 1280x800, 1280x720 or 320x240, where each level's
rows are 16-byte multiples: rectify's byte path, detect's non-DMA staging and scalar FAST / NMS,
describe's narrow staging and the RGB-D byte path run only here, as do the sizes next to the limits
the kernels' packed fields set (W = 2044, H = 2047, 64 x 64, a coarsest level of 41 x 41) and images
that overflow a select score bucket, cut inside a score bin, repeat their descriptors or hold
nothing.  Same bar as tests/test_gpu_parity.py: everything up to the correspondences bit-exact, the
RANSAC winner identical, poses within 1e-9 relative Frobenius.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

import frontend_cases as FC
from helpers import DISTORTION, rel_frobenius
from test_gpu_parity import _check_image_features, _levels, hip_run

pytestmark = pytest.mark.gpu


def _device_run(rect, cfg, frames, batch, keep=False):
    """The frames through a fresh handle in batches of `batch`: per frame the blocks hip_run reads."""
    import torch

    from thor_slam_amd._lib import Handle

    n, K = len(frames), cfg.n_features
    h = Handle([rect], cfg, max_batch=batch)
    dev = torch.from_numpy(np.array(frames)).cuda()      # a writable copy of the cached input
    s = torch.cuda.current_stream().cuda_stream
    per = []
    for b0 in range(0, n, batch):
        nb = min(batch, n - b0)
        h.submit(dev[b0:].data_ptr(), nb, s)
        res = h.read_poses(nb)
        for f in range(nb):
            g = b0 + f
            slot = h.ring_slot(g)
            per.append({
                "pyr": h.frame_block("pyramid", slot, np.uint8).reshape(2, h.pyr_bytes),
                "kp": [h.keypoints(g, 0), h.keypoints(g, 1)],
                "stereo": h.frame_block("stereo", slot, np.int32)[:K],
                "disp": h.frame_block("disp", slot, np.float64)[:K],
                "temporal": h.frame_block("temporal", slot, np.int32)[:K],
                "tuv": h.frame_block("temporal_uv", f, np.float64)[: 2 * K].reshape(K, 2),
                "corr": h.frame_block("corr", f, np.float64)[: 8 * K].reshape(K, 8),
                "T_rel": res["T_rel"][f, 0], "T_abs": res["T_abs"][f, 0], "stats": res["stats"][f, 0],
            })
    if keep:
        return per, h, res
    h.close()
    return per


def _check_front_end(oracle, per, cfg, width, height, what, features_only=False):
    """Pyramids, keypoints, descriptors (features_only stops here), matches, disparities, refined
    positions, correspondences and n_corr of every frame, bit-exact."""
    from thor_slam_amd.params import level_shapes

    wh = level_shapes(width, height, cfg.n_levels)
    off = FC.pyramid_offsets(width, height, cfg.n_levels)
    assert len(per) == len(oracle)
    for i, (rec, o) in enumerate(zip(per, oracle)):
        cur = o["cur"]
        for cam, side in enumerate(("left", "right")):
            for l, lev in enumerate(_levels(rec["pyr"][cam], off, wh)):
                np.testing.assert_array_equal(lev, cur[side]["levels"][l], err_msg=f"{what} frame {i} {side} level {l}")
            _check_image_features(cur[side], rec["kp"][cam], cfg, f"{what} frame {i} {side}")
        if features_only:
            continue
        np.testing.assert_array_equal(rec["stereo"], cur["stereo"], err_msg=f"{what} frame {i} stereo matches")
        np.testing.assert_array_equal(np.isnan(rec["disp"]), np.isnan(cur["disp"]), err_msg=f"{what} frame {i} disparity validity")
        ok = ~np.isnan(cur["disp"])
        np.testing.assert_array_equal(rec["disp"][ok], cur["disp"][ok], err_msg=f"{what} frame {i} refined disparity")
        np.testing.assert_array_equal(rec["temporal"], cur["temporal"], err_msg=f"{what} frame {i} temporal matches")
        if i == 0:
            assert (rec["temporal"] == -1).all() and rec["stats"][0] == 2
            continue
        corr = o["corr"]
        n = corr["X"].size
        np.testing.assert_array_equal(rec["tuv"][corr["j"], 0], corr["u"], err_msg=f"{what} frame {i} refined u")
        np.testing.assert_array_equal(rec["tuv"][corr["j"], 1], corr["v"], err_msg=f"{what} frame {i} refined v")
        assert rec["stats"][1] == n == o["n_corr"], f"{what} frame {i}: n_corr {rec['stats'][1]} vs oracle {n}"
        for col, key in enumerate(("X", "Y", "Z", "du", "dv")):
            np.testing.assert_array_equal(rec["corr"][:n, col], corr[key], err_msg=f"{what} frame {i} corr {key}")


def _check_poses(oracle, per, what):
    for i, (rec, o) in enumerate(zip(per, oracle)):
        st = rec["stats"]
        assert st[0] == o["status"], f"{what} frame {i}: status {st[0]} vs {o['status']}"
        if i == 0:
            np.testing.assert_array_equal(rec["T_abs"], np.eye(4))
        if o["status"] != 0:
            continue
        assert st[4] == o["best_hyp"] and st[3] == o["best_count"], f"{what} frame {i}: RANSAC winner differs"
        assert st[2] == o["n_inliers"], f"{what} frame {i}: inliers {st[2]} vs {o['n_inliers']}"
        assert rel_frobenius(rec["T_rel"], o["T"]) < 1e-9, f"{what} frame {i}: T_rel"
        assert rel_frobenius(rec["T_abs"], o["world_T_cam"]) < 1e-9, f"{what} frame {i}: T_abs"


# -- rendered sequences at G1 .. G8 --------------------------------------------------------------
@pytest.mark.parametrize("batch", [3, 1])
@pytest.mark.parametrize("gid", list(FC.GEOMETRIES))
def test_geometry_bit_exact(gid, batch):
    """batch = 3: one launch; batch = 1: frames 1 and 2 run under the speculative threshold the
    frame before committed, at that geometry."""
    w, h, _, _, distorted = FC.GEOMETRIES[gid]
    sc, per = hip_run(seed=FC.SEED, batch=batch, distorted=distorted, n=FC.N_FRAMES, cfg_items=FC.cfg_items(gid),
                      width=w, height=h)
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, f"{gid} batch {batch}")
    _check_poses(sc["oracle"], per, f"{gid} batch {batch}")


# -- hand-made images ----------------------------------------------------------------------------
@pytest.mark.parametrize("content,fast_threshold", [(c, None) for c in FC.CONTENTS] + [("noise", 0), ("blocks", 254)])
@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_hand_made_content_bit_exact(sid, content, fast_threshold):
    """noise: the top-K cut falls inside a score bin; periodic: the lowest-index tie rules of the
    matcher decide; blocks: a select score bucket above its counting-sort capacity; flat: no
    candidate at any level.  No pose assertions (degenerate scenes)."""
    sc = FC.hand_scenario(sid, content, fast_threshold)
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=FC.N_FRAMES)
    _check_front_end(sc["oracle"], per, sc["cfg"], *FC.HAND_SIZES[sid], f"{sid} {content} t={fast_threshold}")


@pytest.mark.parametrize("sid", sorted(FC.HAND_SIZES))
def test_threshold_learnt_then_overflow_nothing_and_recovery(sid):
    """Batches of 1 over rendered, rendered, blocks, flat, noise, rendered: the speculative
    threshold learnt on texture meets a bucket overflow, then an empty image (its fallback finds
    nothing either), then recovers.  Keypoints and descriptors bit-exact on every frame."""
    sc = FC.mixed_scenario(sid)
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=1)
    _check_front_end(sc["oracle"], per, sc["cfg"], *FC.HAND_SIZES[sid], f"{sid} mixed", features_only=True)


@pytest.mark.parametrize("gid", FC.LIMIT_SIZES)
def test_keypoints_on_the_limits_of_the_key_fields(gid):
    """`dots` at W = 2044, H = 2047 and W = 2047: keypoints on the first and last legal column and
    row (x = 2024 / 2027, y = 2027 in the 11-bit key fields, quad 506 of detect's 9-bit queue entries),
    all in one score bucket above the counting sort's capacity."""
    w, h, _, _, _ = FC.GEOMETRIES[gid]
    sc = FC.limit_scenario(gid)
    per = _device_run(sc["rect"], sc["cfg"], sc["frames"], batch=FC.N_FRAMES)
    _check_front_end(sc["oracle"], per, sc["cfg"], w, h, f"{gid} dots")


# -- RGB-D ---------------------------------------------------------------------------------------
RGBD_W, RGBD_H = 330, 251    # W * H % 4 == 2: k_rgbd_gray's byte path


@functools.lru_cache(maxsize=1)
def _rgbd_odd_scenario():
    from oracle import numpy_slam as O
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=RGBD_W, height=RGBD_H, distortion=DISTORTION)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    rect = rgbd_undistort(cams[ci])
    cfg = HipSlamConfig(rgbd=True, n_features=600, n_levels=3)
    trk = O.OracleTracker(cfg, dict(fx=rect.fx, fy=rect.fy, cx=rect.cx, cy=rect.cy, baseline=rect.baseline,
                                    map_l=rect.map_left, map_r=rect.map_right))
    oracle = [trk.step_rgbd(*src.render_rgbd(i)) for i in range(3)]
    return {"src": src, "rect": rect, "cfg": cfg, "oracle": oracle, "records": src.render_rgbd_sequence(3)[:, None, :]}


def test_rgbd_byte_path_bit_exact():
    from test_gpu_rgbd import _check, _hip

    assert (RGBD_W * RGBD_H) % 4 == 2
    sc = _rgbd_odd_scenario()
    assert not sc["rect"].is_identity
    assert all(o["status"] == 0 for o in sc["oracle"][1:])
    _check(sc, _hip(sc, 3))


def test_rgbd_odd_pixel_count_is_refused():
    """329 x 251: the u16 depth plane behind W * H * 3 colour bytes would be misaligned."""
    from thor_slam_amd._lib import Handle
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.params import HipSlamConfig
    from thor_slam_amd.synthetic import SyntheticRGBDSource

    src = SyntheticRGBDSource(width=329, height=251)
    cams = extract_cameras(CameraRig([src]).calibration, 2)
    (ci, _), = rgbd_pairs(cams)
    with pytest.raises(RuntimeError, match=r"tslam error -1: .*even pixel count"):   # TSLAM_EINVAL
        Handle([rgbd_undistort(cams[ci])], HipSlamConfig(rgbd=True, n_features=600, n_levels=3), max_batch=1)


# -- the dense matcher and the TSDF on the G3 handle's ring ---------------------------------------
def test_g3_stereo_depth_and_tsdf_bit_exact():
    """stereo_depth(0, 3) on the ring-resident level-0 images of the G3 handle (329 x 251: odd pitch,
    odd height) against ref_stereo_depth, and tsdf_integrate_rect of that depth against numpy_tsdf."""
    import torch

    import ref_stereo_depth as REF
    from test_gpu_stereo_depth import DIMS, MAX_D, MAX_W, ORIGIN, TRUNC_VOX, VOX, _level0, _oracle_tsdf, _used

    n, n_disp = FC.N_FRAMES, 48
    sc = FC.geometry_scenario("G3")
    rect = sc["rect"]
    per, h, res = _device_run(rect, sc["cfg"], sc["frames"], batch=n, keep=True)
    try:
        s = torch.cuda.current_stream().cuda_stream
        h.stereo_depth_init(max_frames=n, n_disp=n_disp)
        h.stereo_depth(0, n, pair=0, stream=s)
        got = [h.stereo_depth_read(f) for f in range(n)]
        want = []
        for f in range(n):
            left, right = _level0(h, f, 0), _level0(h, f, 1)
            np.testing.assert_array_equal(left, sc["oracle"][f]["cur"]["rect_left"])
            want.append(REF.stereo_depth(left, right, n_disp, rect.fx * rect.baseline))
            assert (want[f][0] > 0).mean() > 0.3
            np.testing.assert_array_equal(got[f][1], want[f][1], err_msg=f"disp32 of frame {f}")
            np.testing.assert_array_equal(got[f][0], want[f][0], err_msg=f"depth of frame {f}")
        depth_ptr, _, frame_bytes = h.stereo_depth_buffers()
        assert frame_bytes == 2 * 329 * 251
        h.tsdf_init(ORIGIN, DIMS, VOX, TRUNC_VOX, MAX_D, MAX_W)
        h.tsdf_integrate_rect(depth_ptr, frame_bytes, n, first_frame=0, stream=s)
        got_t, got_w = h.tsdf_read()
        used = _used(res)
        assert all(used)
        want_t, want_w = _oracle_tsdf(rect, [d for d, _ in want], res["T_abs"][:, 0], used)
        assert (want_w > 0).sum() > 10000
        np.testing.assert_array_equal(got_w, want_w)
        np.testing.assert_array_equal(got_t, want_t)
    finally:
        h.close()
