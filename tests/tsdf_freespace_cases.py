"""What the free-space layer's tests share (tests/test_tsdf_freespace_cpu.py and
tests/test_gpu_tsdf_freespace.py): the scenes of tests/tsdf_dynamic_cases.py (imported, the volume
37 x 29 x 41 off every brick multiple, the cameras 67 x 77 and 131 x 69), one call of six frames, a
written layer that holds every kind of word, and the resting-object chain.  Every scene is used only
after the guard of tests/ref_tsdf_freespace.py has shown that scaling ``band`` by 1 +- 1e-9 changes no
observation (and the mask's own guard that no pixel sits on its gates).  References are computed once
and handed out read-only."""

from __future__ import annotations

import functools

import numpy as np

import ref_tsdf_freespace as RF
import tsdf_dynamic_cases as C
from oracle import numpy_tsdf as OT

BAND_VOX = 1.5
BAND = BAND_VOX * C.S
DIMS = tuple(int(n) for n in C.DIMS)
SHAPE = DIMS[::-1]
PERMUTED = (0, 1, 2, 5, 4, 3)   # the frames of `call` in another order: the last sphere frame after the box


def start_layer(settle: int) -> np.ndarray:
    """A layer to write before a call: zeros, runs of settle - 1, settled words, and 65535 (saturated,
    with and without the bit), spread over the voxels so that every brick holds all of them."""
    k, j, i = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij")
    kind = (i + 2 * j + 3 * k) % 5
    words = np.select([kind == 1, kind == 2, kind == 3, kind == 4],
                      [settle - 1, RF.SETTLED_BIT | settle, RF.SETTLED_BIT | RF.SATURATED, RF.SATURATED], 0).astype(np.uint32)
    words.setflags(write=False)
    return words


def guard(cam, depth, T, origin=C.ORIGIN, vol=None):
    """Both guards of one used frame; the nearest |sdf| to a gate of the band."""
    ok, gap = RF.guarded(DIMS, origin, C.S, cam, depth, T, C.MAX_D, BAND)
    assert ok and gap > 0.0, gap
    assert C.guarded(depth, T, cam, vol=vol, origin=origin)
    return gap


@functools.lru_cache(maxsize=None)
def call(cam):
    """(frames [6][H][W], poses [6][4][4], object pixels of the sphere): sphere, sphere, static, sphere,
    static on a NaN pose, the box from a perturbed pose; guarded."""
    static = C.static_depth(cam)
    sphere, obj = C.with_sphere(static, cam, *C.SPHERE)
    box, _ = C.with_box(static, cam, C.EDGE_BOX)
    frames = np.stack([sphere, sphere, static, sphere, static, box])
    poses = np.stack([C.T_STAR, C.T_STAR, C.T_STAR, C.T_STAR, C.NAN, C.PERTURBED[0]])
    gaps = [guard(cam, frames[f], poses[f]) for f in (0, 2, 5)]
    frames.setflags(write=False)
    poses.setflags(write=False)
    return frames, poses, obj, min(gaps)


@functools.lru_cache(maxsize=None)
def call_reference(cam, settle=2):
    """The reference of that call from ``start_layer(settle)``: mask, depth, stats, words."""
    frames, poses, _, _ = call(cam)
    t, w = C.volume()
    ref = RF.dynamic(t, w, start_layer(settle), C.ORIGIN, C.S, C.TRUNC, cam, frames, poses, settle, BAND_VOX, max_dist=C.MAX_D,
                     **C.PRM)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def ball_voxels() -> np.ndarray:
    """The voxels whose centre lies in the sphere of the scenes, [nz][ny][nx]."""
    centre = (C.T_STAR @ np.array([*C.SPHERE[0], 1.0]))[:3]
    return np.linalg.norm(C.A.centres() - centre, axis=-1) <= C.SPHERE[1]


CHAIN_SETTLE = 3
CHAIN = ("sphere",) * 5 + ("static",) * 2   # one-frame calls: the object rests, then is taken away


@functools.lru_cache(maxsize=1)
def chain_reference():
    """The resting object, call by call on the 67 x 77 camera: tslam_tsdf_dynamic then
    tslam_tsdf_integrate_rect of the filtered depth, settle_frames 3, band 1.5, default radii.  Per
    call: the mask outputs, and the volume and the layer after it (oracle.numpy_tsdf.integrate and the
    reference's update).  Also (frames by name, object pixels)."""
    cam = C.CAM
    static = C.static_depth(cam)
    sphere, obj = C.with_sphere(static, cam, *C.SPHERE)
    frames = {"sphere": sphere, "static": static}
    t, w = (a.copy() for a in C.volume())
    words = np.zeros(SHAPE, np.uint32)
    q = RF.inverse_pose(C.T_STAR)
    steps = []
    for name in CHAIN:
        assert C.guarded(frames[name], C.T_STAR, cam, vol=(t, w))          # the mask's gates against the volume as it stands
        ref = RF.dynamic(t, w, words, C.ORIGIN, C.S, C.TRUNC, cam, frames[name][None], C.T_STAR[None], CHAIN_SETTLE, BAND_VOX,
                         max_dist=C.MAX_D, **C.PRM)
        words = ref["words"]
        OT.integrate(t, w, ref["depth"][0], q, cam[2:], C.ORIGIN, C.S, C.TRUNC, C.MAX_D, C.MAX_W)
        steps.append({"mask": ref["mask"][0], "depth": ref["depth"][0], "stats": ref["stats"][0], "words": words.copy(),
                      "tsdf": t.copy(), "weight": w.copy()})
    ok, gap = RF.guarded(DIMS, C.ORIGIN, C.S, cam, sphere, C.T_STAR, C.MAX_D, BAND)
    assert ok
    for st in steps:
        for a in st.values():
            a.setflags(write=False)
    return steps, frames, obj, gap
