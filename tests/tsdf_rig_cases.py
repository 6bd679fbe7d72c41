"""Scenes and references shared by the dense-map-of-a-rig tests (cached per process): the
4-camera RGB-D rig on the brackets.urdf joints (tests/golden/brackets_joints.json) in the shared
room, ground-truth body poses, and the volume that surrounds the rig."""

from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

import ref_tsdf_rig as REF

NAMES = ("192.168.2.21", "192.168.2.22", "192.168.2.23", "192.168.2.25")
ORIGIN = (-7.2, -1.8, -7.2)      # volume frame: pair 0's camera at frame 0 (RDF); the room all around it
DIMS = (144, 36, 144)
VOX, TRUNC_VOX, MAX_D, MAX_W = 0.1, 4.0, 10.0, 100.0


def joints() -> dict:
    return json.loads((Path(__file__).parent / "golden" / "brackets_joints.json").read_text())


@functools.lru_cache(maxsize=4)
def rgbd_scene(width: int, height: int, n: int, distorted: bool = False) -> dict:
    """Rendered frames of the bracket RGB-D rig: ``depth[f][p]`` / ``bgr[f][p]``, records
    [n][P][5HW], product undistortion per camera, E[p] = base_T_cam and the ground-truth body poses
    world_T_base[f] (base at frame 0)."""
    from helpers import DISTORTION
    from thor_slam_amd.calib import extract_cameras, rgbd_pairs, rgbd_undistort
    from thor_slam_amd.camera import Extrinsics
    from thor_slam_amd.camera.rig import CameraRig
    from thor_slam_amd.rgbd import pack_rgbd
    from thor_slam_amd.synthetic import RoomScene, SyntheticRGBDSource, circle_trajectory

    mats = joints()
    scene = RoomScene(seed=0)
    traj = circle_trajectory(40)
    srcs = [SyntheticRGBDSource(name=nm, scene=scene, trajectory=traj, rig_T_source=np.array(mats[nm]), seed=k,
                                width=width, height=height, distortion=DISTORTION if distorted else None)
            for k, nm in enumerate(NAMES)]
    rig = CameraRig(srcs, rig_extrinsics={nm: Extrinsics.from_4x4_matrix(np.array(mats[nm])) for nm in NAMES})
    cams = extract_cameras(rig.calibration, 2 * len(NAMES))
    pairs = rgbd_pairs(cams)
    rects = [rgbd_undistort(cams[c]) for c, _ in pairs]
    E = [cams[c].extrinsics.to_4x4_matrix() @ r.left_optical_T_rect() for (c, _), r in zip(pairs, rects)]
    by_name = {s.name: s for s in srcs}
    raw = [[by_name[cams[c].source_name].render_rgbd(i) for c, _ in pairs] for i in range(n)]
    records = np.stack([np.stack([pack_rgbd(b, d) for b, d in fr]) for fr in raw])
    inv0 = np.linalg.inv(traj[0])
    return {"depth": [[d for _, d in fr] for fr in raw], "bgr": [[b for b, _ in fr] for fr in raw], "records": records,
            "rects": rects, "E": E, "world_T_base": np.stack([inv0 @ traj[f] for f in range(n)]),
            "names": [cams[c].source_name for c, _ in pairs]}


def reference(sc: dict, pairs, n: int | None = None, world_T_base=None, used=None, max_weight: float = MAX_W,
              color: bool = True, order: str = "frame", dims=DIMS, origin=ORIGIN, vol: dict | None = None) -> dict:
    """ref_tsdf_rig on a scene's first n frames of cameras ``pairs``."""
    n = len(sc["depth"]) if n is None else n
    wtb = sc["world_T_base"][:n] if world_T_base is None else world_T_base
    used = REF.used_host(wtb) if used is None else used
    depth = [[sc["depth"][f][p] for p in pairs] for f in range(n)]
    bgr = [[sc["bgr"][f][p] for p in pairs] for f in range(n)] if color else None
    return REF.integrate_rig(REF.new_volume(dims) if vol is None else vol, list(pairs), depth, wtb, used, sc["E"], sc["rects"],
                             origin, VOX, TRUNC_VOX * VOX, MAX_D, max_weight, bgr=bgr, order=order)


@functools.lru_cache(maxsize=8)
def host_reference(width: int, height: int, n: int, distorted: bool, pairs: tuple, max_weight: float = MAX_W,
                   order: str = "frame", scene_n: int | None = None) -> dict:
    """The reference on ground-truth body poses of the first n frames (of a scene of ``scene_n``),
    with colour (tsdf / weight are the same without); shared, never written to."""
    vol = reference(rgbd_scene(width, height, scene_n or n, distorted), pairs, n=n, max_weight=max_weight, order=order)
    for a in vol.values():
        a.setflags(write=False)
    return vol
