"""Why the ray caster's step_scale defaults to 0.5 (thor_slam_amd/dense_render.py).

    python tools/tsdf_render_step_scale.py

On the NumPy reference, no GPU: a wall 2 m ahead in a 60 x 30 x 40 volume of 0.05 m, integrated by
oracle/numpy_tsdf.py from one 160x120 depth frame taken at 0, 68 and 79 degrees incidence, rendered
head-on at step_scale 1.0 and 0.5.  Per case: the share of pixels that hit, the mean samples of the
rays that sample at all, and the median |depth - 2 m| of the hits.  The TSDF is projective, so along
the head-on ray it over-estimates the distance to a wall that was seen at a grazing angle, and a full
step jumps the thin negative band.
"""

from __future__ import annotations

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "thor-slam_amd"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
from oracle import numpy_tsdf as NT  # noqa: E402
from thor_slam_amd import dense_render as DR  # noqa: E402

s=0.05; dims=(60,30,40); origin=(-1.5,-0.75,1.0)
W,H,fx,fy,cx,cy=160,120,140.0,140.0,79.5,59.5
wall_z=2.0
for inc in (0,68,79):
    a=np.deg2rad(inc)
    R=np.array([[np.cos(a),0,np.sin(a)],[0,1,0],[-np.sin(a),0,np.cos(a)]])
    fwd=R[:,2]; C=np.array([0,0,wall_z])-2.0*fwd
    T=np.eye(4);T[:3,:3]=R;T[:3,3]=C
    ys,xs=np.mgrid[0:H,0:W]
    d=np.stack([(xs-cx)/fx,(ys-cy)/fy,np.ones((H,W))],-1)@R.T
    with np.errstate(divide='ignore',invalid='ignore'):
        t=(wall_z-C[2])/d[...,2]
    depth=np.where((t>0)&(t<10),np.floor(1000*t+0.5),0).astype(np.uint16)
    tsdf=np.zeros(dims[::-1],np.float32);w=np.zeros_like(tsdf)
    NT.integrate(tsdf,w,depth,DR.rigid_inverse(T),(fx,fy,cx,cy),origin,s,4*s,10.0,100.0)
    for sc in (1.0,0.5):
        o=DR.render_view(tsdf,w,origin,s,(W,H,fx,fy,cx,cy),np.eye(4),step_scale=sc)
        hit=o['depth_m']>0
        print(inc,sc,'hit',round(hit.mean(),3),'mean samples',round(o['samples'][o['samples']>0].mean(),1),'med err',np.median(np.abs(o['depth_m'][hit]-wall_z)) if hit.any() else None)
