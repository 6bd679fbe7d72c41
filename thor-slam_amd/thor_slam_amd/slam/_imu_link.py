"""The IMU coupling of the engine: the filter's motion priors for a staged
batch, the local BA's IMU factors, and what the filter absorbs of a published batch.

The filter (``thor_slam_amd/imu.py``) absorbs the vision of batch s - 1 - ``imu_prior_lag`` and no
later one before batch s's priors, whatever has already come back, so the priors are a function of
the data alone; over the batches still pending the state coasts."""

from __future__ import annotations

import numpy as np

from .._lib import POSE_OK
from ..imu import ImuPropagator, vision_only
from ._se3 import _invert, adjoint


class _ImuLink:
    """``handle`` takes the BA factors (rank 0's on a sharded rig) and counts the frames;
    ``set_motion_prior(rot, w_rot, trn, w_trn)`` puts a batch's priors on every handle;
    ``publish_next()`` publishes the oldest batch in flight, waiting for it (False: none is)."""

    def __init__(self, imu: ImuPropagator, cfg, handle, base_T_rects: list, base_T_imu: np.ndarray,
                 set_motion_prior, publish_next) -> None:
        self.imu, self.cfg, self.h = imu, cfg, handle
        self.P = len(base_T_rects)
        self.e0 = base_T_rects[0]
        self.base_T_imu = base_T_imu
        self.moves = [(_invert(ep) @ self.e0, _invert(self.e0), ep) for ep in base_T_rects]   # (inv(E_p) E_0, inv(E_0), E_p)
        self.set_motion_prior, self.publish_next = set_motion_prior, publish_next
        # submitted batches whose vision the filter has not absorbed yet, in order: {"n": batch
        # number, "samples", "steps", "res": the absorb inputs once published} (no "samples": no data)
        self.batches: list = []
        self.seq = 0                      # batches submitted (numbers the entries)
        self.kf_imu: tuple | None = None  # gyro rotation since the last BA keyframe (R, var, first frame)
        self.kf_ine: tuple | None = None  # samples since the last BA keyframe (list, first frame, w_prev)

    def reset(self) -> None:
        self.batches, self.seq, self.kf_imu, self.kf_ine = [], 0, None, None
        self.imu.reset()

    def priors(self, stamps: list[float], imus: list, prev: float | None) -> None:
        """Per staged frame and pair: the motion predicted by the IMU filter for pair 0's
        rectified-left camera over the frame interval (``prev``: the timestamp of the last frame
        submitted before) — the bias-corrected gyro rotation with its weight and, with the
        accelerometer leg, the translation with its weight — moved into every other pair's camera
        through the rig, inv(E_p) E_0 T inv(E_0) E_p.  The samples are kept for the filter's update
        when the batch's results come back."""
        imu = self.imu
        seq = self.seq
        self.seq += 1
        self._absorb_due(seq)
        if not imu.ready and all(s is None for s in imus):   # no IMU sample yet: nothing to predict,
            self.batches.append({"n": seq, "res": None})       # and the batch may stay in flight
            return
        samples = []
        for ts, s in zip(stamps, imus):
            ok = s is not None and (s[1] is not None or not imu.accel)
            if ok and not imu.ready:
                imu.begin(s[1])            # this frame anchors the filter: no prior for it
                samples.append((None, None, None))
            elif ok and prev is not None and ts > prev:
                samples.append((ts - prev, s[0], s[1]))
            else:
                samples.append((None, None, None))
            prev = ts
        # the vision of the batches still pending (at most imu_prior_lag of them) is not in the
        # filter yet: the state coasts over their samples (oracle/numpy_imu.py lagged_priors)
        coast = [c for e in self.batches if "samples" in e for c in e["samples"]]
        steps = imu.batch_priors(coast + samples)[len(coast):]
        self._ba_imu_factors(steps)
        self._ba_inertial_factors(steps, samples)
        P, n = self.P, len(stamps)
        rot = np.tile(np.eye(3), (n, P, 1, 1))
        trn = np.zeros((n, P, 3))
        wr, wt = np.zeros((n, P)), np.zeros((n, P))
        for k, st in enumerate(steps):
            if st is None:
                continue
            t0 = np.eye(4)
            t0[:3, :3], t0[:3, 3] = st.R_rel, st.t_rel
            for p, (a, ie0, ep) in enumerate(self.moves):
                tp = t0 if p == 0 else a @ t0 @ ie0 @ ep   # the same products, in the same order, as before
                rot[k, p], trn[k, p] = tp[:3, :3], tp[:3, 3]
                wr[k, p], wt[k, p] = st.w_rot, st.w_trans
        self.set_motion_prior(rot, wr, trn, wt)
        self.batches.append({"n": seq, "samples": samples, "steps": steps, "res": None})

    def _absorb_due(self, seq: int) -> None:
        """Before batch ``seq``'s priors: the filter absorbs the vision of every batch numbered
        <= seq - 1 - imu_prior_lag (waiting for its results if needed), in order, and no other."""
        lag = max(int(self.cfg.imu_prior_lag), 0)
        while self.batches and self.batches[0]["n"] <= seq - 1 - lag:
            while self.batches[0]["res"] is None:
                if not self.publish_next():
                    raise RuntimeError("IMU filter: a batch to absorb was never published")
            e = self.batches.pop(0)
            if "samples" in e:
                self.imu.absorb(e["samples"], *e["res"])

    def _ba_imu_factors(self, steps: list) -> None:
        """The local BA's IMU rotation factors (one stereo pair): the per-frame gyro rotations of
        the staged batch composed since the last keyframe; at each keyframe whose whole interval
        had IMU steps, the rotation from the previous keyframe's camera and the inverse of the
        summed rotation variances (1 / rad^2: the reprojection residuals have unit pixel weight)
        go to tslam_ba_imu_factor before the batch is submitted."""
        cfg = self.cfg
        if cfg.ba_window <= 0 or self.P != 1:
            return
        if self._ine_on():   # the inertial records carry the gyro rotation (and the gyroscope bias)
            return
        g = self.h.frames_done
        for k, st in enumerate(steps):
            gk = g + k
            if st is None or self.kf_imu is None:
                self.kf_imu = None if st is None else (st.R_rel.copy(), 1.0 / st.w_rot, gk)
            else:
                rot, var, start = self.kf_imu
                self.kf_imu = (st.R_rel @ rot, var + 1.0 / st.w_rot, start)
            if gk % cfg.ba_kf_interval == 0:
                acc = self.kf_imu
                if acc is not None and acc[2] == gk - cfg.ba_kf_interval + 1 and acc[1] > 0.0:
                    self.h.ba_imu_factor(gk, acc[0], 1.0 / acc[1])
                self.kf_imu = (np.eye(3), 0.0, gk + 1)

    def _ine_on(self) -> bool:
        """The local BA takes tightly coupled inertial factors (accelerometer leg, filter started)."""
        return (self.cfg.ba_window > 0 and bool(self.cfg.ba_inertial) and bool(self.imu.accel) and bool(self.imu.ready))

    def _ba_inertial_factors(self, steps: list, samples: list) -> None:
        """The local BA's tightly coupled inertial factors (accelerometer leg): the frame
        intervals' samples since the last BA keyframe are preintegrated with the filter's current
        biases (tslam_imu_preintegrate); at each keyframe whose whole interval had samples the
        record and the keyframe's predicted world velocity go to tslam_ba_inertial_factor, and the
        window gets the filter's gravity and accelerometer-bias prior (tslam_ba_inertial) before
        the batch is submitted.  One stereo pair: in pair 0's rectified-left camera; a rig: in the
        body (base_link) frame of its body window (pair = n_pairs), the filter's camera-0 vectors
        rotated into it (the velocity only seeds the solve)."""
        cfg, imu = self.cfg, self.imu
        if not self._ine_on():
            return
        rig = self.P > 1
        pair = self.P if rig else 0
        R0 = self.e0[:3, :3]   # base_R_rect0: camera-0 vectors into the body world
        st = imu.st
        g = imu.gravity()
        self.h.ba_inertial(R0 @ g if rig else g, st.ba, 1.0 / max(st.var_b, 1e-12), st.bg,
                           1.0 / max(st.var_g, 1e-12), pair=pair)
        floors = dict(r_floor=cfg.ba_inertial_r_floor, ba_floor=cfg.ba_inertial_ba_floor, bg_floor=cfg.ba_inertial_bg_floor)
        g = self.h.frames_done
        for k, (step, smp) in enumerate(zip(steps, samples)):
            gk = g + k
            if step is None or step.v1 is None or smp[0] is None:
                self.kf_ine = None
            else:
                if self.kf_ine is None:
                    self.kf_ine = ([], gk, None)
                self.kf_ine[0].append(smp)
            if gk % cfg.ba_kf_interval == 0:
                acc = self.kf_ine
                if acc is not None and acc[1] == gk - cfg.ba_kf_interval + 1 and len(acc[0]) == cfg.ba_kf_interval:
                    if rig:
                        rec = imu.preintegrate(acc[0], st.bg, st.ba, None if acc[2] is None else R0 @ acc[2],
                                               cfg.ba_inertial_v_floor, cfg.ba_inertial_p_floor,
                                               frame_R_imu=self.base_T_imu[:3, :3], lever=self.base_T_imu[:3, 3],
                                               **floors)
                        self.h.ba_inertial_factor(gk, rec, R0 @ step.v1, pair=pair)
                    else:
                        rec = imu.preintegrate(acc[0], st.bg, st.ba, acc[2], cfg.ba_inertial_v_floor,
                                               cfg.ba_inertial_p_floor, **floors)
                        self.h.ba_inertial_factor(gk, rec, step.v1)
                self.kf_ine = ([], gk + 1, None if step is None else step.w.copy())

    def record(self, res: dict) -> None:
        """A published batch's result into its entry: what the filter absorbs of the tracked motions
        (at the next prior that may use it)."""
        entry = next((e for e in self.batches if e["res"] is None), None)
        if entry is None:
            return
        if "samples" not in entry:
            entry["res"] = ()
            return
        steps = entry["steps"]
        if self.P == 1:   # the vision-only motion behind each prior-weighted solution
            st = res["stats"][:, 0]
            sig = np.ascontiguousarray(st[:, 6:8]).view(np.float64)[:, 0]   # sigma^2 (tslam.h)
            t_rel, cov = res["T_rel"][:, 0].copy(), res["cov"][:, 0].copy()
            for k, step in enumerate(steps[:len(st)]):
                if step is not None and int(st[k, 0]) == POSE_OK:
                    t_rel[k], cov[k] = vision_only(t_rel[k], cov[k], float(sig[k]), step)
            entry["res"] = (st[:, 0].copy(), t_rel, cov)
        else:   # the rig's body motion, moved into pair 0's camera (the filter's frame)
            e0 = self.e0
            ie0, ad = _invert(e0), adjoint(_invert(e0))
            rig = res["rig"]
            t_rel = np.stack([ie0 @ m @ e0 for m in rig["T_rel"]])
            cov = np.stack([ad @ c @ ad.T for c in rig["cov"]])
            entry["res"] = (rig["stats"][:, 0].copy(), t_rel, cov)
