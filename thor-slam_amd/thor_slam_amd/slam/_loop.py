"""Loop closure on the host: the keyframe pose graph and its two drivers.

Place recognition runs over every pair's camera (P database entries per keyframe, keyframe-major)
and verification on the pair that voted best; the keyframe nodes are pair 0's rectified-left poses
(on a multi-pair rig taken from the rig's body poses, k_rig_pose), and the pose-graph correction
moves the body poses.  ``_SyncLoop`` searches at the keyframe, waiting for the device (a sharded
rig: on rank 0's handle); ``_AsyncLoop`` (one device, ``tslam_loop_auto``) runs the search as jobs on
the handle's loop stream while tracking goes on.  The engine's publish path drives either through
``observe`` / ``node`` / ``advance`` and reads ``corr``, ``reloc`` and ``items``; ``fresh()`` gives
``reset`` an empty graph of the same kind."""

from __future__ import annotations

import collections
import logging

import numpy as np

from .._lib import POSE_LOST, POSE_OK, Handle, SingularSystemError
from ..loop import span_edges
from ..params import HipSlamConfig
from ._se3 import _invert

logger = logging.getLogger(__package__ + ".hip_engine")   # the engine's logger, as before the split


class _LoopGraph:
    """Host side of loop closure: keyframe nodes (rect-left world_T_cam), edges, and the
    correction applied to poses after the last solve (corrected = corr @ raw)."""

    asynchronous = False   # searches run as loop jobs; batches may stay in flight
    reloc = False          # RELOCALIZING: no pose is published
    items = ()             # searches in progress

    def __init__(self, handle: Handle, cfg: HipSlamConfig, n_pairs: int, rect0_T_rect: list) -> None:
        self.h, self.cfg, self.P = handle, cfg, n_pairs
        self.m = rect0_T_rect
        self.info_m = self.information(cfg)
        self.frames: list[int] = []
        self.stamps: list[float] = []
        self.raw: list[np.ndarray] = []     # pose at insertion, before loop correction
        self.T: list[np.ndarray] = []       # current (optimised) node poses
        self.edges: list[tuple[int, int]] = []
        self.meas: list[np.ndarray] = []
        self.info: list[np.ndarray] = []
        self.loops: list[tuple[int, int, int]] = []
        self.pairs: list[tuple[int, int]] = []     # per loop: (pair of the older entry, verifying pair)
        self.relocs: list = []      # (keyframe of c, g, inliers)
        self.corr = np.eye(4)
        self.cost = 0.0

    @staticmethod
    def information(cfg) -> np.ndarray:
        return np.diag([1.0 / cfg.pg_sigma_t ** 2] * 3 + [1.0 / cfg.pg_sigma_r ** 2] * 3)

    def fresh(self) -> "_LoopGraph":
        """An empty graph of the same kind on the same handle (``reset``)."""
        return type(self)(self.h, self.cfg, self.P, self.m)

    def _append(self, g: int, raw: np.ndarray, ts: float, first: bool) -> tuple:
        """Keyframe g as the next node, with its odometry edge from the node before unless it is
        the ``first`` of a segment (placed by the current correction).  Returns (node, edge)."""
        idx = len(self.frames)
        if first:
            T, Z = self.corr @ raw, None
        else:
            Z = _invert(self.raw[-1]) @ raw
            T = self.T[-1] @ Z
            self.edges.append((idx - 1, idx))
            self.meas.append(Z)
            self.info.append(self.info_m)
        self.frames.append(g)
        self.stamps.append(ts)
        self.raw.append(raw.copy())
        self.T.append(T)
        return idx, Z

    def observe(self, g: int, status: int) -> None:
        """Frame g's tracking status, before its node."""

    def advance(self, until: int | None = None) -> None:
        """Progress the searches without waiting; complete those due at frame ``until``."""


class _SyncLoop(_LoopGraph):
    """The search at the keyframe itself, each step waited for."""

    full = False

    def node(self, g: int, raw: np.ndarray, ts: float) -> None:
        """Keyframe g: store every pair's view of it in the device database (entry idx * P + p),
        add its odometry edge, look for a loop among the keyframes at least ``loop_min_gap`` older
        (signature votes of each pair's entry against every older entry of every pair; the best
        vote wins, lower pair first), verify it (RANSAC on the voting pair's camera against the
        entry's landmarks) and, on a verified loop, re-solve the pose graph on the device.  A
        pair-q view of a place pair p saw gives the node edge in pair 0's frame:
        T_c^-1 T_q = M_p V^-1 M_q^-1 with V = cam_q_T_cam_p and M_p = rect0_T_rect_p."""
        cfg, h, P = self.cfg, self.h, self.P
        idx = len(self.frames)
        if idx >= cfg.loop_max_keyframes:
            if not self.full:
                logger.warning("loop closure: keyframe database full (%d); no further keyframes", idx)
                self.full = True
            return
        slots = [h.loop_add_keyframe(g, pair=p)[0] for p in range(P)]
        assert slots == list(range(idx * P, idx * P + P))
        self._append(g, raw, ts, first=idx == 0)
        n_allowed = idx - cfg.loop_min_gap + 1
        if n_allowed <= 0:
            return
        best, q, e = -1, 0, 0
        for p, slot in enumerate(slots):
            votes = h.loop_query(slot, n_allowed * P)
            j = int(np.argmax(votes))
            if votes[j] > best:
                best, q, e = int(votes[j]), p, j
        if best < cfg.loop_min_votes:
            return
        ver = h.loop_verify(g, e, pair=q)
        if int(ver["stats"][0]) != POSE_OK or int(ver["stats"][2]) < cfg.loop_min_inliers:
            return
        j, p = divmod(e, P)
        meas = self.m[p] @ _invert(ver["T"]) @ _invert(self.m[q])
        try:
            sol = h.pose_graph(np.stack(self.T), np.array(self.edges + [(j, idx)]), np.stack(self.meas + [meas]),
                               np.stack(self.info + [self.info_m]), cfg.pg_iters)
        except SingularSystemError as exc:   # LoopPolicy's rejection: the loop is dropped, tracking goes on
            logger.warning("loop closure: keyframe %d -> %d rejected (%s)", self.frames[j], g, exc)
            return
        self.edges.append((j, idx))
        self.meas.append(meas)
        self.info.append(self.info_m)
        self.loops.append((self.frames[j], g, int(ver["stats"][2])))
        self.pairs.append((p, q))
        self.T = list(sol["T"])
        self.cost = sol["cost"]
        self.corr = self.T[-1] @ _invert(raw)
        logger.info("loop closure: keyframe %d -> %d (%d inliers), pose graph cost %.3g", self.frames[j], g,
                    int(ver["stats"][2]), sol["cost"])


class _AsyncLoop(_LoopGraph):
    """Loop closure without host waits (one device, ``tslam_loop_auto``): the policy of
    ``oracle/numpy_loop.py`` ``LoopPolicy`` on the device's loop jobs.  The submit path stores every
    keyframe in the database in stream order; a tracked keyframe becomes a node whose search
    (signature votes -> verification -> span solve) runs as jobs on the handle's loop stream while
    tracking goes on; items progress at every call without waiting and complete, oldest first, at
    the latest when their due frame (keyframe + ``loop_latency``) is published — so the published
    poses are a function of the data alone, whatever the timing."""

    MAX_JOBS = 48   # of the library's 64 unreturned job slots

    asynchronous = True

    def __init__(self, handle: Handle, cfg: HipSlamConfig, n_pairs: int, rect0_T_rect: list) -> None:
        super().__init__(handle, cfg, n_pairs, rect0_T_rect)
        self.odo: list = []                 # per node: its odometry edge (None: first of a segment)
        self.items: collections.deque = collections.deque()
        self.jobs = 0   # submitted, not yet returned
        self._busy = False
        self.last_loop: int | None = None   # node of the last closed loop (loop_cooldown)
        self.trace: dict | None = None   # set to {} to record every job's inputs and results (tests)
        self.failures: list = []
        self.rejected: list = []   # (keyframe of c, g) of loops whose span solve was rejected
        # relocalisation after a LOST run (LoopPolicy.observe / _relocate)
        self.lost_run = 0
        self.reloc = False          # RELOCALIZING
        self.anchor_end = 0         # candidates of the episode: nodes < anchor_end
        self.seg_start = 0          # first node of the unanchored segment
        self.last_due = -1

    def observe(self, g: int, status: int) -> None:
        """oracle LoopPolicy.observe: the LOST-run bookkeeping of frame g."""
        if status == POSE_LOST:
            self.lost_run += 1
            after = self.cfg.reloc_after_lost
            if after > 0 and self.lost_run == after and self.frames:
                if not self.reloc:
                    self.reloc = True
                    self.anchor_end = len(self.frames)
                self.seg_start = len(self.frames)
        else:
            self.lost_run = 0

    # -- oracle LoopPolicy._node: node idx = database position idx (tslam_loop_auto) ----------
    def node(self, g: int, raw: np.ndarray, ts: float) -> None:
        idx = len(self.frames)
        _, Z = self._append(g, raw, ts, first=idx == 0 or (self.reloc and idx == self.seg_start))
        self.odo.append(Z)
        cfg = self.cfg
        kind = "reloc" if self.reloc else "loop"
        lo, hi = self._reloc_window(idx) if self.reloc else self._window(idx)
        due = max(g + (cfg.reloc_latency if self.reloc else cfg.loop_latency), self.last_due)
        self.last_due = due
        it = {"idx": idx, "g": g, "due": due, "lo": lo, "n_kf": hi - lo + 1, "kind": kind,
              "stage": "new" if hi >= lo else "done"}
        self.items.append(it)
        self._progress(it, False, len(self.items) == 1)

    def _window(self, idx: int) -> tuple[int, int]:   # oracle numpy_loop.candidate_window
        cfg = self.cfg
        margin = (cfg.loop_latency + 2 * cfg.batch_size - 1) // cfg.loop_kf_interval + 1
        return max(0, idx - cfg.loop_max_keyframes + margin), idx - cfg.loop_min_gap

    def _reloc_window(self, idx: int) -> tuple[int, int]:   # oracle LoopPolicy.reloc_window
        cfg = self.cfg
        margin = (cfg.loop_latency + 2 * cfg.batch_size - 1) // cfg.loop_kf_interval + 1
        return max(0, idx - cfg.loop_max_keyframes + margin), self.anchor_end - 1

    def _entry(self, pos: int, p: int) -> int:
        return (pos % self.cfg.loop_max_keyframes) * self.P + p

    def _result(self, job, block: bool):
        # jobs finish in submission order on the loop stream: once one is still running, a later
        # one is too, so this pass polls no further (each poll is an event query)
        if not block and self._busy:
            return None
        try:
            r = job.result(block)
        except RuntimeError:   # a failed job is returned too (its slot is free): count it out
            self.jobs -= 1
            raise
        if r is not None:
            self.jobs -= 1
        elif not block:
            self._busy = True
        return r

    # -- progress without waiting; `block`: complete it (its due frame is being published) --------
    def advance(self, until: int | None = None) -> None:
        first = True
        self._busy = False
        for it in list(self.items):
            must = until is not None and it["due"] <= until
            self._progress(it, must, first)
            if it["stage"] != "done":
                if must:
                    raise RuntimeError("loop closure: a due item did not complete")
                first = False
                continue
            if first:
                self.items.popleft()

    def _progress(self, it: dict, block: bool, head: bool) -> None:
        cfg, P, h = self.cfg, self.P, self.h
        if it["stage"] == "new":
            if self.jobs + P > self.MAX_JOBS and not block:
                return
            it["votes"] = [h.loop_job_vote(self._entry(it["idx"], q), it["lo"], it["n_kf"]) for q in range(P)]
            self.jobs += P
            it["stage"] = "vote"
        if it["stage"] == "vote":
            got = it.setdefault("got", [None] * P)
            for q, job in enumerate(it["votes"]):
                if got[q] is None:
                    try:
                        got[q] = self._result(job, block)
                    except RuntimeError:   # a failed job (a device error): the item ends here (its
                        it["stage"] = "done"  # other vote jobs stay counted: their slots are unreturned
                        raise
            if any(v is None for v in got):
                return
            if self.trace is not None:
                for q, v in enumerate(got):
                    self.trace[("vote", it["idx"], q)] = (it["lo"], it["n_kf"], v.copy())
            # oracle numpy_loop.best_vote: most votes; ties to the lower query pair, then the newest
            # position (the smallest span), then the lower pair
            best, q, j = -1, 0, 0
            for qq in range(P):
                v = got[qq].reshape(-1, P)
                r = int(np.argmax(v[::-1].reshape(-1)))
                jj = (v.shape[0] - 1 - r // P) * P + r % P
                if int(got[qq][jj]) > best:
                    best, q, j = int(got[qq][jj]), qq, jj
            if best < cfg.loop_min_votes:
                it["stage"] = "done"
                return
            c, pc = it["lo"] + j // P, j % P
            it.update(q=q, c=c, pc=pc, stage="verify")
            it["job"] = h.loop_job_verify(it["g"], self._entry(it["idx"], q), self._entry(c, pc), pair=q)
            self.jobs += 1
        if it["stage"] == "verify":
            try:
                ver = self._result(it["job"], block)
            except RuntimeError:   # a failed job (a device error): the item ends here
                it["stage"] = "done"
                raise
            if ver is None:
                return
            if self.trace is not None:
                self.trace[("verify", it["idx"])] = (it["q"], it["c"], it["pc"], ver)
            if int(ver["stats"][0]) != POSE_OK or int(ver["stats"][2]) < cfg.loop_min_inliers:
                it["stage"] = "done"
                return
            it.update(ver=ver, stage="verified")
        if it["kind"] == "reloc":
            if it["stage"] == "verified" and block:   # applied at the due frame (LoopPolicy._relocate)
                self._relocate(it)
                it["stage"] = "done"
            return
        if it["stage"] == "verified" and head:
            # the span solve starts once every older item is applied, so its inputs (the span's
            # poses and edges, with this loop's edge) are what they are at the due frame
            a, idx, q, pc = it["c"], it["idx"], it["q"], it["pc"]
            if self.last_loop is not None and idx - self.last_loop <= cfg.loop_cooldown:
                it["stage"] = "done"   # within the cooldown of the last closed loop
                return
            it["last_loop"] = self.last_loop   # restored when the span solve is rejected
            self.last_loop = idx
            ver = it["ver"]
            it["edge"] = (a, idx, self.m[pc] @ _invert(ver["T"]) @ _invert(self.m[q]))
            edges = self.edges + [(a, idx)]
            meas = self.meas + [it["edge"][2]]
            sel = span_edges(edges, a, idx)
            args = (np.stack(self.T[a:idx + 1]), np.array([edges[e] for e in sel]) - a, np.stack([meas[e] for e in sel]),
                    np.stack([self.info_m] * len(sel)))
            it["job"] = h.loop_job_pose_graph(*args, cfg.pg_iters)
            it["args"] = args
            self.jobs += 1
            it.update(a=a, stage="solve")
        if it["stage"] == "solve":
            try:
                sol = self._result(it["job"], block)
            except SingularSystemError as exc:
                # LoopPolicy's rejection: the span's normal matrix is not positive definite, so the
                # loop is dropped (no edge, no correction, the cooldown unchanged) and tracking goes
                # on — process_frames keeps the reference's contract (interface.py:192-200)
                self.failures.append({"idx": it["idx"], "g": it["g"], "args": it["args"], "ver": it["ver"],
                                      "q": it["q"], "c": it["c"], "pc": it["pc"], "error": str(exc)})
                self.rejected.append((self.frames[it["a"]], it["g"]))
                self.last_loop = it["last_loop"]
                if self.trace is not None:
                    self.trace[("solve", it["idx"])] = (it["args"], None)
                it["stage"] = "done"
                logger.warning("loop closure: keyframe %d -> %d rejected (%s)", self.frames[it["a"]], it["g"], exc)
                return
            if sol is None:
                return
            it.update(sol=sol, stage="solved")
        if it["stage"] == "solved" and block:   # applied at the due frame, as LoopPolicy does
            a, idx, sol, ver = it["a"], it["idx"], it["sol"], it["ver"]
            if self.trace is not None:
                self.trace[("solve", idx)] = (it["args"], sol)
            self.edges.append((a, idx))
            self.meas.append(it["edge"][2])
            self.info.append(self.info_m)
            self.loops.append((self.frames[a], it["g"], int(ver["stats"][2])))
            self.pairs.append((it["pc"], it["q"]))
            self.T[a:idx + 1] = list(sol["T"])
            for i in range(idx + 1, len(self.T)):
                if self.odo[i] is None:   # a segment break: the nodes after it are anchored otherwise
                    break
                self.T[i] = self.T[i - 1] @ self.odo[i]
            self.corr = self.T[-1] @ _invert(self.raw[-1])
            self.cost = sol["cost"]
            it["stage"] = "done"
            logger.info("loop closure: keyframe %d -> %d (%d inliers), span of %d nodes, cost %.3g",
                        self.frames[a], it["g"], int(it["ver"]["stats"][2]), idx - a + 1, sol["cost"])

    def _relocate(self, it: dict) -> None:
        """oracle LoopPolicy._relocate, from the item's verified candidate: the unanchored
        segment moves rigidly onto the candidate keyframe's pose and tracking resumes."""
        idx, c, q, pc, ver = it["idx"], it["c"], it["q"], it["pc"], it["ver"]
        if not self.reloc or idx < self.seg_start:
            return
        Z = self.m[pc] @ _invert(ver["T"]) @ _invert(self.m[q])
        D = self.T[c] @ Z @ _invert(self.T[idx])
        for i in range(self.seg_start, len(self.T)):
            self.T[i] = D @ self.T[i]
        self.edges.append((c, idx))
        self.meas.append(Z)
        self.info.append(self.info_m)
        self.corr = D @ self.corr
        self.relocs.append((self.frames[c], it["g"], int(ver["stats"][2])))
        self.reloc = False
        self.last_loop = idx
        logger.info("relocalised: keyframe %d against keyframe %d (%d inliers)", it["g"], self.frames[c],
                    int(ver["stats"][2]))
