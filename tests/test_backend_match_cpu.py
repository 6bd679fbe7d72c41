"""The crafted back-end matcher cases (tests/backend_match_cases.py) against an independent scalar
reference — plain Python integers, explicit loops, ``int.bit_count`` — and the NumPy oracles the GPU
tests compare the device with (``numpy_map.match_map``, ``numpy_loop.vote``,
``numpy_loop.keyframe_landmarks``).  No GPU.

The rule the scalar reference carries: best = the lexicographic minimum of (distance, index) over
the trains, second = that minimum over the others; accepted iff best <= max_hamming and (no second
or 100 * best < ratio_pct * second).

Non-triviality: in every boundary and fuzz case the reference accepts at least a quarter and rejects
at least a quarter of the valid queries.  Three kinds of case cannot: a map of no points accepts
nothing; the ``far`` variant (best distance 256) forces every train to be the complement of the
query, so all trains are equal and every query of the case ties; and votes of signatures with
fewer than four query landmarks or fewer than two candidate landmarks have too few outcomes.
Those are checked for equality only.
"""

from __future__ import annotations

import math

import numpy as np
import pytest

import backend_match_cases as B
from oracle import numpy_loop as L
from oracle import numpy_map as M

CFG = B.cfg()
MH, RATIO = CFG.max_hamming, CFG.ratio_pct


# -- the scalar reference --------------------------------------------------------------------------
def as_int(d) -> int:
    return int.from_bytes(np.asarray(d, dtype="<u4").tobytes(), "little")


def ints(desc) -> list:
    raw = np.ascontiguousarray(desc, dtype="<u4").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def dist(a: int, b: int) -> int:
    return (a ^ b).bit_count()


def scalar_best_second(q: int, trains: list):
    """((bd, bi), (sd, si) or None) by the rule above; None for no trains."""
    if not trains:
        return None, None
    bd, bi = 257, -1
    for j, t in enumerate(trains):   # ascending j and a strict "<": the lowest index among equal distances
        d = (q ^ t).bit_count()
        if d < bd:
            bd, bi = d, j
    sd, si = 257, -1
    for j, t in enumerate(trains):
        if j == bi:
            continue
        d = (q ^ t).bit_count()
        if d < sd:
            sd, si = d, j
    return (bd, bi), ((sd, si) if si >= 0 else None)


def scalar_accept(best, second) -> bool:
    if best is None or best[0] > MH:
        return False
    return second is None or 100 * best[0] < RATIO * second[0]


def scalar_valid(frame: dict) -> list:
    out = []
    for k in range(B.K):
        level = int(frame["kps"][k, 1]) & 0xFF
        out.append(k - B.KOFF[level] < int(frame["kcount"][level]))
    return out


_VALID = {}


def cached_valid(frame: dict) -> list:
    if id(frame) not in _VALID:
        _VALID[id(frame)] = (frame, scalar_valid(frame))   # the frame is kept alive with its entry
    return _VALID[id(frame)][1]


def scalar_match_map(frame: dict, map_desc) -> np.ndarray:
    trains = ints(map_desc)
    out = np.full(B.K, -1, dtype=np.int64)
    for k, ok in enumerate(cached_valid(frame)):
        if not ok:
            continue
        best, second = scalar_best_second(as_int(frame["desc"][k]), trains)
        if scalar_accept(best, second):
            out[k] = best[1]
    return out


def scalar_vote(q_desc, c_desc, S: int) -> int:
    trains = ints(c_desc[:S])
    votes = 0
    if not trains:
        return 0
    for q in ints(q_desc[:S]):
        votes += scalar_accept(*scalar_best_second(q, trains))
    return votes


def scalar_landmarks(frame: dict, intr) -> dict:
    """Valid keypoints with a finite disparity > 0, in keypoint order; z = fx B / d, x = (u - cx) z /
    fx, y = (v - cy) z / fy with (u, v) = ((x + 0.5) 2^l - 0.5, (y + 0.5) 2^l - 0.5)."""
    fx, fy, cx, cy, fxb = intr
    xyz, desc, kp = [], [], []
    for k, ok in enumerate(scalar_valid(frame)):
        d = float(frame["disp"][k])
        if not ok or not math.isfinite(d) or not d > 0.0:
            continue
        xy, level = int(frame["kps"][k, 0]), int(frame["kps"][k, 1]) & 0xFF
        sc = float(1 << level)
        u, v = (float(xy & 0xFFFF) + 0.5) * sc - 0.5, (float(xy >> 16) + 0.5) * sc - 0.5
        z = fxb / d
        xyz.append([(u - cx) * z / fx, (v - cy) * z / fy, z])
        desc.append(frame["desc"][k])
        kp.append(k)
    return {"xyz": np.array(xyz, dtype=np.float64).reshape(-1, 3), "desc": np.array(desc, dtype=np.uint32).reshape(-1, 8),
            "kp": np.array(kp, dtype=np.int64)}


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_mixed(match: np.ndarray, valid, what: str) -> None:
    n = int(np.sum(valid))
    acc = int(np.sum(match[np.asarray(valid)] >= 0))
    assert 4 * acc >= n and 4 * (n - acc) >= n, f"{what}: {acc} of {n} valid queries accepted"


# -- boundary constructions ------------------------------------------------------------------------
def test_boundary_variants_have_the_distances_they_claim():
    variants = B.boundary_variants(CFG)
    g = math.gcd(100, RATIO)
    on_line = [(v.bd, v.sd) for v in variants if v.vid.startswith("eq") and "-" not in v.vid]
    assert on_line == [(RATIO * t // g, 100 * t // g) for t in range(1, 256 * g // 100 + 1)] and len(on_line) >= 50
    assert all(100 * bd == RATIO * sd for bd, sd in on_line)
    ids = [v.vid for v in variants]
    assert len(set(ids)) == len(ids)
    for want in ("mh", "mh+1", "zero-single", "zero-twice", "far", "tie3"):
        assert want in ids
    for v in variants:
        d = B.variant_descs(*v[:4])
        q = as_int(d["q"])
        assert dist(q, as_int(d["best"])) == v.bd
        assert [dist(q, as_int(s)) for s in d["seconds"]] == [v.sd] * v.n_second
        if 0 < v.sd < 256:   # distinct trains: a tie is between different descriptors
            assert len({as_int(x) for x in [d["best"]] + d["seconds"]}) == 1 + v.n_second
        assert dist(q, as_int(B.complement(d["q"]))) == 256 >= min(v.sd + 8, 256)
        assert dist(q, as_int(d["extra"])) == 236
        # the acceptance each variant claims, from the rule itself
        assert v.accept == (v.bd <= MH and 100 * v.bd < RATIO * v.sd)
    by = {v.vid: v for v in variants}
    assert by["eq1"].accept is False and by["eq1-bd"].accept is True and by["eq1-sd"].accept is False
    assert (by["mh"].bd, by["mh+1"].bd) == (MH, MH + 1) and by["mh"].accept and not by["mh+1"].accept


def test_reloc_boundary_cases_against_scalar_and_oracle():
    n_cases, seen_pos = 0, set()
    for case in B.reloc_boundary_cases(CFG):
        v, fr, tr, a, b = case["variant"], case["frame"], case["map_desc"], case["a"], case["b"]
        d = B.variant_descs(*v[:4])
        trains = ints(tr)
        q = as_int(d["q"])
        # the construction: best at a, second at b, nothing else nearer than min(sd + 8, 256)
        assert dist(q, trains[a]) == v.bd and dist(q, trains[b]) == v.sd
        others = sorted(dist(q, t) for j, t in enumerate(trains) if j not in (a, b))
        assert sum(x == v.sd for x in others if v.sd < 236) == v.n_second - 1
        assert all(x >= min(v.sd + 8, 256) for x in others if x != v.sd), case["id"]
        want = scalar_match_map(fr, tr)
        assert want[B.Q_DESIGNED] == B.designed_match(v, a, b), case["id"]
        best, second = scalar_best_second(q, trains)
        assert best[0] == v.bd and second[0] == v.sd, case["id"]
        if v.bd < v.sd:
            assert best[1] == a
        got = M.match_map(B.features(fr), tr, CFG)
        np.testing.assert_array_equal(got, want, err_msg=case["id"])
        valid = cached_valid(fr)
        assert np.array_equal(B.features(fr)["valid"], valid) and 3 <= sum(valid) <= 4 and valid[B.Q_DESIGNED]
        if v.vid != "far":
            assert_mixed(want, valid, case["id"])
        else:
            assert (want < 0).all()
        n_cases += 1
        seen_pos.add((len(tr), a, b))
    nv = len(B.boundary_variants(CFG))
    assert n_cases == nv * (20 + 56) and len(seen_pos) == 76
    for M_, p in ((513, (511, 512)), (513, (512, 511)), (1025, (511, 512)), (1025, (1023, 1024)), (1025, (1024, 0)), (1025, (513, 510))):
        assert (M_,) + p in seen_pos


def test_vote_boundary_cases_against_scalar_and_oracle():
    S = B.VOTE_S
    n = 0
    for v, q, cands in B.vote_boundary_cases(CFG):
        assert len(cands) == 12
        for a, b, c in cands:
            assert len(c) == S + 1 and np.array_equal(c[S], q[0])   # the copy past the signature
            want = scalar_vote(q, c, S)
            assert L.vote(q, c, S, MH, RATIO) == want, (v.vid, a, b)
            designed = scalar_accept(*scalar_best_second(as_int(q[0]), ints(c[:S])))
            assert designed == v.accept, (v.vid, a, b)
            if v.vid != "far":
                assert 4 * want >= len(q) and 4 * (len(q) - want) >= len(q), (v.vid, a, b, want)
            if not v.accept and v.bd > 0:   # reaching the copy at index S would accept the designed query
                assert scalar_vote(q[:1], c, S + 1) == 1
            n += 1
    assert n == 12 * len(B.boundary_variants(CFG))


# -- tie-heavy fuzz and the map sizes ----------------------------------------------------------------
@pytest.mark.parametrize("size", B.MAP_SIZES)
def test_fuzz_map_cases_against_scalar_and_oracle(size):
    case = B.fuzz_map_case(size)
    fr, tr = case["frame"], case["map_desc"]
    assert len(tr) == size
    want = scalar_match_map(fr, tr)
    np.testing.assert_array_equal(M.match_map(B.features(fr), tr, CFG), want)
    valid = np.array(cached_valid(fr))
    assert valid.sum() == 300 + B.QUOTAS[1] + B.QUOTAS[2] - 1
    assert (want[~valid] < 0).all()
    if size == 0:
        assert (want < 0).all()
        return
    assert_mixed(want, valid, case["id"])
    if size == 1:   # no second: max_hamming alone decides, on both sides of it
        d = np.array([dist(as_int(fr["desc"][k]), as_int(tr[0])) for k in np.nonzero(valid)[0]])
        np.testing.assert_array_equal(want[valid] >= 0, d <= MH)
        assert (d <= MH).any() and (d > MH).any()
    if size >= 511:   # tie-heavy: hundreds of trains repeat a distance for every query, some the best one
        trains = ints(tr)
        best_ties = 0
        for k in np.nonzero(valid)[0][:100]:
            ds = [dist(as_int(fr["desc"][k]), t) for t in trains]
            assert size - len(set(ds)) >= 200
            best_ties += ds.count(min(ds)) > 1
        assert best_ties >= 5, best_ties
    if size > B.RL_CHUNK:   # some accepted matches lie in every LDS chunk
        assert ((want >= 0) & (want < B.RL_CHUNK)).any() and (want >= B.RL_CHUNK).any()


# -- compaction patterns -----------------------------------------------------------------------------
@pytest.mark.parametrize("pid", [p[0] for p in B.PATTERNS])
def test_store_patterns_against_scalar_and_oracle(pid):
    case = B.store_pattern_case(pid)
    fr, intr = case["frame"], B.intrinsics()
    want = scalar_landmarks(fr, intr)
    got = L.keyframe_landmarks(B.features(fr), fr["disp"], intr)
    np.testing.assert_array_equal(got["kp"], want["kp"])
    np.testing.assert_array_equal(got["desc"], want["desc"])
    assert same_bits(got["xyz"], want["xyz"])
    np.testing.assert_array_equal(want["kp"], np.nonzero(case["survivors"])[0])
    n = len(want["kp"])
    if pid in B.TRIVIAL_PATTERNS:
        assert n == (B.K if pid == "everything" else 0)
    else:
        assert 1 <= n <= B.K - 1
    if pid.startswith("single-"):
        assert list(want["kp"]) == [int(pid.split("-")[1])]
    # the keypoints the pattern drops hold every kind of dead disparity, the ones past the counts live ones
    valid = np.array(scalar_valid(fr))
    dead = fr["disp"][valid & ~case["survivors"]]
    if dead.size >= 6:
        assert np.isnan(dead).any() and np.isposinf(dead).any() and (dead == 0).any() and (dead < 0).any()
    assert (fr["disp"][~valid] > 0).all() and np.isfinite(fr["disp"][~valid]).all()
    assert np.isfinite(want["xyz"]).all() and (want["xyz"][:, 2] > 0).all()


def test_patterns_cover_the_level_counts():
    kinds = set()
    for _, _, kcount in B.PATTERNS:
        for c, q in zip(kcount, B.QUOTAS):
            kinds.add("empty" if c == 0 else "full" if c == q else "short" if c == q - 1 else "other")
    assert {"empty", "full", "short"} <= kinds
    assert B.K % 256 != 0 and B.KOFF == [0, 763, 953]


@pytest.mark.parametrize("pid", [p[0] for p in B.PATTERNS])
def test_reloc_patterns_against_scalar_and_oracle(pid):
    case = B.reloc_pattern_case(pid)
    fr, tr = case["frame"], case["map_desc"]
    want = scalar_match_map(fr, tr)
    np.testing.assert_array_equal(M.match_map(B.features(fr), tr, CFG), want)
    on = np.nonzero(case["survivors"])[0]
    np.testing.assert_array_equal(np.nonzero(want >= 0)[0], on)
    np.testing.assert_array_equal(want[on], np.arange(on.size))
    if pid not in B.TRIVIAL_PATTERNS:
        assert 1 <= on.size <= B.K - 1
    # records and map points agree under the identity pose (level 0 exactly, coarser levels to their pixel)
    fx, fy, cx, cy, _ = B.intrinsics()
    u, v = B.level0(fr)
    X = case["map_xyz"][want[on]]
    eu, ev = fx * X[:, 0] / X[:, 2] + cx - u[on], fy * X[:, 1] / X[:, 2] + cy - v[on]
    lev = B.LEVEL_OF[on]
    assert (np.abs(eu) <= 0.5 * (1 << lev) + 1e-9).all() and (np.abs(ev) <= 0.5 * (1 << lev) + 1e-9).all()
    assert (np.abs(eu[lev == 0]) < 1e-9).all()
    assert (X[:, 2] >= 1).all() and (X[:, 2] <= 5).all()
    rows = M.corr_rows(M.correspondences(B.features(fr), want, case["map_xyz"], B.intrinsics()[:4]))
    assert rows.shape == (on.size, 8) and np.isfinite(rows).all()
    np.testing.assert_allclose(np.linalg.norm(rows[:, 5:8], axis=1), 1.0, rtol=0, atol=1e-15)


# -- signatures and windows --------------------------------------------------------------------------
@pytest.mark.parametrize("S", B.SIGNATURES)
def test_signature_cases_against_scalar_and_oracle(S):
    frames = B.signature_sequence(S)
    intr = B.intrinsics()
    lms = []
    for fr in frames:
        want = scalar_landmarks(fr, intr)
        got = L.keyframe_landmarks(B.features(fr), fr["disp"], intr)
        np.testing.assert_array_equal(got["desc"], want["desc"])
        assert same_bits(got["xyz"], want["xyz"])
        lms.append(want)
    assert [len(x["kp"]) for x in lms] == [2 * S + 40, 2 * S + 40, max(S - 1, 0), S, S + 1, 0, 1]
    db = [lms[5], lms[6], lms[2], lms[3], lms[4]]   # entry = position mod 5: 0 and 1 were overwritten
    assert sorted(len(x["kp"]) for x in db) == sorted([0, 1, max(S - 1, 0), S, S + 1])
    mixed = 0
    for q in range(B.DB_CAP):
        for c in range(B.DB_CAP):
            want = scalar_vote(db[q]["desc"], db[c]["desc"], S)
            assert L.vote(db[q]["desc"], db[c]["desc"], S, MH, RATIO) == want, (S, q, c)
            nq, nc = min(S, len(db[q]["kp"])), min(S, len(db[c]["kp"]))
            if nq == 0 or nc == 0:
                assert want == 0
            if nq >= 4 and nc >= 2 and q != c:
                assert 4 * want >= nq and 4 * (nq - want) >= nq, (S, q, c, want, nq)
                mixed += 1
    assert mixed >= (6 if S >= 5 else 0)
    # the stale entries would vote differently: what entries 0 and 1 held before they were reused
    if S >= 4:
        assert scalar_vote(db[3]["desc"], lms[0]["desc"], S) != scalar_vote(db[3]["desc"], db[0]["desc"], S)


def test_windows_wrap():
    got = {w: B.window_entries(*w) for w in B.WINDOWS}
    assert got[(0, 1)] == [0] and got[(0, 5)] == [0, 1, 2, 3, 4]
    assert got[(3, 1)] == [3] and got[(3, 5)] == [3, 4, 0, 1, 2]
    assert got[(4, 1)] == [4] and got[(4, 5)] == [4, 0, 1, 2, 3]
    assert B.window_entries(3, 2, capk=5, P=2) == [6, 7, 8, 9]
