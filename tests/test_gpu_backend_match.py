"""The back-end Hamming matchers and compactors on the device — ``k_reloc_match`` / ``k_reloc_corr``
(k_reloc.hip), ``k_loop_vote`` / ``loop_store_block`` (k_loop.hip) — on the crafted inputs of
tests/backend_match_cases.py, compared exactly (integers equal, f64 as bits) with the NumPy oracles
that tests/test_backend_match_cpu.py pins to a scalar reference.

The inputs go in through ``Handle.copy_in``: a small handle processes four frames of noise, then the
frames' ring slots (left camera: keypoint records, level counts, descriptors, disparities) are
overwritten with a case's frame before ``map_upload`` / ``relocalize`` / ``reloc_read`` or
``loop_add_keyframe`` / ``loop_query`` / ``loop_job_vote`` / ``loop_verify`` run on them.

A failing case is reported by its id; every test collects all its failing ids before it asserts.
"""

from __future__ import annotations

import numpy as np
import pytest

import backend_match_cases as B
from oracle import numpy_loop as L
from oracle import numpy_map as OM

pytestmark = pytest.mark.gpu

CFG = B.cfg()
MIN_CORR = max(6, CFG.min_inliers)


@pytest.fixture(scope="module")
def handle():
    import torch

    from thor_slam_amd._lib import Handle

    h = Handle([B.rect()], CFG, max_batch=B.N_FRAMES)
    assert (h.K, h.n_levels, list(h.quotas), list(h.koff)) == (B.K, B.N_LEVELS, list(B.QUOTAS), list(B.KOFF))
    assert h.n_cams == 2 and h.n_pairs == 1
    noise = np.random.default_rng(1).integers(0, 256, (B.N_FRAMES, 2, B.HEIGHT, B.WIDTH), dtype=np.uint8)
    dev = torch.from_numpy(noise).cuda()
    h.submit(dev.data_ptr(), B.N_FRAMES, torch.cuda.current_stream().cuda_stream)
    h.sync()
    assert h.frames_done == B.N_FRAMES
    yield h
    h.close()


def write_frame(h, g: int, frame: dict) -> None:
    """The frame into the left camera (camera 0 of pair 0) of global frame g's ring slot."""
    slot = h.ring_slot(g)
    for which, key in (("keypoints", "kps"), ("kcount", "kcount"), ("desc", "desc"), ("disp", "disp")):
        _, _, per = h.buffer_info(which)
        h.copy_in(which, slot * per, frame[key])


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def reloc_mismatch(h, res: dict, frame: dict, map_desc, map_xyz) -> str:
    """'' when what the device left equals the reference: all K matches, the count, the first
    n_corr correspondence rows bit for bit, and the status rule of k_reloc_corr."""
    feat = B.features(frame)
    want = OM.match_map(feat, np.asarray(map_desc, dtype=np.uint32).reshape(-1, 8), CFG)
    rows = OM.corr_rows(OM.correspondences(feat, want, map_xyz, B.intrinsics()[:4]))
    n = int((want >= 0).sum())
    rd = h.reloc_read()
    st = res["stats"]
    if not np.array_equal(rd["match"], want):
        bad = np.nonzero(rd["match"] != want)[0]
        return f"match differs at keypoints {bad[:6].tolist()}: got {rd['match'][bad[:6]].tolist()}, want {want[bad[:6]].tolist()}"
    if (want[~feat["valid"]] >= 0).any():
        return "the reference matched a keypoint past its count"
    if st[1] != n:
        return f"stats[1] = {st[1]}, {n} matches"
    if rd["corr"].shape != rows.shape or not np.array_equal(bits(rd["corr"]), bits(rows)):
        return f"correspondence rows differ ({rd['corr'].shape} vs {rows.shape})"
    # k_reloc_corr leaves status 1 exactly when n < max(6, min_inliers), and the pose solve behind it
    # replaces the status.  Below the bound nothing was solved: no inliers, no winner.  At or above
    # it the solve ran (it left a winner); the maps here agree with the keypoints under the identity
    # pose, so it succeeds wherever a pose exists, that is with four or more distinct map points
    # matched, and with fewer it fails in RANSAC, not in k_reloc_corr.
    solved = not (st[3] == 0 and st[4] == -1)
    if n < MIN_CORR:
        ok = st[0] == 1 and not solved and st[2] == 0
    elif np.unique(want[want >= 0]).size >= 4:
        ok = st[0] != 1 and solved
    else:
        ok = st[0] == 1 and solved
    if not ok:
        return f"stats[0] = {st[0]} with {n} correspondences (stats {st.tolist()})"
    return ""


def run_reloc(h, g: int, frame: dict, map_desc, map_xyz) -> str:
    h.map_upload(map_xyz, map_desc)
    return reloc_mismatch(h, h.relocalize(g), frame, map_desc, map_xyz)


# -- relocalisation matches ------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("size", (513, 1025))
def test_reloc_boundary_order_and_position(handle, size, part):
    """Every boundary variant with its best and second train at every ordered pair of positions from
    {0, 1, M-2, M-1} and the edges of the 512-descriptor LDS chunks (a quarter of the variants per
    part)."""
    h = handle
    xyz = B.map_points()[:size]
    fails, n, last = [], 0, None
    variants = B.boundary_variants(CFG)
    keep = {v.vid for i, v in enumerate(variants) if i % 4 == part}
    for case in B.reloc_boundary_cases(CFG, sizes=(size,)):
        if case["variant"].vid not in keep:
            continue
        if case["frame"] is not last:
            last = case["frame"]
            write_frame(h, 1, last)
        msg = run_reloc(h, 1, last, case["map_desc"], xyz)
        if msg:
            fails.append(f"{case['id']}: {msg}")
        n += 1
    assert n == len(keep) * len(B.position_pairs(size, B.CHUNK_POSITIONS)) and n > 0
    assert not fails, f"{len(fails)} of {n} cases failed, e.g. " + "; ".join(fails[:12])


def test_reloc_map_sizes_tie_heavy_and_stale_state(handle):
    """Tie-heavy maps of 0, 1, 2 and 511 ... 1025 points, ordered so that every short map follows
    a longer one on the same handle: nothing of the longer map or of its matches may be read."""
    h = handle
    fails = []
    order = (1025, 0, 2, 1024, 1, 513, 512, 511, 0)
    assert set(order) == set(B.MAP_SIZES)
    for i, size in enumerate(order):
        case = B.fuzz_map_case(size)
        want = OM.match_map(B.features(case["frame"]), case["map_desc"], CFG)
        fr, xyz = B.consistent_geometry(case["frame"], want, size, 5100 + size)
        write_frame(h, i % B.N_FRAMES, fr)
        msg = run_reloc(h, i % B.N_FRAMES, fr, case["map_desc"], xyz)
        if msg:
            fails.append(f"{case['id']} (step {i}): {msg}")
        if size == 0:
            assert (want < 0).all()
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("pid", [p[0] for p in B.PATTERNS])
def test_reloc_correspondence_compaction(handle, pid):
    """Accept flags in the validity patterns (empty, single keypoints at the wave and pass edges,
    everything, alternating, whole waves, random) through k_reloc_corr's multi-pass block scan."""
    case = B.reloc_pattern_case(pid)
    write_frame(handle, 2, case["frame"])
    msg = run_reloc(handle, 2, case["frame"], case["map_desc"], case["map_xyz"])
    assert not msg, f"{case['id']}: {msg}"
    n = int(case["survivors"].sum())
    assert handle.reloc_read()["corr"].shape == (n, 8)


def test_loop_verify_leaves_the_same_matches(handle):
    """loop_verify matches the query frame against a database entry's landmarks (its count read back
    from the device): matches, rows and counts as the reference on the entry's descriptors and xyz."""
    h = handle
    case = B.verify_case()
    h.loop_init(4, 256)
    write_frame(h, 0, case["candidate"])
    write_frame(h, 3, case["query"])
    slot, n = h.loop_add_keyframe(0)
    kf = L.keyframe_landmarks(B.features(case["candidate"]), case["candidate"]["disp"], B.intrinsics())
    assert n == len(kf["kp"]) > 256
    msg = reloc_mismatch(h, h.loop_verify(3, slot), case["query"], kf["desc"], kf["xyz"])
    assert not msg, msg
    # an entry with no landmark: nothing matches, and nothing of the last verification stays readable
    write_frame(h, 0, B.store_pattern_case("empty")["frame"])
    slot, n = h.loop_add_keyframe(0)
    assert n == 0
    msg = reloc_mismatch(h, h.loop_verify(3, slot), case["query"], np.zeros((0, 8), np.uint32), np.zeros((0, 3)))
    assert not msg, msg


# -- keyframe store --------------------------------------------------------------------------------
def test_keyframe_store_patterns(handle):
    """Every validity pattern through loop_store_block's block scan (K = 1000: four passes, the
    last one partial), into a database of three entries so that each entry is reused by patterns
    with fewer landmarks."""
    h = handle
    h.loop_init(3, 256)
    fails = []
    order = ["everything"] + [p[0] for p in B.PATTERNS if p[0] != "everything"]
    for i, pid in enumerate(order):
        case = B.store_pattern_case(pid)
        fr = case["frame"]
        write_frame(h, i % B.N_FRAMES, fr)
        slot, n = h.loop_add_keyframe(i % B.N_FRAMES)
        want = L.keyframe_landmarks(B.features(fr), fr["disp"], B.intrinsics())
        got = h.loop_read_keyframe(slot)
        ok = (slot == i % 3 and n == len(want["kp"]) == int(case["survivors"].sum()) and got["desc"].shape == want["desc"].shape
              and np.array_equal(got["desc"], want["desc"]) and np.array_equal(bits(got["xyz"]), bits(want["xyz"])))
        if not ok:
            fails.append(f"{case['id']}: {n} landmarks, want {len(want['kp'])}")
    assert not fails, "; ".join(fails)


# -- votes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", B.SIGNATURES)
def test_signature_votes_and_windows(handle, S):
    """Signatures off the wave size against entries of 0, 1, S-1, S, S+1 landmarks (as candidate and
    as query), in a five-entry database filled past its capacity; the vote jobs over wrapping windows
    equal loop_query and the reference."""
    h = handle
    h.loop_init(B.DB_CAP, S)
    db = [None] * B.DB_CAP
    for i, fr in enumerate(B.signature_sequence(S)):
        write_frame(h, i % B.N_FRAMES, fr)
        slot, n = h.loop_add_keyframe(i % B.N_FRAMES)
        want = L.keyframe_landmarks(B.features(fr), fr["disp"], B.intrinsics())
        assert slot == i % B.DB_CAP and n == len(want["kp"])
        got = h.loop_read_keyframe(slot)
        np.testing.assert_array_equal(got["desc"], want["desc"])
        np.testing.assert_array_equal(bits(got["xyz"]), bits(want["xyz"]))
        db[slot] = want["desc"]
    assert sorted(len(d) for d in db) == sorted([0, 1, max(S - 1, 0), S, S + 1])
    fails = []
    for q in range(B.DB_CAP):
        want = np.array([L.vote(db[q], db[c], S, CFG.max_hamming, CFG.ratio_pct) for c in range(B.DB_CAP)])
        votes = h.loop_query(q, B.DB_CAP)
        if not np.array_equal(votes, want):
            fails.append(f"S{S}-query{q} ({len(db[q])} landmarks): {votes.tolist()} want {want.tolist()}")
        for k0, n_kf in B.WINDOWS:
            got = h.loop_job_vote(q, k0, n_kf).result(block=True)
            ent = B.window_entries(k0, n_kf)
            if not (np.array_equal(got, want[ent]) and np.array_equal(got, votes[ent])):
                fails.append(f"S{S}-query{q}-window({k0},{n_kf}): {got.tolist()} want {want[ent].tolist()}")
    assert not fails, "; ".join(fails[:10])


def test_vote_boundary_order_and_position(handle):
    """Every boundary variant as a query keyframe (designed, anchor and random landmark) against
    twelve candidates: best and second at every ordered pair of {0, 1, S-2, S-1} of a 256-entry
    signature, and an exact copy of the designed query at index S, which the signature ends before."""
    h = handle
    S = B.VOTE_S
    cases = list(B.vote_boundary_cases(CFG))
    h.loop_init(13 * len(cases), S)
    fails, g = [], 0
    for v, q, cands in cases:
        base = None
        for a, b, c in cands + [(None, None, q)]:
            tail = q[0] if a is not None else c[0]
            write_frame(h, g % B.N_FRAMES, B.landmark_frame(c, 9000 + g, tail=tail))
            slot, n = h.loop_add_keyframe(g % B.N_FRAMES)
            assert n == len(c) and slot == g
            base = slot if base is None else base
            g += 1
        q_slot = base + len(cands)
        votes = h.loop_query(q_slot, q_slot)[base:]
        want = np.array([L.vote(q, c, S, CFG.max_hamming, CFG.ratio_pct) for _, _, c in cands])
        for (a, b, _), got, w in zip(cands, votes, want):
            if got != w:
                fails.append(f"{v.vid}-b{a}-s{b}: {got} votes, want {w}")
    assert not fails, f"{len(fails)} cases failed, e.g. " + "; ".join(fails[:12])
