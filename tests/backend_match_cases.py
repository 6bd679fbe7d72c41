"""Crafted inputs for the back-end Hamming matchers and compactors: ``k_reloc_match`` /
``k_reloc_corr`` (k_reloc.hip) and ``k_loop_vote`` / ``loop_store_block`` (k_loop.hip).
tests/test_backend_match_cpu.py checks every case against a scalar restatement and the NumPy
oracle without a GPU, tests/test_gpu_backend_match.py writes them into the ring buffers of a
small handle (``Handle.copy_in``) and compares the device bit for bit.

Everything here is NumPy, seeded, and independent of the oracle.  One geometry serves all cases:
320 x 240, three levels, 1000 keypoints (K is no multiple of 256: level offsets 0 / 763 / 953).

A *frame* is what one ring slot of the left camera holds: ``kps`` u32 [K][2] (x | y << 16,
level | angle << 8 | score << 16), ``kcount`` i32 [levels], ``desc`` u32 [K][8], ``disp`` f64 [K].
The record at position k carries the level whose quota range holds k, so keypoint k is valid iff
k - koff[level] < kcount[level]: the valid keypoints are a prefix of every level, the ones past
the count are interleaved between the levels and hold live descriptors (copies of train
descriptors: a matcher that ignored the count would accept them).

Boundary construction.  A designed query q has its best train at exactly ``bd`` flipped bits, its
second at exactly ``sd`` flipped bits, and every other train is the complement of q (distance
256 >= min(sd + 8, 256); with sd > 248 nothing else exists at that distance).  Besides q every
boundary case holds an *anchor* query (a copy of the best train: distance 0, accepted) and a
random query (about 128 bits from everything: rejected on max_hamming), so that each case has
accepted and rejected queries whatever the designed one does.
"""

from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

from helpers import make_source, rig_calibration
from thor_slam_amd.calib import extract_cameras, stereo_pairs, stereo_rectify
from thor_slam_amd.params import HipSlamConfig, level_quotas, level_shapes

WIDTH, HEIGHT, N_FEATURES, N_LEVELS, N_FRAMES = 320, 240, 1000, 3, 4
K = N_FEATURES
QUOTAS = level_quotas(N_FEATURES, N_LEVELS)                 # [763, 190, 47]
KOFF = [sum(QUOTAS[:l]) for l in range(N_LEVELS)]           # [0, 763, 953]
LEVEL_WH = level_shapes(WIDTH, HEIGHT, N_LEVELS)
LEVEL_OF = np.repeat(np.arange(N_LEVELS), QUOTAS)           # level of keypoint position k
RL_CHUNK = 512                                              # map descriptors per LDS pass of k_reloc_match
MAP_SIZES = (0, 1, 2, 511, 512, 513, 1024, 1025)
SIGNATURES = (1, 2, 63, 64, 65, 255, 256)
DB_CAP = 5                                                  # max_keyframes of the signature / window cases
WINDOWS = [(k0, n_kf) for k0 in (0, 3, 4) for n_kf in (1, 5)]
FULL, MIXED_A, MIXED_B = tuple(QUOTAS), (QUOTAS[0] - 1, 0, QUOTAS[2]), (QUOTAS[0], QUOTAS[1] - 1, 0)


def cfg() -> HipSlamConfig:
    return HipSlamConfig(n_features=N_FEATURES, n_levels=N_LEVELS)


@functools.lru_cache(maxsize=None)
def rect():
    cams = extract_cameras(rig_calibration(make_source(1, WIDTH, HEIGHT, distorted=False)), 2)
    (li, ri), = stereo_pairs(cams)
    return stereo_rectify(cams[li], cams[ri])


def intrinsics() -> tuple:
    """(fx, fy, cx, cy, fx * baseline) of the handle's only pair."""
    r = rect()
    return (r.fx, r.fy, r.cx, r.cy, r.fx * r.baseline)


# -- descriptors -----------------------------------------------------------------------------------
def random_desc(rng, n: int) -> np.ndarray:
    return rng.integers(0, 2 ** 32, (n, 8), dtype=np.uint32)


def flipped(rng, d: np.ndarray, n: int) -> np.ndarray:
    """``d`` [8] u32 with exactly ``n`` distinct bits flipped."""
    out = np.array(d, dtype=np.uint32, copy=True)
    for b in rng.choice(256, size=n, replace=False):
        out[b >> 5] ^= np.uint32(1 << (int(b) & 31))
    return out


def complement(d: np.ndarray) -> np.ndarray:
    return ~np.asarray(d, dtype=np.uint32)


def _alphabet(rng) -> np.ndarray:
    """Three 32-bit words 8, 10 and 18 bits apart."""
    w0 = int(rng.integers(0, 2 ** 32))
    bits = rng.permutation(32)
    m1 = sum(1 << int(b) for b in bits[:8])
    m2 = sum(1 << int(b) for b in bits[8:18])
    return np.array([w0, w0 ^ m1, w0 ^ m2], dtype=np.uint32)


def alphabet_desc(rng, n: int, words: np.ndarray) -> np.ndarray:
    """Tie-heavy descriptors: each of the 8 words is one of three fixed words, then 0-2 random bits
    flip.  Distances are sums of {0, 8, 10, 18} per word, so hundreds of exact ties occur per query."""
    d = words[rng.integers(0, 3, (n, 8))]
    for i in range(n):
        d[i] = flipped(rng, d[i], int(rng.integers(0, 3)))
    return d.astype(np.uint32)


# -- frames ----------------------------------------------------------------------------------------
def pack_records(x, y, angle, score) -> np.ndarray:
    x, y = np.asarray(x, dtype=np.uint32), np.asarray(y, dtype=np.uint32)
    meta = LEVEL_OF.astype(np.uint32) | (np.asarray(angle, dtype=np.uint32) << 8) | (np.asarray(score, dtype=np.uint32) << 16)
    return np.stack([x | (y << 16), meta], axis=1).astype(np.uint32)


def random_records(rng) -> np.ndarray:
    w = np.array([LEVEL_WH[l][0] for l in LEVEL_OF])
    h = np.array([LEVEL_WH[l][1] for l in LEVEL_OF])
    return pack_records(rng.integers(0, w), rng.integers(0, h), rng.integers(0, 256, K), rng.integers(21, 256, K))


def valid_mask(kcount) -> np.ndarray:
    k = np.arange(K)
    return k - np.asarray(KOFF)[LEVEL_OF] < np.asarray(kcount)[LEVEL_OF]


def make_frame(kps, kcount, desc, disp=None) -> dict:
    f = {"kps": np.ascontiguousarray(kps, dtype=np.uint32), "kcount": np.asarray(kcount, dtype=np.int32),
         "desc": np.ascontiguousarray(desc, dtype=np.uint32),
         "disp": np.full(K, np.nan) if disp is None else np.asarray(disp, dtype=np.float64)}
    assert f["kps"].shape == (K, 2) and f["desc"].shape == (K, 8) and f["disp"].shape == (K,)
    assert np.array_equal(f["kps"][:, 1] & 0xFF, LEVEL_OF) and all(0 <= c <= q for c, q in zip(f["kcount"], QUOTAS))
    return f


def features(frame: dict) -> dict:
    """The frame as the oracle's left-image dict (kp, valid, desc)."""
    kps = frame["kps"]
    kp = {"x": (kps[:, 0] & 0xFFFF).astype(np.int64), "y": (kps[:, 0] >> 16).astype(np.int64),
          "level": (kps[:, 1] & 0xFF).astype(np.int64)}
    return {"kp": kp, "valid": valid_mask(frame["kcount"]), "desc": frame["desc"]}


def level0(frame: dict):
    f = features(frame)["kp"]
    sc = np.left_shift(1, f["level"]).astype(np.float64)
    return (f["x"] + 0.5) * sc - 0.5, (f["y"] + 0.5) * sc - 0.5


@functools.lru_cache(maxsize=None)
def map_points(n: int = 1100) -> np.ndarray:
    """Finite points in front of the camera (z in [1, 5]); a map of M points takes the first M."""
    rng = np.random.default_rng(900)
    z = rng.uniform(1.0, 5.0, n)
    return np.stack([rng.uniform(-1, 1, n) * z, rng.uniform(-0.7, 0.7, n) * z, z], axis=1)


def consistent_geometry(frame: dict, match: np.ndarray, M: int, seed: int) -> tuple[dict, np.ndarray]:
    """Keypoint positions and map points that agree under the identity pose, for a given set of
    matches (which depend on the descriptors alone): map point m projects to a level-0 pixel, and
    every keypoint matched to m sits on the pixel of its level nearest to it (exact on level 0), so
    the solve behind the matcher sees a consistent scene.  Returns (frame with new records, xyz)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, _ = intrinsics()
    top_w, top_h = LEVEL_WH[-1]
    px = rng.integers(2, 4 * top_w - 2, max(M, 1)).astype(np.float64)
    py = rng.integers(2, 4 * top_h - 2, max(M, 1)).astype(np.float64)
    z = rng.uniform(1.0, 5.0, max(M, 1))
    xyz = np.stack([(px - cx) * z / fx, (py - cy) * z / fy, z], axis=1)[:M]
    kps = frame["kps"].copy()
    j = np.nonzero(match >= 0)[0]
    sc = np.left_shift(1, LEVEL_OF[j]).astype(np.float64)
    x = np.rint((px[match[j]] + 0.5) / sc - 0.5).astype(np.uint32)
    y = np.rint((py[match[j]] + 0.5) / sc - 0.5).astype(np.uint32)
    kps[j, 0] = x | (y << 16)
    return dict(frame, kps=kps), xyz


# -- boundary variants -----------------------------------------------------------------------------
Variant = namedtuple("Variant", "vid bd sd n_second accept")


def _accepts(c, bd: int, sd: int) -> bool:
    return bd <= c.max_hamming and 100 * bd < c.ratio_pct * sd


def boundary_variants(c=None) -> list:
    """(bd, sd) on the ratio line 100 bd = ratio_pct sd with both neighbours, the max_hamming edge,
    distances 0 and 256, exact duplicates and equal-distance ties.  ``n_second`` trains share sd."""
    c = c or cfg()
    g = math.gcd(100, c.ratio_pct)
    out = []
    t = 1
    while 100 * t // g <= 256:
        bd, sd = c.ratio_pct * t // g, 100 * t // g
        out.append(Variant(f"eq{t}", bd, sd, 1, False))
        out.append(Variant(f"eq{t}-bd", bd - 1, sd, 1, _accepts(c, bd - 1, sd)))
        out.append(Variant(f"eq{t}-sd", bd, sd - 1, 1, False))
        t += 1
    mh = c.max_hamming
    out += [Variant("mh", mh, 256, 1, True), Variant("mh+1", mh + 1, 256, 1, False),
            Variant("zero-single", 0, 256, 1, True), Variant("zero-twice", 0, 0, 1, False),
            Variant("far", 256, 256, 1, False),
            Variant("tie2-1", 1, 1, 1, False), Variant(f"tie2-{mh}", mh, mh, 1, False),
            Variant("tie3", 12, 40, 3, True)]
    for v in out:
        assert 0 <= v.bd <= v.sd <= 256 and v.accept == (_accepts(c, v.bd, v.sd) and v.bd < 256)
    return out


@functools.lru_cache(maxsize=None)
def variant_descs(vid: str, bd: int, sd: int, n_second: int) -> dict:
    """The designed query, its best and second trains (distinct unless bd = sd in {0, 256}), the
    anchor and random queries, and one extra accepted pair for the duplicate case."""
    rng = np.random.default_rng(1000 * bd + sd + 100000 * n_second)
    q = random_desc(rng, 1)[0]
    best = flipped(rng, q, bd)
    seconds = []
    while len(seconds) < n_second:
        s = flipped(rng, q, sd)
        if sd in (0, 256) or not any(np.array_equal(s, o) for o in [best] + seconds):
            seconds.append(s)
    rnd = random_desc(rng, 1)[0]
    extra = flipped(rng, complement(q), 20)   # 236 bits from q: a train of its own, 20 from the fillers
    return {"q": q, "best": best, "seconds": seconds, "random": rnd, "extra": extra}


def boundary_trains(v: Variant, n: int, a: int, b: int) -> np.ndarray:
    """``n`` trains: the best at ``a``, the second at ``b``, further trains at the second's distance
    (tie3) on the first free positions after 2, the duplicate case's extra train after those, and the
    complement of the query everywhere else."""
    d = variant_descs(*v[:4])
    tr = np.tile(complement(d["q"]), (n, 1))
    free = [i for i in range(2, n) if i not in (a, b)]
    tr[a], tr[b] = d["best"], d["seconds"][0]
    for s in d["seconds"][1:]:
        tr[free.pop(0)] = s
    if v.vid == "zero-twice":
        tr[free.pop(0)] = d["extra"]
    return tr


# designed query at the last level's first slot (thread 185 of the last, partial block), the anchor
# and the random query at 0 and 1, the duplicate case's accepted query at 2
Q_DESIGNED, Q_ANCHOR, Q_RANDOM, Q_EXTRA = KOFF[2], 0, 1, 2


@functools.lru_cache(maxsize=None)
def boundary_frame(v: Variant) -> dict:
    d = variant_descs(*v[:4])
    rng = np.random.default_rng(31)
    desc = np.tile(d["best"], (K, 1))            # past the counts: copies of the best train
    desc[Q_DESIGNED], desc[Q_ANCHOR], desc[Q_RANDOM] = d["q"], d["best"], d["random"]
    kcount = [2, 0, 1]
    if v.vid == "zero-twice":
        desc[Q_EXTRA], kcount = d["extra"], [3, 0, 1]
    return make_frame(random_records(rng), kcount, desc)


def position_pairs(n: int, extra=()) -> list:
    pos = sorted({p for p in (0, 1, n - 2, n - 1) + tuple(extra) if 0 <= p < n})
    return [(a, b) for a in pos for b in pos if a != b]


CHUNK_POSITIONS = (RL_CHUNK - 2, RL_CHUNK - 1, RL_CHUNK, RL_CHUNK + 1, 2 * RL_CHUNK - 1, 2 * RL_CHUNK)


def designed_match(v: Variant, a: int, b: int) -> int:
    """What the designed query must get: the best train's index when accepted, else -1."""
    return a if v.accept else -1


def reloc_boundary_cases(c=None, sizes=(513, 1025)):
    """Every variant x map size x ordered (best, second) position pair from {0, 1, M-2, M-1} and the
    LDS chunk edges.  Yields dicts: id, variant, frame (one object per variant), map_desc, a, b."""
    for v in boundary_variants(c):
        fr = boundary_frame(v)
        for M in sizes:
            for a, b in position_pairs(M, CHUNK_POSITIONS):
                yield {"id": f"{v.vid}-M{M}-b{a}-s{b}", "variant": v, "frame": fr, "map_desc": boundary_trains(v, M, a, b),
                       "a": a, "b": b}


# -- votes: boundary cases -------------------------------------------------------------------------
VOTE_S = 256


def landmark_frame(desc: np.ndarray, seed: int, tail: np.ndarray | None = None) -> dict:
    """A frame whose stereo landmarks are exactly ``desc`` in order: the first len(desc) keypoints of
    level 0 are valid with a disparity, everything behind them (``tail`` descriptors, default copies of
    the first) is past the count and has a disparity too."""
    n = len(desc)
    assert n <= QUOTAS[0]
    rng = np.random.default_rng(seed)
    if tail is None:
        tail = desc[0] if n else np.zeros(8, np.uint32)
    full = np.tile(np.asarray(tail, dtype=np.uint32), (K, 1))
    full[:n] = desc
    return make_frame(random_records(rng), [n, 0, 0], full, rng.uniform(0.5, 60.0, K))


def vote_boundary_cases(c=None):
    """Per variant one query keyframe (designed, anchor, random: 3 landmarks; the duplicate case 4)
    and a candidate per ordered position pair from {0, 1, S-2, S-1}: S trains and, at index S, an
    exact copy of the designed query that the signature must not reach.  Yields (variant, query
    descriptors, [(a, b, candidate descriptors [S + 1][8])])."""
    for v in boundary_variants(c):
        d = variant_descs(*v[:4])
        q = [d["q"], d["best"], d["random"]] + ([d["extra"]] if v.vid == "zero-twice" else [])
        cands = [(a, b, np.concatenate([boundary_trains(v, VOTE_S, a, b), d["q"][None]])) for a, b in position_pairs(VOTE_S)]
        yield v, np.stack(q), cands


# -- tie-heavy fuzz ----------------------------------------------------------------------------------
def fuzz_map_case(M: int, seed: int = 0) -> dict:
    """Alphabet descriptors on both sides; every third query is a copy of a train with 0-2 more
    flips.  Counts: level 0 short, level 1 full, level 2 one short of its quota."""
    rng = np.random.default_rng(5000 + 10 * M + seed)
    words = _alphabet(rng)
    tr = alphabet_desc(rng, M, words)
    desc = alphabet_desc(rng, K, words)
    if M > 2:   # (one or two trains: the plain alphabet already lands on both sides of the rule)
        for k in range(0, K, 3):
            desc[k] = flipped(rng, tr[int(rng.integers(0, M))], int(rng.integers(0, 3)))
    return {"id": f"fuzz-M{M}", "frame": make_frame(random_records(rng), [300, QUOTAS[1], QUOTAS[2] - 1], desc),
            "map_desc": tr}


def fuzz_signature(n: int, seed: int, words: np.ndarray, pool: np.ndarray | None = None) -> np.ndarray:
    """``n`` alphabet landmarks; with a ``pool``, every other one is a pool entry with 0-2 more flips."""
    rng = np.random.default_rng(seed)
    d = alphabet_desc(rng, n, words)
    if pool is not None and len(pool):
        for k in range(0, n, 2):
            d[k] = flipped(rng, pool[int(rng.integers(0, len(pool)))], int(rng.integers(0, 3)))
    return d


def signature_sequence(S: int) -> list:
    """The frames stored one after the other into a 5-entry database with signature S: seven
    keyframes, so entries 0 and 1 are written twice — first with the most landmarks (2 S + 40), then
    with 0 and 1 — and the database ends up holding 0, 1, S - 1, S, S + 1 landmarks.  Every keyframe
    draws from one pool, so votes between any two of them are mixed."""
    rng = np.random.default_rng(7000 + S)
    words = _alphabet(rng)
    pool = alphabet_desc(rng, 48, words)
    counts = [2 * S + 40, 2 * S + 40, max(S - 1, 0), S, S + 1, 0, 1]
    return [landmark_frame(fuzz_signature(n, 7100 + 10 * S + i, words, pool), 7200 + 10 * S + i,
                           tail=pool[i % len(pool)]) for i, n in enumerate(counts)]


def window_entries(k0: int, n_kf: int, capk: int = DB_CAP, P: int = 1) -> list:
    """Entries a vote job over (k0, n_kf) reads, in output order: ((k0 + b / P) % capk) * P + b % P."""
    return [((k0 + b // P) % capk) * P + b % P for b in range(n_kf * P)]


# -- validity patterns of the compactors -------------------------------------------------------------
DEAD_DISPARITIES = (np.nan, np.inf, 0.0, -0.0, -3.5, -np.inf)


def _patterns() -> list:
    """(id, wanted mask over the keypoint positions, level counts)."""
    k = np.arange(K)
    rng = np.random.default_rng(8000)
    out = [("empty", np.zeros(K, bool), FULL), ("no-counts", np.ones(K, bool), (0, 0, 0)), ("everything", np.ones(K, bool), FULL)]
    out += [(f"single-{i}", k == i, FULL) for i in (0, 63, 64, 255, 256, K - 1)]
    out += [("even", k % 2 == 0, MIXED_A), ("odd", k % 2 == 1, MIXED_B),
            ("waves-on-off", (k // 64) % 2 == 0, MIXED_A), ("waves-off-on", (k // 64) % 2 == 1, MIXED_B),
            ("lanes-63-64", np.isin(k % 128, (63, 64)), FULL), ("passes-255-256", np.isin(k % 512, (255, 256)), FULL),
            ("random-half", rng.random(K) < 0.5, MIXED_A), ("random-sparse", rng.random(K) < 0.05, MIXED_B),
            ("random-dense", rng.random(K) < 0.95, MIXED_A)]
    return out


PATTERNS = _patterns()
TRIVIAL_PATTERNS = ("empty", "no-counts", "everything")


def pattern_survivors(pid: str) -> np.ndarray:
    _, want, kcount = next(p for p in PATTERNS if p[0] == pid)
    return want & valid_mask(kcount)


def store_pattern_case(pid: str) -> dict:
    """A frame for the keyframe store: the survivors have finite positive disparities, the other
    valid keypoints cycle through NaN, +inf, 0, -0, a negative and -inf, and the keypoints past the
    counts have positive disparities (only the count keeps them out)."""
    _, want, kcount = next(p for p in PATTERNS if p[0] == pid)
    rng = np.random.default_rng(8100 + [p[0] for p in PATTERNS].index(pid))
    valid = valid_mask(kcount)
    disp = rng.uniform(0.5, 60.0, K)
    dead = np.nonzero(valid & ~want)[0]
    disp[dead] = np.array(DEAD_DISPARITIES)[np.arange(dead.size) % len(DEAD_DISPARITIES)]
    return {"id": f"store-{pid}", "frame": make_frame(random_records(rng), kcount, random_desc(rng, K), disp),
            "survivors": want & valid}


def reloc_pattern_case(pid: str) -> dict:
    """The same patterns as accept flags of the relocalisation matcher: survivor number j is train j
    with 0-3 flipped bits (accepted, its own map point), the other valid keypoints are random (about
    128 bits from every train: rejected), the keypoints past the counts are exact copies of train 0.
    Records and map points agree under the identity pose."""
    _, want, kcount = next(p for p in PATTERNS if p[0] == pid)
    rng = np.random.default_rng(8200 + [p[0] for p in PATTERNS].index(pid))
    valid = valid_mask(kcount)
    on = np.nonzero(want & valid)[0]
    M = max(on.size, 2)
    tr = random_desc(rng, M)
    desc = random_desc(rng, K)
    desc[~valid] = tr[0]
    for j, k in enumerate(on):
        desc[k] = flipped(rng, tr[j], int(rng.integers(0, 4)))
    match = np.full(K, -1, dtype=np.int64)
    match[on] = np.arange(on.size)
    fr, xyz = consistent_geometry(make_frame(random_records(rng), kcount, desc), match, M, 8300)
    return {"id": f"reloc-{pid}", "frame": fr, "map_desc": tr, "map_xyz": xyz, "survivors": want & valid}


def verify_case() -> dict:
    """A candidate keyframe (the ``even`` store pattern: a few hundred landmarks) and a query frame
    for ``loop_verify``: the same pixel positions (so the two views agree under the identity pose),
    every count full, and descriptors that are the candidate's with 0-2 flipped bits where it has a
    landmark and random elsewhere."""
    cand = store_pattern_case("even")
    rng = np.random.default_rng(8400)
    desc = random_desc(rng, K)
    for k in np.nonzero(cand["survivors"])[0]:
        desc[k] = flipped(rng, cand["frame"]["desc"][k], int(rng.integers(0, 3)))
    return {"id": "verify-even", "candidate": cand["frame"], "query": make_frame(cand["frame"]["kps"], FULL, desc)}
