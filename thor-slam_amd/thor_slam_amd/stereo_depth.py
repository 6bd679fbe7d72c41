"""Dense stereo depth on the device: a depth image from a rectified stereo pair, so that a stereo
rig feeds the TSDF volume the way an RGB-D camera does.  The reference needs no such step because
its cameras compute stereo depth themselves (DepthAI on-device StereoDepth)
and hand nvblox a depth image.  The rules below are the spec, in integers so that the device
(``csrc/k_stereo_depth.hip``) is bit-exact with an independent NumPy restatement
(``tests/ref_stereo_depth.py``; the product does not import it).

Inputs: the rectified level-0 images L, R (u8 [H][W]) of one pair; fxb = fx * baseline of the pair.
Parameters: n_disp D (candidates 0..D-1, 4..256), uniqueness u (0..99), lr_tol (px, >= 0).

1. Census 7x7 of L and R: 48 bits per pixel, a bit is 1 iff the neighbour is strictly less than
   the centre; neighbours outside the image read the replicated border pixel.
2. Cost C(d, y, x) = popcount(censusL(y, x) ^ censusR(y, x - d)) for x >= d, the constant 48 for
   x < d.
3. Aggregation A(d, y, x) = sum of C(d, ., .) over the 5x5 window centred on (y, x), window
   coordinates clamped to the image (replicated border of each d plane); A <= 1200.
3a. Semi-global aggregation (opt-in; ``csrc/k_sd_sgm.hip``, restated in ``tests/ref_stereo_sgm.py``).
   Parameters: penalties P1, P2 with 0 <= P1 <= P2 <= 2400 in units of A (defaults 100, 1200);
   ``paths``, a bit mask 1..15 (default 15): bit 1 left->right, r = (+1, 0); bit 2 right->left,
   r = (-1, 0); bit 4 top->bottom, r = (0, +1); bit 8 bottom->top, r = (0, -1).  For each enabled
   path r and pixel p = (x, y), with q = p - r: if q is outside the image, L_r(p, d) = A(d, p);
   otherwise, with M = min_k L_r(q, k),
   L_r(p, d) = A(d, p) + min(L_r(q, d), L_r(q, d-1) + P1, L_r(q, d+1) + P1, M + P2) - M,
   the terms with d-1 < 0 or d+1 > D-1 left out.  S(d, p) = the sum of L_r(p, d) over the enabled
   paths.  Rules 4 to 6 and 8 apply unchanged with S in place of A.  Rule 7 takes its three values
   from A at S's winner: c0 = A(d1 - 1, y, x), m1 = A(d1, y, x), c2 = A(d1 + 1, y, x), and clamps off
   to [-16, 16] (d1 need not minimise A).  The penalties cap a path's d1 +- 1 neighbours at its
   minimum + P1, so a parabola through S is flatter than through A and biases the offset: on the
   clean 320x240 scene (baseline 0.075, D = 32) the median relative depth error is 0.032 with rule 7
   on S against 0.016 on A, where the box matcher has 0.016.  L_r <= 1200 + P2 <= 3600 and
   S <= 4 (1200 + P2) <= 14400, so u16 holds both and the right winner's key (cost << 8 | d) fits
   32 bits.  With P1 = P2 = 0, L_r = A and S = n A: rules 4 to 6 are scale-invariant and d1 is A's
   winner, whose offset lies in [-16, 16] already, so the output is the box matcher's, bit for bit.
4. Left winner: d1 = the smallest d minimising A(d, y, x), m1 = that minimum, m2 = the minimum of A
   over all d with |d - d1| > 1 (2^30 if there is none).
5. Right winner, from the same volume: dR(y, xr) = the smallest d minimising A(d, y, xr + d) over d
   with xr + d < W.
6. A pixel is valid iff d1 >= 1, m1 * 100 <= m2 * (100 - u), x - d1 >= 0 and
   |dR(y, x - d1) - d1| <= lr_tol.
7. Sub-pixel in 1/32 px: if 1 <= d1 <= D - 2, with c0 = A(d1 - 1, y, x), c2 = A(d1 + 1, y, x) and
   den = c0 - 2 m1 + c2 > 0: off = floor((32 (c0 - c2) + den) / (2 den)) (a true floor, so
   off in [-16, 16]); otherwise off = 0.  disp32 = 32 d1 + off as u16, 0 where invalid.
8. Depth: mm = floor((fxb * 32000.0) / (double) disp32 + 0.5) (f64: one multiply, one divide, one
   add, in that order); depth = mm as u16, or 0 where the pixel is invalid or mm > 65535.

Post-filters (opt-in; ``csrc/k_sd_filter.hip``, restated in ``tests/ref_stereo_filter.py``).  Both
act on disp32 after rule 7, i.e. after the left-right check (u16, 0 = invalid, <= 8176), after the
box matcher and after rule 3a alike; rule 9 first, then rule 10; rule 8 is then computed from the
filtered disp32.

9. Median.  Parameter m in {0 (off), 3, 5, 7}.  A pixel with disp32 = 0 stays 0.  For a valid
   pixel, take the m x m window centred on it, window coordinates clamped to the image (a clamped
   position counts as often as it occurs), and let v_0 <= ... <= v_(n-1) be the non-zero values in
   it (n >= 1: the centre is one of them).  The output is v at index floor((n - 1) / 2), the lower
   median.  All outputs are computed from the unfiltered input.  The rule never changes which
   pixels are valid: a median that treats 0 as a value invents disparities across holes.
10. Speckle.  Parameters ``speckle_size`` s, 0 (off) .. 65535, and ``speckle_range`` r, 0 .. 8191
   in disp32 units (default 32 = 1 px).  Two 4-neighbours are linked iff both are non-zero and
   |a - b| <= r.  Components are the transitive closure of the links (the ends of a ramp may differ
   by far more than r).  Every pixel of a component with at most s pixels becomes 0.  The result
   depends on the partition alone, so every labelling algorithm gives the same bits.

Out of scope: 8 or 16 aggregation paths, 8-connected speckles, temporal, edge-preserving and
hole-filling filters, filtering depth rather than disparity, matching on a coarser pyramid level, a colour layer from the gray images; the engine integrates pair 0 only (the C ABI
takes any pair) and does not run on sharded rigs.
"""

from __future__ import annotations

CENSUS_RADIUS = 3      # 7x7 window, 48 bits
BOX_RADIUS = 2         # 5x5 aggregation
COST_OUTSIDE = 48      # C(d, y, x) for x < d
SUBPIXEL = 32          # disparity units per pixel
NO_SECOND_MINIMUM = 1 << 30

N_DISP_MIN, N_DISP_MAX = 4, 256
DEFAULT_UNIQUENESS = 10
DEFAULT_LR_TOL = 1

# rule 3a
SGM_P_MAX = 2400
SGM_DEFAULT_P1, SGM_DEFAULT_P2 = 100, 1200
SGM_PATH_LR, SGM_PATH_RL, SGM_PATH_TB, SGM_PATH_BT = 1, 2, 4, 8
SGM_PATHS_ALL = 15


# rules 9 and 10
MEDIAN_SIZES = (0, 3, 5, 7)
SPECKLE_SIZE_MAX = 65535
SPECKLE_RANGE_MAX = 8191
DEFAULT_SPECKLE_RANGE = 32


def check_filter_params(median: int, speckle_size: int, speckle_range: int = DEFAULT_SPECKLE_RANGE) -> None:
    if median not in MEDIAN_SIZES:
        raise ValueError(f"median must be one of {MEDIAN_SIZES}")
    if not 0 <= speckle_size <= SPECKLE_SIZE_MAX:
        raise ValueError(f"speckle_size must be in [0, {SPECKLE_SIZE_MAX}]")
    if not 0 <= speckle_range <= SPECKLE_RANGE_MAX:
        raise ValueError(f"speckle_range must be in [0, {SPECKLE_RANGE_MAX}]")


def check_params(n_disp: int, uniqueness: int, lr_tol: int) -> None:
    if n_disp != 0 and not N_DISP_MIN <= n_disp <= N_DISP_MAX:
        raise ValueError(f"n_disp must be 0 (the handle's max_disparity) or in [{N_DISP_MIN}, {N_DISP_MAX}]")
    if not 0 <= uniqueness <= 99:
        raise ValueError("uniqueness must be in [0, 99]")
    if lr_tol < 0:
        raise ValueError("lr_tol must be >= 0")


def check_sgm_params(p1: int, p2: int, paths: int = SGM_PATHS_ALL, chunk_frames: int = 0) -> None:
    if not 0 <= p1 <= p2 <= SGM_P_MAX:
        raise ValueError(f"SGM penalties must satisfy 0 <= p1 <= p2 <= {SGM_P_MAX}")
    if not 1 <= paths <= SGM_PATHS_ALL:
        raise ValueError(f"paths must be a bit mask in [1, {SGM_PATHS_ALL}]")
    if chunk_frames < 0:
        raise ValueError("chunk_frames must be >= 0")
