// k_tsdf_dynamic.hip — dynamic objects kept out of the dense map: the free-space depth mask
// (tslam_tsdf_dynamic).  Spec and CPU restatement: thor_slam_amd/dense_dynamic.py (steps 1-6; every
// f64 operation below is one of its written operations, in its order; -ffp-contract=off keeps them
// unfused).
//
//   k_dynamic_poses     per frame: world_T_cam's rotation rows, the centre and the use flag
//                       (k_render_poses' table), and the frame's stats slot cleared.
//   k_dynamic_classify  one thread per pixel, a wave per 64 consecutive columns of a row, a block of
//                       four rows.  The pose entry and the window record are read with uniform loads;
//                       the pixel's depth is looked up as k_tsdf_integrate looks it up and written
//                       to the output image as it is; its point's voxel is gathered once (tsdf,
//                       weight, and the free-space layer's word while that layer exists: a
//                       settled voxel is no candidate, thor_slam_amd/dense_freespace.py).  The wave's candidates are one ballot, written as one word by one
//                       lane, with the ballot of its valid pixels beside it; bits past the last
//                       column are 0.  (Counting here, two atomics per wave on a frame's two
//                       counters, made this kernel 1.03 ms for 64 frames of 640 x 400; the words
//                       are counted by k_dynamic_apply instead.)
//   k_dynamic_apply     a block per tile of 16 rows x 8 words (512 columns).  The candidate words of
//                       the tile, with a halo of 2 * open_radius + dilate_radius rows and one word on
//                       each side, go through erosion, dilation and dilation in LDS: horizontally
//                       AND / OR over the shifts -r..r of a word with the carries of its neighbours,
//                       vertically AND / OR over rows.  What lies outside the image is 0 in every
//                       step.  Then the tile's mask bytes are written (eight at a time where the
//                       address allows), masked depth pixels are zeroed, and the valid pixels among
//                       them counted.  The tile's own words give its valid pixels and candidates
//                       (pop counts); the three counts go through LDS to one atomic each per block.
//
// The counts are integer atomics (order-independent).  Nothing waits, and every pixel of every slot
// of the call is written.
#include "tslam_common.h"

#define DYN_ROWS 16                                                   // rows of a tile
#define DYN_WORDS 8                                                   // words of a tile
#define DYN_HALO (2 * DYNAMIC_MAX_OPEN + DYNAMIC_MAX_DILATE)          // rows above and below, at most
#define DYN_LROWS (DYN_ROWS + 2 * DYN_HALO)
#define DYN_LWORDS (DYN_WORDS + 2)

__global__ void k_dynamic_poses(BatchCtx c, int pair, int f0, const double* host_wTc, int n, double* out, int32_t* stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double use = 1.0;
    const double* T = call_pose(c, pair, f0, host_wTc, i, &use);
    double* q = out + (size_t)i * TSDF_POSE;
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) q[3 * r + k] = T[4 * r + k];
        q[9 + r] = T[4 * r + 3];
    }
    q[12] = use;
    int32_t* s = stats + (size_t)i * DYNAMIC_STATS;
    s[0] = use != 0.0 ? 0 : 1;
    s[1] = s[2] = s[3] = 0;
}

__global__ __launch_bounds__(256) void k_dynamic_classify(TsdfDynamicArgs a, int words) {
    const int f = blockIdx.z;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int y = blockIdx.y * 4 + wave;
    if (y >= a.H) return;   // the whole wave (no barrier below)
    const int x = blockIdx.x * 64 + lane;
    const double* __restrict__ q = a.poses + (size_t)f * TSDF_POSE;   // uniform: scalar loads
    const bool used = q[12] != 0.0;
    bool valid = false, cand = false;
    if (x < a.W) {
        // 1: the lookup
        int ix = x, iy = y;
        if (a.map) {
            const int32_t* mp = a.map + ((size_t)y * a.W + x) * 2;
            ix = min(max((mp[0] + 16) >> 5, 0), a.W - 1);
            iy = min(max((mp[1] + 16) >> 5, 0), a.H - 1);
        }
        const uint16_t mm = reinterpret_cast<const uint16_t*>(a.depth + (size_t)f * a.stride)[(size_t)iy * a.W + ix];
        a.out_depth[((size_t)f * a.H + y) * a.W + x] = mm;   // k_dynamic_apply zeroes what the mask covers
        const double D = (double)mm * 0.001;
        valid = used && D > 0.0 && D <= a.max_dist;
        if (valid) {
            double ox = a.ox, oy = a.oy, oz = a.oz;
            if (a.win) {   // the rolling window: the corner from the cumulative shift (three uniform loads)
                ox = a.ox + a.s * (double)a.win->shift[0];
                oy = a.oy + a.s * (double)a.win->shift[1];
                oz = a.oz + a.s * (double)a.win->shift[2];
            }
            // 2: the point in the volume's frame
            const double dc0 = ((double)x - a.cx) / a.fx, dc1 = ((double)y - a.cy) / a.fy;
            const double pc0 = D * dc0, pc1 = D * dc1;
            const double p0 = ((q[0] * pc0 + q[1] * pc1) + q[2] * D) + q[9];
            const double p1 = ((q[3] * pc0 + q[4] * pc1) + q[5] * D) + q[10];
            const double p2 = ((q[6] * pc0 + q[7] * pc1) + q[8] * D) + q[11];
            // 3: its voxel; in floating point before any conversion: a NaN is outside
            const double g0 = floor((p0 - ox) / a.s), g1 = floor((p1 - oy) / a.s), g2 = floor((p2 - oz) / a.s);
            if (g0 >= 0.0 && g0 <= (double)(a.nx - 1) && g1 >= 0.0 && g1 <= (double)(a.ny - 1) && g2 >= 0.0 &&
                g2 <= (double)(a.nz - 1)) {
                const size_t v = ((size_t)(int)g2 * a.ny + (size_t)(int)g1) * a.nx + (size_t)(int)g0;
                const float w = a.weight[v], t = a.tsdf[v];
                const uint32_t fs = a.layer ? a.layer[v] : 0u;   // the free-space word beside them (uniform: null when off)
                // 4: seen free, reliably, and not released to the map
                cand = ((double)w >= a.min_free_weight) & ((double)t >= a.thr) & ((fs & FREESPACE_SETTLED) == 0);
            }
        }
    }
    const uint64_t mv = __ballot(valid), mc = __ballot(cand);
    if (lane == 0) {   // the pair of words of (row, 64 columns): candidates, valid pixels (counted by k_dynamic_apply)
        uint64_t* w = a.bits + (((size_t)f * a.H + y) * words + blockIdx.x) * 2;
        w[0] = mc;
        w[1] = mv;
    }
}

// bit x of the result = AND (ERODE) or OR over bits x - r .. x + r of the row; `lo` holds the 64
// columns before w's, `hi` the 64 after (bit 0 = the first column of a word)
template <bool ERODE>
__device__ __forceinline__ uint64_t dyn_row_op(uint64_t lo, uint64_t w, uint64_t hi, int r) {
    uint64_t v = w;
    for (int k = 1; k <= r; ++k) {
        const uint64_t left = (w << k) | (lo >> (64 - k)), right = (w >> k) | (hi << (64 - k));
        v = ERODE ? (v & left & right) : (v | left | right);
    }
    return v;
}

// One separable step over the tile's rows in LDS: horizontally src -> tmp, vertically tmp -> dst
// (dst may be src).  Rows and words the tile does not hold count as 0; `keep` (dilation into the
// next step's input) zeroes what lies outside the image.
template <bool ERODE>
__device__ __forceinline__ void dyn_step(uint64_t (*src)[DYN_LWORDS], uint64_t (*tmp)[DYN_LWORDS], uint64_t (*dst)[DYN_LWORDS],
                                         int rows, int r, bool keep, int y_first, int H, int word_first, int W) {
    if (r == 0) {
        if (src != dst)
            for (int i = threadIdx.x; i < rows * DYN_LWORDS; i += blockDim.x) dst[i / DYN_LWORDS][i % DYN_LWORDS] = src[i / DYN_LWORDS][i % DYN_LWORDS];
        __syncthreads();
        return;
    }
    for (int i = threadIdx.x; i < rows * DYN_LWORDS; i += blockDim.x) {
        const int row = i / DYN_LWORDS, c = i % DYN_LWORDS;
        const uint64_t lo = c > 0 ? src[row][c - 1] : 0, hi = c + 1 < DYN_LWORDS ? src[row][c + 1] : 0;
        tmp[row][c] = dyn_row_op<ERODE>(lo, src[row][c], hi, r);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * DYN_LWORDS; i += blockDim.x) {
        const int row = i / DYN_LWORDS, c = i % DYN_LWORDS;
        uint64_t v = tmp[row][c];
        for (int k = 1; k <= r; ++k) {
            const uint64_t up = row - k >= 0 ? tmp[row - k][c] : 0, down = row + k < rows ? tmp[row + k][c] : 0;
            v = ERODE ? (v & up & down) : (v | up | down);
        }
        if (keep) {   // 5: everything outside the image counts as 0 in the next step
            const int y = y_first + row;
            const int64_t x0 = ((int64_t)word_first + c) * 64;   // the word's first column (the left halo: -64)
            uint64_t in = 0;
            if (y >= 0 && y < H && x0 >= 0 && x0 < W) in = W - x0 >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << (W - x0)) - 1);
            v &= in;
        }
        dst[row][c] = v;   // its own element only: no thread reads dst in this pass
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_dynamic_apply(TsdfDynamicArgs a, int words) {
    __shared__ uint64_t s_a[DYN_LROWS][DYN_LWORDS];
    __shared__ uint64_t s_b[DYN_LROWS][DYN_LWORDS];
    __shared__ int s_count[3];   // valid pixels, candidates, valid pixels under the mask
    const int f = blockIdx.z;
    const int halo = 2 * a.open_radius + a.dilate_radius, rows = DYN_ROWS + 2 * halo;
    const int y_first = blockIdx.y * DYN_ROWS - halo, word_first = blockIdx.x * DYN_WORDS - 1;
    if (threadIdx.x < 3) s_count[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t* __restrict__ bits = a.bits + (size_t)f * a.H * words * 2;
    int n_valid = 0, n_cand = 0;
    for (int i = threadIdx.x; i < rows * DYN_LWORDS; i += blockDim.x) {
        const int row = i / DYN_LWORDS, c = i % DYN_LWORDS;
        const int y = y_first + row, w = word_first + c;
        uint64_t mc = 0;
        if (y >= 0 && y < a.H && w >= 0 && w < words) {
            const uint64_t* p = bits + ((size_t)y * words + w) * 2;
            mc = p[0];
            if (row >= halo && row < halo + DYN_ROWS && c >= 1 && c <= DYN_WORDS) {   // the tile's own words: counted here, once
                n_cand += __popcll(mc);
                n_valid += __popcll(p[1]);
            }
        }
        s_a[row][c] = mc;
    }
    if (n_valid) atomicAdd(&s_count[0], n_valid);
    if (n_cand) atomicAdd(&s_count[1], n_cand);
    __syncthreads();
    // 5: E = erosion, O = dilation of E, M = dilation of O
    dyn_step<true>(s_a, s_b, s_a, rows, a.open_radius, false, y_first, a.H, word_first, a.W);
    dyn_step<false>(s_a, s_b, s_a, rows, a.open_radius, true, y_first, a.H, word_first, a.W);
    dyn_step<false>(s_a, s_b, s_a, rows, a.dilate_radius, true, y_first, a.H, word_first, a.W);

    // 6: a thread per byte of the tile's words (8 columns)
    int under = 0;
    uint8_t* __restrict__ mask = a.out_mask + (size_t)f * a.H * a.W;
    uint16_t* __restrict__ depth = a.out_depth + (size_t)f * a.H * a.W;
    for (int i = threadIdx.x; i < DYN_ROWS * DYN_WORDS * 8; i += blockDim.x) {
        const int row = i / (DYN_WORDS * 8), b = i % (DYN_WORDS * 8);
        const int y = blockIdx.y * DYN_ROWS + row;
        const int x0 = (blockIdx.x * DYN_WORDS + b / 8) * 64 + (b % 8) * 8;
        if (y >= a.H || x0 >= a.W) continue;
        const uint32_t m = (uint32_t)(s_a[halo + row][1 + b / 8] >> ((b % 8) * 8)) & 0xffu;
        const size_t o = (size_t)y * a.W + x0;
        uint8_t* mp = mask + o;
        if (x0 + 8 <= a.W && (reinterpret_cast<uintptr_t>(mp) & 7) == 0) {
            // bit k of m into byte k: the eight copies of m, each masked to its own bit, then to 0 / 1
            const uint64_t spread = ((uint64_t)m * 0x0101010101010101ull) & 0x8040201008040201ull;
            *reinterpret_cast<uint64_t*>(mp) = ((spread + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
        } else {
            for (int k = 0; k < 8 && x0 + k < a.W; ++k) mp[k] = (uint8_t)((m >> k) & 1u);
        }
        for (uint32_t left = m; left; left &= left - 1) {
            const int k = __builtin_ctz(left);
            const double D = (double)depth[o + k] * 0.001;   // the looked-up value, as k_dynamic_classify left it
            under += (D > 0.0 && D <= a.max_dist) ? 1 : 0;
            depth[o + k] = 0;
        }
    }
    if (under) atomicAdd(&s_count[2], under);
    __syncthreads();
    if (threadIdx.x < 3 && s_count[threadIdx.x]) atomicAdd(&a.stats[(size_t)f * DYNAMIC_STATS + 1 + threadIdx.x], s_count[threadIdx.x]);
}

void launch_tsdf_dynamic(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfDynamicArgs& a,
                         double* poses, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(k_dynamic_poses, dim3((a.n + 63) / 64), dim3(64), 0, s, c, pair, f0, host_wTc_dev, a.n, poses, a.stats);
    TsdfDynamicArgs b = a;
    b.poses = poses;
    const int words = (a.W + 63) / 64;
    hipLaunchKernelGGL(k_dynamic_classify, dim3((unsigned)words, (unsigned)((a.H + 3) / 4), (unsigned)a.n), dim3(256), 0, s, b, words);
    hipLaunchKernelGGL(k_dynamic_apply, dim3((unsigned)((words + DYN_WORDS - 1) / DYN_WORDS), (unsigned)((a.H + DYN_ROWS - 1) / DYN_ROWS),
                                             (unsigned)a.n),
                       dim3(256), 0, s, b, words);
}
