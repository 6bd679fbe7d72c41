// k_sd_sgm.hip — semi-global aggregation for the dense stereo matcher (rule 3a of
// thor_slam_amd/stereo_depth.py; DESIGN.md §6c "Semi-global aggregation"): up to four paths over
// the box-aggregated volume A, their sum S, and the winners of rules 4-6 from S (rule 7's parabola
// from A).  A path crosses the bands of k_sd_match, so the volume lives in device memory here: A
// and S, u16 [n][H][W][pitch] with d contiguous and pitch = D rounded up to 4 (a pixel's cell is
// 8-byte aligned; the pad cells are never read as values).
//
//   k_sd_match<true>  (k_stereo_depth.hip) writes A.
//   k_sgm_path<NV>    one wave per line (a row for the horizontal paths, a column for the vertical
//                     ones), four lines per block, lanes over d: lane l holds d = l NV .. l NV + NV - 1
//                     (NV = 1, 2, 4 for D <= 64, 128, 256), so the d - 1 / d + 1 terms are register
//                     neighbours but for one value from each adjacent lane, and min_k L_r(q, k) is
//                     a register minimum plus a 6-step __shfl_xor butterfly.  A step depends on the
//                     step before; the loads of A and S for SGM_PF steps ahead are in flight in a
//                     register ring while it runs.  The first enabled path stores S, the others add.
//   k_sgm_winners     one wave per (frame, row), 64 columns a step: the step's S cells come in with
//                     coalesced loads and go to an LDS tile (row pitch padded by one word: a lane
//                     per column reads without bank conflicts), each lane scans its column's d for
//                     the left winner (the rules and tie-breaks of k_sd_match; the sub-pixel parabola
//                     reads A at the winner) and sends (S << 8 | d) to the right pixel's slot of an
//                     LDS ring with atomicMin; the ring is written out as in k_sd_match.
//                     out: disp32, wl, wr for k_sd_finish.
#include "tslam_common.h"

#define SGM_PF 8                  // steps of A / S in flight ahead of the recurrence
#define SGM_LINES 4               // lines (waves) per block
#define SGM_BIG (1 << 20)         // above every L + P (<= 6000), far from overflow
#define SGM_TILE 64               // columns per step of k_sgm_winners
#define SGM_RING 512              // right-winner ring columns (>= SGM_TILE + 255)
#define SGM_WBIG (1 << 30)        // rule 4's "no second minimum"

static_assert(SGM_RING >= SGM_TILE + 255 && (SGM_RING & (SGM_RING - 1)) == 0, "ring covers a step's right pixels");

struct SgmArgs {
    const uint16_t* vol;     // A [n][H][W][pitch]
    uint16_t* sum;           // S, the same layout
    int W, H, D, pitch, n;
    int p1, p2;
};

// NV u16 cells as one aligned load / store
template <int NV> struct SgmCell;
template <> struct SgmCell<1> { typedef uint16_t T; };
template <> struct SgmCell<2> { typedef uint32_t T; };
template <> struct SgmCell<4> { typedef uint2 T; };

__device__ __forceinline__ void sgm_unpack(uint16_t c, int (&v)[1]) { v[0] = c; }
__device__ __forceinline__ void sgm_unpack(uint32_t c, int (&v)[2]) {
    v[0] = (int)(c & 0xFFFFu);
    v[1] = (int)(c >> 16);
}
__device__ __forceinline__ void sgm_unpack(uint2 c, int (&v)[4]) {
    v[0] = (int)(c.x & 0xFFFFu);
    v[1] = (int)(c.x >> 16);
    v[2] = (int)(c.y & 0xFFFFu);
    v[3] = (int)(c.y >> 16);
}
__device__ __forceinline__ void sgm_pack(const int (&v)[1], uint16_t& c) { c = (uint16_t)v[0]; }
__device__ __forceinline__ void sgm_pack(const int (&v)[2], uint32_t& c) { c = (uint32_t)v[0] | ((uint32_t)v[1] << 16); }
__device__ __forceinline__ void sgm_pack(const int (&v)[4], uint2& c) {
    c = make_uint2((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16));
}

// dir 0: left -> right, 1: right -> left (lines = rows); 2: top -> bottom, 3: bottom -> top
// (lines = columns).  first: S = L (nothing to read); otherwise S += L.
template <int NV>
__global__ __launch_bounds__(64 * SGM_LINES) void k_sgm_path(SgmArgs g, int dir, int first) {
    typedef typename SgmCell<NV>::T Cell;
    const int lane = threadIdx.x & 63;
    const int horiz = dir < 2;
    const int per = horiz ? g.H : g.W;              // lines per frame
    const int line = blockIdx.x * SGM_LINES + (threadIdx.x >> 6);
    if (line >= g.n * per) return;                  // wave-uniform
    const int f = line / per, r = line - f * per;
    const int len = horiz ? g.W : g.H;
    const size_t px0 = (size_t)f * g.W * g.H + (horiz ? (size_t)r * g.W + (dir == 0 ? 0 : g.W - 1)
                                                      : (size_t)(dir == 2 ? 0 : g.H - 1) * g.W + r);
    const ptrdiff_t step = (ptrdiff_t)((dir & 1) ? -1 : 1) * (horiz ? 1 : g.W) * g.pitch;   // cells between pixels
    const bool active = lane * NV < g.pitch;        // the lane has cells of the pixel (all NV or none)
    const size_t off0 = px0 * g.pitch + (active ? lane * NV : 0);
    const Cell* ap = reinterpret_cast<const Cell*>(g.vol + off0);
    Cell* sp = reinterpret_cast<Cell*>(g.sum + off0);
    const ptrdiff_t cstep = step / NV;              // pitch is a multiple of 4, so of NV
    bool valid[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) valid[j] = lane * NV + j < g.D;

    Cell abuf[SGM_PF], sbuf[SGM_PF];
#pragma unroll
    for (int k = 0; k < SGM_PF; ++k) {
        abuf[k] = Cell{};
        sbuf[k] = Cell{};
        if (k < len && active) {
            abuf[k] = ap[k * cstep];
            if (!first) sbuf[k] = sp[k * cstep];
        }
    }
    int Lp[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) Lp[j] = SGM_BIG;

    for (int i0 = 0; i0 < len; i0 += SGM_PF) {
#pragma unroll
        for (int k = 0; k < SGM_PF; ++k) {
            const int i = i0 + k;
            if (i >= len) break;                    // wave-uniform
            int A[NV], S[NV];
            sgm_unpack(abuf[k], A);
            sgm_unpack(sbuf[k], S);
            if (i + SGM_PF < len && active) {       // the slot's next tenant
                abuf[k] = ap[(ptrdiff_t)(i + SGM_PF) * cstep];
                if (!first) sbuf[k] = sp[(ptrdiff_t)(i + SGM_PF) * cstep];
            }
            int Ln[NV];
            if (i == 0) {
#pragma unroll
                for (int j = 0; j < NV; ++j) Ln[j] = valid[j] ? A[j] : SGM_BIG;
            } else {
                int M = Lp[0];
#pragma unroll
                for (int j = 1; j < NV; ++j) M = min(M, Lp[j]);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) M = min(M, __shfl_xor(M, o));
                int lo = __shfl_up(Lp[NV - 1], 1), hi = __shfl_down(Lp[0], 1);
                lo = lane == 0 ? SGM_BIG : lo;      // d - 1 < 0
                hi = lane == 63 ? SGM_BIG : hi;     // d + 1 > 255; below that the neighbour holds SGM_BIG
                const int far = M + g.p2;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const int dn = j ? Lp[j - 1] : lo, up = j < NV - 1 ? Lp[j + 1] : hi;
                    const int t = min(min(Lp[j], min(dn, up) + g.p1), far) - M;
                    Ln[j] = valid[j] ? A[j] + t : SGM_BIG;
                }
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                S[j] = valid[j] ? S[j] + Ln[j] : 0;
                Lp[j] = Ln[j];
            }
            if (active) {
                Cell c;
                sgm_pack(S, c);
                sp[(ptrdiff_t)i * cstep] = c;
            }
        }
    }
}

static inline __host__ __device__ int sgm_tile_pitch(int pitch) { return pitch / 2 + 1; }   // words; odd
static inline __host__ __device__ size_t sgm_win_lds(int pitch) { return ((size_t)SGM_TILE * sgm_tile_pitch(pitch) + SGM_RING) * 4; }

__global__ __launch_bounds__(64) void k_sgm_winners(SgmArgs g, int uniq, uint16_t* disp, uint8_t* wl, uint8_t* wr) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sgm_lds[];
    const int W = g.W, H = g.H, D = g.D, hw = g.pitch / 2, tp = sgm_tile_pitch(g.pitch);
    uint32_t* tile = sgm_lds;                       // [SGM_TILE][tp]: two d per word
    uint32_t* rb = sgm_lds + SGM_TILE * tp;         // [SGM_RING]
    const int tid = threadIdx.x;
    const int f = blockIdx.x / H, y = blockIdx.x - f * H;
    const size_t row = ((size_t)f * H + y) * W;
    for (int i = tid; i < SGM_RING; i += 64) rb[i] = 0xFFFFFFFFu;
    int flushed = 0;   // right pixels [0, flushed) of the row are written out
    for (int x0 = 0; x0 < W; x0 += SGM_TILE) {
        __syncthreads();                            // the previous step's scan / flush is done
        const int npx = min(SGM_TILE, W - x0);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(g.sum + (row + x0) * g.pitch);
        for (int i = tid; i < npx * hw; i += 64) {
            const int c = i / hw;
            tile[c * tp + (i - c * hw)] = src[i];
        }
        __syncthreads();
        const int x = x0 + tid;
        if (x < W) {
            // the left winner while d ascends, as in k_sd_match (its parabola neighbours come from A below)
            int best = SGM_WBIG, bd = -4, m2 = SGM_WBIG, q1 = SGM_WBIG, q2 = SGM_WBIG;
            const uint32_t* col = tile + tid * tp;
            for (int d = 0; d < D; ++d) {
                const int S = (int)((col[d >> 1] >> (16 * (d & 1))) & 0xFFFFu);
                const bool nb = S < best, right = d == bd + 1;
                m2 = nb ? q2 : (right ? m2 : min(m2, S));
                bd = nb ? d : bd;
                best = nb ? S : best;
                q2 = q1;
                q1 = min(q1, S);
                // right winner of pixel (y, x - d): smallest d among the minima
                if (x - d >= 0) atomicMin(&rb[(x - d) & (SGM_RING - 1)], ((uint32_t)S << 8) | (uint32_t)d);
            }
            const int d1 = bd, m1 = best;
            bool ok = d1 >= 1 && x - d1 >= 0;
            if (m2 != SGM_WBIG) ok = ok && m1 * 100 <= m2 * (100 - uniq);
            // rule 3a's sub-pixel step: the parabola through A, not S, at d1 (the penalties flatten S
            // around its minimum); d1 need not be A's minimum, so the offset is clamped
            int off = 0;
            if (d1 >= 1 && d1 <= D - 2) {
                const uint16_t* av = g.vol + (row + x) * g.pitch + d1;
                const int a0 = av[-1], a1 = av[0], a2 = av[1];
                const int den = a0 - 2 * a1 + a2;
                if (den > 0) {   // true floor of (32 (a0 - a2) + den) / (2 den)
                    const int num = 32 * (a0 - a2) + den, dn = 2 * den;
                    int q = num / dn;
                    if (num % dn != 0 && num < 0) --q;
                    off = min(max(q, -16), 16);
                }
            }
            disp[row + x] = ok ? (uint16_t)(32 * d1 + off) : (uint16_t)0;
            wl[row + x] = (uint8_t)d1;
        }
        __syncthreads();   // every candidate of this step is in the ring
        // right pixels left of the next step's span are final
        const bool last = x0 + SGM_TILE >= W;
        const int upto = last ? W : max(x0 + SGM_TILE - (D - 1), 0);
        for (int xr = flushed + tid; xr < upto; xr += 64) {
            uint32_t* e = rb + (xr & (SGM_RING - 1));
            wr[row + xr] = (uint8_t)(*e & 0xFFu);
            *e = 0xFFFFFFFFu;
        }
        if (upto > flushed) flushed = upto;
    }
}

template <int NV>
static void sgm_launch_paths(const SgmArgs& g, int paths, hipStream_t st) {
    int first = 1;
    for (int dir = 0; dir < 4; ++dir) {
        if (!(paths >> dir & 1)) continue;
        const int lines = g.n * (dir < 2 ? g.H : g.W);
        hipLaunchKernelGGL(k_sgm_path<NV>, dim3((unsigned)((lines + SGM_LINES - 1) / SGM_LINES)), dim3(64 * SGM_LINES), 0, st, g,
                           dir, first);
        first = 0;
    }
}

hipError_t launch_stereo_depth_sgm(const StereoDepthArgs& s, const StereoSgmArgs& q, hipStream_t st) {
    if (s.n <= 0) return hipSuccess;
    SgmArgs g;
    g.vol = q.vol;
    g.sum = q.sum;
    g.W = s.W;
    g.H = s.H;
    g.D = s.n_disp;
    g.pitch = sd_sgm_pitch(s.n_disp);
    g.n = s.n;
    g.p1 = q.p1;
    g.p2 = q.p2;
    hipError_t e = launch_sd_volume(s, q.vol, g.pitch, st);
    if (e != hipSuccess) return e;
    if (g.D <= 64) sgm_launch_paths<1>(g, q.paths, st);
    else if (g.D <= 128) sgm_launch_paths<2>(g, q.paths, st);
    else sgm_launch_paths<4>(g, q.paths, st);
    hipLaunchKernelGGL(k_sgm_winners, dim3((unsigned)(g.n * g.H)), dim3(64), sgm_win_lds(g.pitch), st, g, s.uniqueness, s.disp32,
                       s.win_left, s.win_right);
    e = hipGetLastError();
    return e != hipSuccess ? e : launch_sd_finish(s, st);
}
