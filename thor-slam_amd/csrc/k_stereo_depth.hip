// k_stereo_depth.hip — dense stereo depth on the rectified level-0 images: census 7x7, Hamming
// cost, 5x5 box aggregation, winner-take-all with uniqueness, left-right check, sub-pixel
// disparity (1/32 px) and depth (u16 mm).  Spec: thor_slam_amd/stereo_depth.py; DESIGN.md §6c.
//
// The cost volume never leaves the CU.  Two kernels (design (b) of DESIGN.md §6c):
//
//   k_sd_match   one 256-thread block per (frame, band of SD_TH rows), walking the band's full width
//                in steps of SD_OUT columns.  Per step: the raw rows of both images (census + box
//                halo: 5 rows above and below, 5 columns left and right; coordinates clamped, i.e.
//                the replicated border) go to an LDS tile, the right image's census of the step's
//                whole disparity span is computed from it into LDS, the left census of a thread's
//                own column (SD_ROWS rows) stays in registers.  Then for each d, thread = column:
//                SD_ROWS Hamming costs (2 popcounts of the XOR), the vertical 5-sums of the band's
//                rows as a running sum, exchanged through LDS for the horizontal 5-sum.  The left
//                winner (minimum, excluded-neighbour second minimum, parabola neighbours) is
//                tracked in registers while d ascends; the right winner of pixel x - d is an LDS
//                minimum on the key (A << 8 | d) in a 512-column ring that is written out (u8) once
//                a column can get no more candidates.
//                out: disp32 u16 (0 = rejected by d1 >= 1 / uniqueness / x - d1 >= 0), the left
//                winner d1 u8 and the right winner dR u8.
//   k_sd_finish  per pixel: left-right check against dR(y, x - d1), disp32 zeroed where it fails,
//                depth = floor(fxb * 32000 / disp32 + 1/2) mm (f64: one multiply, one divide, one add).
#include "tslam_common.h"

#define SD_TH 8                  // output rows per band
#define SD_ROWS (SD_TH + 4)      // census rows a thread holds (box halo 2 above and below)
#define SD_RAW_ROWS (SD_TH + 10) // raw rows of the tile (census halo 3 more)
#define SD_BLOCK 256
#define SD_OUT (SD_BLOCK - 4)    // output columns per step (box halo 2 left and right)
#define SD_RING 512              // right-winner ring columns (>= SD_OUT + 255)
#define SD_BIG (1 << 30)

static_assert(SD_RING >= SD_OUT + 255 && (SD_RING & (SD_RING - 1)) == 0, "ring covers a step's right pixels");

// dynamic LDS: right census [SD_ROWS][rcols] (8 B), right-winner ring [SD_TH][SD_RING] (4 B), and a
// region shared by the raw tiles (census phase) and the vertical-sum exchange (disparity loop)
static inline __host__ __device__ int sd_rcols(int D) { return SD_BLOCK + D - 1; }
static inline __host__ __device__ int sd_raw_pitch_r(int D) { return (sd_rcols(D) + 6 + 3) & ~3; }
#define SD_RAW_PITCH_L ((SD_BLOCK + 6 + 3) & ~3)
static inline __host__ __device__ size_t sd_lds_bytes(int D) {
    const size_t cen = (size_t)SD_ROWS * sd_rcols(D) * 8, ring = (size_t)SD_TH * SD_RING * 4;
    const size_t raw = (size_t)SD_RAW_ROWS * (sd_raw_pitch_r(D) + SD_RAW_PITCH_L);
    const size_t xch = (size_t)2 * SD_BLOCK * 16;
    return cen + ring + ((raw > xch ? raw : xch) + 15) / 16 * 16;
}

// census of the pixel at tile position (row r, column c) = the tile's (r + 3, c + 3) centre: 48
// bits, 1 = neighbour < centre, 7 per tile row (the centre's own bit is 0 in both images, so it
// adds nothing to a Hamming distance).  The row loop stays rolled: unrolled, the 49 byte loads of
// every census of a thread are hoisted together and spill.
__device__ __forceinline__ uint2 sd_census(const uint8_t* t, int pitch, int r, int c) {
    const uint8_t* p = t + r * pitch + c;
    const uint32_t ctr = p[3 * pitch + 3];
    uint64_t w = 0;
#pragma unroll 1
    for (int j = 0; j < 7; ++j) {
        uint32_t rowbits = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) rowbits = (rowbits << 1) | (p[i] < ctr ? 1u : 0u);
        w = (w << 7) | rowbits;
        p += pitch;
    }
    return make_uint2((uint32_t)w, (uint32_t)(w >> 32));
}

struct SdArgs {
    const uint8_t* left;     // frame 0's rectified left / right level-0 image (dense rows, pitch W)
    const uint8_t* right;
    int64_t stride;          // bytes between frames (ring: between ring slots)
    int ring;                // 0: frame f at f * stride; else at ((first + f) % ring) * stride
    int64_t first;
    int W, H, D, n;
    int uniq, lr_tol;
    double fxb;
    uint16_t* disp;          // [n][H][W]
    uint16_t* depth;         // [n][H][W]
    uint8_t* wl;             // [n][H][W] left winner d1
    uint8_t* wr;             // [n][H][W] right winner dR
};

__device__ __forceinline__ size_t sd_frame_off(const SdArgs& a, int f) {
    return (size_t)(a.ring ? (a.first + f) % a.ring : (int64_t)f) * (size_t)a.stride;
}

// VOL: the semi-global matcher's first stage (k_sd_sgm.hip).  The same census, cost and box sums,
// but A(d, y, x) goes to device memory, u16 [n][H][W][pitch] with d contiguous, four d per 8-byte
// store, and no winner is tracked: the paths cross bands, so the winners come from their sums.
template <bool VOL>
__global__ __launch_bounds__(SD_BLOCK) void k_sd_match(SdArgs a, int nbands, uint16_t* vol, int pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sd_lds[];
    const int W = a.W, H = a.H, D = a.D;
    const int rcols = sd_rcols(D), pitch_r = sd_raw_pitch_r(D);
    uint2* cenR = reinterpret_cast<uint2*>(sd_lds);                                   // [SD_ROWS][rcols]
    uint32_t* rb = reinterpret_cast<uint32_t*>(sd_lds + (size_t)SD_ROWS * rcols * 8); // [SD_TH][SD_RING]
    uint8_t* shared = reinterpret_cast<uint8_t*>(rb + SD_TH * SD_RING);
    uint8_t* rawR = shared;                                   // [SD_RAW_ROWS][pitch_r]
    uint8_t* rawL = shared + (size_t)SD_RAW_ROWS * pitch_r;   // [SD_RAW_ROWS][SD_RAW_PITCH_L]
    uint4* xch = reinterpret_cast<uint4*>(shared);            // [2][SD_BLOCK] packed vertical sums

    const int tid = threadIdx.x;
    const int f = blockIdx.x / nbands, y0 = (blockIdx.x - f * nbands) * SD_TH;
    const size_t fo = sd_frame_off(a, f);
    const uint8_t* L = a.left + fo;
    const uint8_t* R = a.right + fo;
    const size_t out0 = (size_t)f * W * H;

    if constexpr (!VOL)
        for (int i = tid; i < SD_TH * SD_RING; i += SD_BLOCK) rb[i] = 0xFFFFFFFFu;
    int flushed = 0;   // right pixels [0, flushed) of the band are written out

    for (int xc = 0; xc < W; xc += SD_OUT) {
        const int base = xc - 2 - (D - 1);   // image column of cenR column 0
        __syncthreads();                      // the previous step's exchange / flush is done
        // raw tiles, clamped coordinates: rows y0 - 5 .., left columns xc - 5 .., right base - 3 ..
        for (int i = tid; i < SD_RAW_ROWS * SD_RAW_PITCH_L; i += SD_BLOCK) {
            const int r = i / SD_RAW_PITCH_L, c = i - r * SD_RAW_PITCH_L;
            const int y = min(max(y0 - 5 + r, 0), H - 1), x = min(max(xc - 5 + c, 0), W - 1);
            rawL[i] = L[(size_t)y * W + x];
        }
        for (int i = tid; i < SD_RAW_ROWS * pitch_r; i += SD_BLOCK) {
            const int r = i / pitch_r, c = i - r * pitch_r;
            const int y = min(max(y0 - 5 + r, 0), H - 1), x = min(max(base - 3 + c, 0), W - 1);
            rawR[i] = R[(size_t)y * W + x];
        }
        __syncthreads();
        // census.  Row slot r stands for image row clamp(y0 - 2 + r) and a column position for its
        // clamped column (the box window's replicated border is a border of the cost planes), so a
        // slot's census is taken at the clamped pixel's place in the tile.
        for (int i = tid; i < SD_ROWS * rcols; i += SD_BLOCK) {
            const int r = i / rcols, c = i - r * rcols, x = base + c;
            if (x < 0 || x >= W) continue;   // never read: cost 48 left of the image, no column right of it
            const int yy = min(max(y0 - 2 + r, 0), H - 1);
            cenR[i] = sd_census(rawR, pitch_r, yy - (y0 - 2), c);
        }
        const int p = xc - 2 + tid;              // this thread's column position
        const int cp = min(max(p, 0), W - 1);    // its column (xc - 2 <= cp <= xc + SD_BLOCK - 3)
        uint2 cL[SD_ROWS];
#pragma unroll
        for (int r = 0; r < SD_ROWS; ++r) {
            const int yy = min(max(y0 - 2 + r, 0), H - 1);
            cL[r] = sd_census(rawL, SD_RAW_PITCH_L, yy - (y0 - 2), cp - (xc - 2));
        }
        __syncthreads();   // census done: the raw tiles' region becomes the exchange buffer

        const bool outcol = tid >= 2 && tid < SD_BLOCK - 2 && p < W;   // then cp == p
        int best[SD_TH], bd[SD_TH], m2[SD_TH], c0[SD_TH], c2[SD_TH], p1[SD_TH], p2[SD_TH], prev[SD_TH];
#pragma unroll
        for (int k = 0; k < SD_TH; ++k) {
            best[k] = SD_BIG;
            bd[k] = -4;
            m2[k] = c0[k] = c2[k] = p1[k] = p2[k] = SD_BIG;
            prev[k] = 0;
        }
        uint32_t pk[VOL ? SD_TH : 1][2] = {};   // VOL: A of d & ~3 .. d of each row, packed
        uint16_t* vcol = VOL ? vol + (out0 + (size_t)y0 * W + cp) * (size_t)pitch : nullptr;
        const int t0 = max(tid - 2, 0), t1 = max(tid - 1, 0), t3 = min(tid + 1, SD_BLOCK - 1), t4 = min(tid + 2, SD_BLOCK - 1);
        for (int d = 0; d < D; ++d) {
            const int xr = cp - d;             // right column of this cost; xr - base >= 0 always
            const uint2* cr = cenR + (xr - base);
            int cost[SD_ROWS];
#pragma unroll
            for (int r = 0; r < SD_ROWS; ++r) {
                const uint2 q = cr[r * rcols];
                const int hd = __builtin_popcount(cL[r].x ^ q.x) + __builtin_popcount(cL[r].y ^ q.y);
                cost[r] = xr >= 0 ? hd : 48;
            }
            // vertical 5-sums of the band's rows (running sum), two rows per word
            int v[SD_TH];
            v[0] = cost[0] + cost[1] + cost[2] + cost[3] + cost[4];
#pragma unroll
            for (int k = 1; k < SD_TH; ++k) v[k] = v[k - 1] - cost[k - 1] + cost[k + 4];
            uint4* xb = xch + (d & 1) * SD_BLOCK;
            xb[tid] = make_uint4((uint32_t)v[0] | ((uint32_t)v[1] << 16), (uint32_t)v[2] | ((uint32_t)v[3] << 16),
                                 (uint32_t)v[4] | ((uint32_t)v[5] << 16), (uint32_t)v[6] | ((uint32_t)v[7] << 16));
            __syncthreads();
            // horizontal 5-sum of the neighbours' packed sums (<= 1200 per half: no carry)
            const uint4 n0 = xb[t0], n1 = xb[t1], n3 = xb[t3], n4 = xb[t4], n2 = xb[tid];
            const uint32_t s[4] = {n0.x + n1.x + n2.x + n3.x + n4.x, n0.y + n1.y + n2.y + n3.y + n4.y,
                                   n0.z + n1.z + n2.z + n3.z + n4.z, n0.w + n1.w + n2.w + n3.w + n4.w};
#pragma unroll
            for (int k = 0; k < SD_TH; ++k) {
                const int A = (int)((s[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
                if constexpr (VOL) {
                    const uint32_t sh = (uint32_t)A << (16 * (d & 1));
                    pk[k][0] |= (d & 2) ? 0u : sh;
                    pk[k][1] |= (d & 2) ? sh : 0u;
                    if ((d & 3) == 3 || d == D - 1) {   // pitch is a multiple of 4: the store is aligned and inside the cell
                        if (outcol && y0 + k < H)
                            *reinterpret_cast<uint2*>(vcol + (size_t)k * W * pitch + (d & ~3)) = make_uint2(pk[k][0], pk[k][1]);
                        pk[k][0] = pk[k][1] = 0;
                    }
                    continue;
                }
                // left winner while d ascends: a new strict minimum at d takes the prefix minimum up to
                // d - 2 as its excluded-neighbour second minimum and A(d - 1) as its left parabola
                // neighbour; otherwise A is the right neighbour (d == d1 + 1) or joins the second minimum
                const bool nb = A < best[k], right = d == bd[k] + 1;
                m2[k] = nb ? p2[k] : (right ? m2[k] : min(m2[k], A));
                c2[k] = nb ? SD_BIG : (right ? A : c2[k]);
                c0[k] = nb ? prev[k] : c0[k];
                bd[k] = nb ? d : bd[k];
                best[k] = nb ? A : best[k];
                p2[k] = p1[k];
                p1[k] = min(p1[k], A);
                prev[k] = A;
                // right winner of pixel (y0 + k, p - d): smallest d among the minima
                if (outcol && xr >= 0 && y0 + k < H)
                    atomicMin(&rb[k * SD_RING + (xr & (SD_RING - 1))], ((uint32_t)A << 8) | (uint32_t)d);
            }
        }
        if constexpr (VOL) continue;
        if (outcol) {
#pragma unroll
            for (int k = 0; k < SD_TH; ++k) {
                if (y0 + k >= H) continue;
                const int d1 = bd[k], m1 = best[k];
                bool ok = d1 >= 1 && p - d1 >= 0;
                if (m2[k] != SD_BIG) ok = ok && m1 * 100 <= m2[k] * (100 - a.uniq);
                int off = 0;
                if (d1 >= 1 && d1 <= D - 2) {
                    const int den = c0[k] - 2 * m1 + c2[k];
                    if (den > 0) {   // true floor of (32 (c0 - c2) + den) / (2 den)
                        const int num = 32 * (c0[k] - c2[k]) + den, dn = 2 * den;
                        int q = num / dn;
                        if (num % dn != 0 && num < 0) --q;
                        off = q;
                    }
                }
                const size_t o = out0 + (size_t)(y0 + k) * W + p;
                a.disp[o] = ok ? (uint16_t)(32 * d1 + off) : (uint16_t)0;
                a.wl[o] = (uint8_t)d1;
            }
        }
        __syncthreads();   // every candidate of this step is in the ring
        // right pixels left of the next step's span are final
        const bool last = xc + SD_OUT >= W;
        const int upto = last ? W : max(xc + SD_OUT - (D - 1), 0);
        const int nfl = upto - flushed;
        for (int i = tid; i < nfl * SD_TH; i += SD_BLOCK) {
            const int k = i / nfl, x = flushed + (i - k * nfl);
            uint32_t* e = rb + k * SD_RING + (x & (SD_RING - 1));
            if (y0 + k < H) a.wr[out0 + (size_t)(y0 + k) * W + x] = (uint8_t)(*e & 0xFFu);
            *e = 0xFFFFFFFFu;
        }
        if (nfl > 0) flushed = upto;
    }
}

__global__ __launch_bounds__(256) void k_sd_finish(SdArgs a) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, f = blockIdx.z;
    if (x >= a.W) return;
    const size_t row = (size_t)f * a.W * a.H + (size_t)y * a.W, o = row + x;
    int dv = a.disp[o];
    if (dv) {
        const int d1 = a.wl[o];
        const int dr = a.wr[row + (x - d1)];   // x - d1 >= 0 where disp32 != 0
        if (abs(dr - d1) > a.lr_tol) {
            dv = 0;
            a.disp[o] = 0;
        }
    }
    uint16_t mm = 0;
    if (dv) {
        const double m = floor((a.fxb * 32000.0) / (double)dv + 0.5);
        if (m <= 65535.0) mm = (uint16_t)m;
    }
    a.depth[o] = mm;
}

static SdArgs sd_args(const StereoDepthArgs& s) {
    SdArgs a;
    a.left = s.left;
    a.right = s.right;
    a.stride = s.stride;
    a.ring = s.ring;
    a.first = s.first;
    a.W = s.W;
    a.H = s.H;
    a.D = s.n_disp;
    a.n = s.n;
    a.uniq = s.uniqueness;
    a.lr_tol = s.lr_tol;
    a.fxb = s.fxb;
    a.disp = s.disp32;
    a.depth = s.depth;
    a.wl = s.win_left;
    a.wr = s.win_right;
    return a;
}

template <bool VOL>
static hipError_t sd_launch_match(const SdArgs& a, uint16_t* vol, int pitch, hipStream_t st) {
    const size_t lds = sd_lds_bytes(a.D);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_sd_match<VOL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int nbands = (a.H + SD_TH - 1) / SD_TH;
    hipLaunchKernelGGL(k_sd_match<VOL>, dim3((unsigned)(a.n * nbands)), dim3(SD_BLOCK), lds, st, a, nbands, vol, pitch);
    return hipGetLastError();
}

hipError_t launch_stereo_depth(const StereoDepthArgs& s, hipStream_t st) {
    const SdArgs a = sd_args(s);
    if (a.n <= 0) return hipSuccess;
    const hipError_t e = sd_launch_match<false>(a, nullptr, 0, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sd_finish, dim3((a.W + 255) / 256, a.H, a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sd_volume(const StereoDepthArgs& s, uint16_t* vol, int pitch, hipStream_t st) {
    const SdArgs a = sd_args(s);
    return a.n <= 0 ? hipSuccess : sd_launch_match<true>(a, vol, pitch, st);
}

hipError_t launch_sd_finish(const StereoDepthArgs& s, hipStream_t st) {
    const SdArgs a = sd_args(s);
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sd_finish, dim3((a.W + 255) / 256, a.H, a.n), dim3(256), 0, st, a);
    return hipGetLastError();
}
