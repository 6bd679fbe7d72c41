// k_sd_filter.hip — the post-filters of the dense stereo matcher: rules 9 (median over the valid
// values of an m x m window) and 10 (speckle: 4-connected components of similar disparity with at
// most s pixels are removed) of thor_slam_amd/stereo_depth.py, then rule 8's depth from the
// filtered disp32.  DESIGN.md §6c.  Opt-in (tslam_stereo_depth_filter): nothing here runs otherwise.
//
//   k_sdf_median<M>   32 x 8 pixels per block, the tile and its halo of M / 2 in LDS (clamped
//                     coordinates; a zero becomes 0xFFFF).  A thread holds its window in registers
//                     and selects the floor((n - 1) / 2)-th smallest of the n valid values by 13
//                     bit passes, most significant first: among the values that agree with the bits
//                     decided so far, c have the next bit clear; the k-th lies among them iff
//                     k < c.  An invalid value has every bit set, so it is never among the c and
//                     only ever ranks above the n valid ones.  Out of place: src -> dst.
//   k_sdf_label_tile  one block per 64 x 16 tile, a wave per row (4 rows each).  Horizontal runs
//                     from a ballot of the link-to-left flags, vertical links into an LDS
//                     union-find, one LDS add per run for the component sizes.  out: label = frame
//                     pixel index of the pixel's tile-local root; count = the local component's
//                     size at the local root's pixel, 0 elsewhere.
//   k_sdf_merge       one thread per pixel of a tile's first row / first column (not the image's):
//                     a lock-free union with the neighbour across the border, skipped where the
//                     previous pixel along the border already joins the same two tile components.
//   k_sdf_sum         every local root adds its count to its final root's (one atomic per tile and
//                     component) and points its label straight at it.
//   k_sdf_apply       per pixel: disp32 zeroed where the final root's count <= s; depth.  Without
//                     labels (median only) it is the plain depth pass.
//
// The phases are separate launches on one stream; no block waits for another.
#include "tslam_common.h"

#define SDF_MED_W 32
#define SDF_MED_H 8
#define SDF_TW 64                 // tile width = one wave
#define SDF_TH 16
#define SDF_ROWS 4                // rows per wave: SDF_TH / (256 / 64)
#define SDF_NONE 0xFFFFu

static_assert(SDF_TW == 64 && SDF_ROWS * 4 == SDF_TH, "a wave per tile row, four waves");

template <int M>
__global__ __launch_bounds__(256) void k_sdf_median(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int W, int H) {
    constexpr int R = M / 2, LW = SDF_MED_W + 2 * R, LH = SDF_MED_H + 2 * R;
    __shared__ uint16_t t[LH * LW];
    const int tid = threadIdx.x, x0 = blockIdx.x * SDF_MED_W, y0 = blockIdx.y * SDF_MED_H;
    const size_t fo = (size_t)blockIdx.z * W * H;
    for (int i = tid; i < LH * LW; i += 256) {
        const int r = i / LW, c = i - r * LW;
        const int y = min(max(y0 - R + r, 0), H - 1), x = min(max(x0 - R + c, 0), W - 1);
        const uint16_t v = src[fo + (size_t)y * W + x];
        t[i] = v ? v : (uint16_t)SDF_NONE;
    }
    __syncthreads();
    const int lx = tid & (SDF_MED_W - 1), ly = tid / SDF_MED_W, x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    uint32_t v[M * M];
    int n = 0;
#pragma unroll
    for (int j = 0; j < M; ++j)
#pragma unroll
        for (int i = 0; i < M; ++i) {
            v[j * M + i] = t[(ly + j) * LW + lx + i];
            n += v[j * M + i] != SDF_NONE;
        }
    uint32_t out = 0;
    if (v[R * M + R] != SDF_NONE) {       // an invalid centre stays invalid; else n >= 1
        int k = (n - 1) >> 1;
#pragma unroll
        for (int b = 12; b >= 0; --b) {
            const uint32_t m = 0x1FFFu & ~((1u << b) - 1u);   // the decided bits and bit b
            int c = 0;
#pragma unroll
            for (int i = 0; i < M * M; ++i) c += (v[i] & m) == out;
            if (k >= c) {
                out |= 1u << b;
                k -= c;
            }
        }
    }
    dst[fo + (size_t)y * W + x] = (uint16_t)out;
}

// Union-find on indices, in LDS (tile-local) and in device memory (frame-wide).  The invariant of
// both: parent[i] <= i at all times.  A label starts at the smallest index of its run or tile
// component, and the only later write is an atomicMin with a smaller index, so every find walks
// strictly decreasing indices and ends at an i with parent[i] == i: it terminates by construction,
// whatever other threads do meanwhile.  A union hangs the larger root under the smaller; when the
// atomicMin finds that the larger one was no root any more (old != a), the edge it just redirected
// is kept by uniting old with b next, again with smaller indices: no connection is ever lost and
// the retries are bounded by the indices.
template <int SCOPE>
__device__ __forceinline__ uint32_t sdf_find(uint32_t* parent, uint32_t i) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(parent + i, __ATOMIC_RELAXED, SCOPE);
        if (p == i) return i;
        i = p;
    }
}

template <int SCOPE>
__device__ __forceinline__ void sdf_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = sdf_find<SCOPE>(parent, a);
        b = sdf_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ bool sdf_linked(int a, int b, int r) { return a != 0 && b != 0 && abs(a - b) <= r; }

__global__ __launch_bounds__(256) void k_sdf_label_tile(const uint16_t* __restrict__ src, uint32_t* __restrict__ label,
                                                         uint32_t* __restrict__ count, int W, int H, int r) {
    __shared__ uint16_t val[SDF_TH * SDF_TW];
    __shared__ uint32_t par[SDF_TH * SDF_TW];
    __shared__ uint32_t cnt[SDF_TH * SDF_TW];
    __shared__ uint64_t row_starts[SDF_TH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * SDF_TW + lane, y0 = blockIdx.y * SDF_TH;
    const size_t fo = (size_t)blockIdx.z * W * H;

    int v[SDF_ROWS];
    uint64_t starts[SDF_ROWS];
#pragma unroll
    for (int k = 0; k < SDF_ROWS; ++k) {
        const int ly = wave + 4 * k, y = y0 + ly, idx = ly * SDF_TW + lane;
        v[k] = (x < W && y < H) ? (int)src[fo + (size_t)y * W + x] : 0;
        const int left = __shfl_up(v[k], 1);
        const bool link = lane > 0 && sdf_linked(v[k], left, r);
        starts[k] = __ballot(!link);                                  // bit 0 is always set
        const uint64_t upto = starts[k] & ((2ull << lane) - 1ull);    // lane 63: 2^64 wraps to 0, the mask to all ones
        val[idx] = (uint16_t)v[k];
        par[idx] = (uint32_t)(ly * SDF_TW + 63 - __clzll((long long)upto));   // the run's first pixel
        cnt[idx] = 0;
        if (lane == 0) row_starts[ly] = starts[k];
    }
    __syncthreads();
    // vertical links.  Where this pixel and the one above both continue a run and the column to the
    // left is linked upwards too, that column's union already joins the two runs.
#pragma unroll
    for (int k = 0; k < SDF_ROWS; ++k) {
        const int ly = wave + 4 * k, idx = ly * SDF_TW + lane;
        const bool up = ly > 0 && sdf_linked(v[k], val[ly > 0 ? idx - SDF_TW : idx], r);
        const uint64_t ups = __ballot(up);
        if (!up) continue;
        const uint64_t above = row_starts[ly - 1];
        const bool covered = lane > 0 && !((starts[k] >> lane) & 1) && !((above >> lane) & 1) && ((ups >> (lane - 1)) & 1);
        if (!covered) sdf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)idx, (uint32_t)(idx - SDF_TW));
    }
    __syncthreads();
    uint32_t root[SDF_ROWS];
#pragma unroll
    for (int k = 0; k < SDF_ROWS; ++k) {
        const int idx = (wave + 4 * k) * SDF_TW + lane;
        root[k] = sdf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, (uint32_t)idx);
        if (v[k] != 0 && ((starts[k] >> lane) & 1)) {                 // one add per run: its length
            const uint64_t next = (starts[k] >> lane) >> 1;
            const int len = next ? __builtin_ctzll(next) + 1 : SDF_TW - lane;
            atomicAdd(&cnt[root[k]], (uint32_t)len);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SDF_ROWS; ++k) {
        const int ly = wave + 4 * k, y = y0 + ly, idx = ly * SDF_TW + lane;
        if (x >= W || y >= H) continue;
        const uint32_t p = (uint32_t)(y * W + x);
        const uint32_t g = (uint32_t)((y0 + (int)(root[k] >> 6)) * W + blockIdx.x * SDF_TW + (int)(root[k] & 63));
        label[fo + p] = v[k] != 0 ? g : p;
        count[fo + p] = (v[k] != 0 && root[k] == (uint32_t)idx) ? cnt[idx] : 0u;
    }
}

__global__ __launch_bounds__(256) void k_sdf_merge(const uint16_t* __restrict__ src, uint32_t* label, int W, int H, int r) {
    const int nh = ((H + SDF_TH - 1) / SDF_TH - 1) * W, nv = ((W + SDF_TW - 1) / SDF_TW - 1) * H;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int x, y, q, back;            // back: to the previous pixel along the border, 0 at a tile's first
    if (i < nh) {                 // a tile's first row and the row above it
        const int by = i / W;
        x = i - by * W;
        y = (by + 1) * SDF_TH;
        q = (y - 1) * W + x;
        back = (x % SDF_TW) ? 1 : 0;
    } else if (i < nh + nv) {     // a tile's first column and the column left of it
        const int j = i - nh, bx = j / H;
        y = j - bx * H;
        x = (bx + 1) * SDF_TW;
        q = y * W + x - 1;
        back = (y % SDF_TH) ? W : 0;
    } else {
        return;
    }
    const uint16_t* s = src + (size_t)blockIdx.y * W * H;
    const int p = y * W + x, a = s[p], b = s[q];
    if (!sdf_linked(a, b, r)) return;
    // Where the previous pair along the border, inside the same two tiles, is linked to this one on
    // both sides and across, its union (or the one that covers it in turn) joins the same two tile
    // components: a smooth surface costs one union per border, not one per pixel.
    if (back) {
        const int a1 = s[p - back], b1 = s[q - back];
        if (sdf_linked(a, a1, r) && sdf_linked(b, b1, r) && sdf_linked(a1, b1, r)) return;
    }
    sdf_union<__HIP_MEMORY_SCOPE_AGENT>(label + blockIdx.y * (size_t)W * H, (uint32_t)p, (uint32_t)q);
}

__global__ __launch_bounds__(256) void k_sdf_sum(uint32_t* label, uint32_t* count, int npx) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const size_t fo = (size_t)blockIdx.y * npx;
    const uint32_t c = count[fo + p];     // != 0: a tile-local root.  Only a final root's count is added to, and it adds nothing
    if (c == 0) return;
    const uint32_t root = sdf_find<__HIP_MEMORY_SCOPE_AGENT>(label + fo, (uint32_t)p);
    if (root == (uint32_t)p) return;
    atomicAdd(&count[fo + root], c);
    __hip_atomic_store(label + fo + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // still an ancestor, still smaller
}

__global__ __launch_bounds__(256) void k_sdf_apply(const uint16_t* src, uint16_t* disp, uint16_t* __restrict__ depth,
                                                    uint32_t* label, const uint32_t* __restrict__ count, int npx, uint32_t size,
                                                    double fxb) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    const size_t fo = (size_t)blockIdx.y * npx, o = fo + p;
    int dv = src[o];
    if (dv && label) {
        const uint32_t root = sdf_find<__HIP_MEMORY_SCOPE_AGENT>(label + fo, (uint32_t)p);
        if (count[fo + root] <= size) dv = 0;
    }
    disp[o] = (uint16_t)dv;
    uint16_t mm = 0;
    if (dv) {
        const double m = floor((fxb * 32000.0) / (double)dv + 0.5);
        if (m <= 65535.0) mm = (uint16_t)m;
    }
    depth[o] = mm;
}

__global__ __launch_bounds__(256) void k_sdf_load(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint16_t v = src[i];
    dst[i] = v > 8191 ? (uint16_t)8191 : v;
}

hipError_t launch_sd_filter_load(const uint16_t* src, uint16_t* dst, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sdf_load, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, n);
    return hipGetLastError();
}

hipError_t launch_sd_filter(const StereoFilterArgs& a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    const int W = a.W, H = a.H, npx = W * H;
    const uint16_t* src = a.disp32;
    if (a.median) {
        const dim3 grid((W + SDF_MED_W - 1) / SDF_MED_W, (H + SDF_MED_H - 1) / SDF_MED_H, a.n);
        if (a.median == 3) hipLaunchKernelGGL(k_sdf_median<3>, grid, dim3(256), 0, st, src, a.tmp, W, H);
        else if (a.median == 5) hipLaunchKernelGGL(k_sdf_median<5>, grid, dim3(256), 0, st, src, a.tmp, W, H);
        else hipLaunchKernelGGL(k_sdf_median<7>, grid, dim3(256), 0, st, src, a.tmp, W, H);
        src = a.tmp;
    }
    const bool speckle = a.speckle_size > 0;
    if (speckle) {
        const int ntx = (W + SDF_TW - 1) / SDF_TW, nty = (H + SDF_TH - 1) / SDF_TH;
        hipLaunchKernelGGL(k_sdf_label_tile, dim3(ntx, nty, a.n), dim3(256), 0, st, src, a.label, a.count, W, H, a.speckle_range);
        const int nborder = (nty - 1) * W + (ntx - 1) * H;
        if (nborder > 0)
            hipLaunchKernelGGL(k_sdf_merge, dim3((nborder + 255) / 256, a.n), dim3(256), 0, st, src, a.label, W, H, a.speckle_range);
        hipLaunchKernelGGL(k_sdf_sum, dim3((npx + 255) / 256, a.n), dim3(256), 0, st, a.label, a.count, npx);
    }
    hipLaunchKernelGGL(k_sdf_apply, dim3((npx + 255) / 256, a.n), dim3(256), 0, st, src, a.disp32, a.depth,
                       speckle ? a.label : nullptr, a.count, npx, (uint32_t)a.speckle_size, a.fxb);
    return hipGetLastError();
}
