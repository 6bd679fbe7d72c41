// k_tsdf_store_mesh.hip — one marching-cubes mesh of the whole dense map: the rolling window and the
// brick store together (thor_slam_amd/dense_store.py, "The mesh of the whole map", is the spec;
// tests/ref_tsdf_store_mesh.py restates it).  The rules are k_dense.hip's, over the store's absolute
// voxel grid: a vertex depends on absolute coordinates alone, never on where the window stands.
//
//   k_wmesh_list   walks the hash table's cells and appends (one atomicAdd each) the key of every
//                  brick that holds a voxel and lies outside the window's brick range, then the keys
//                  of the window's own bricks, by arithmetic from the TsdfWindow record.  The host
//                  sorts the compacted keys (8 B per brick) into ascending (bz, by, bx).
//   k_wmesh_count  one block of 512 threads per listed brick.  Eight lanes find the 8 source bricks
//                  b + {0, 1}^3 in the table (a slot, -1, or WMESH_IN_WINDOW for a brick the window
//                  holds whole); the 9 x 9 x 9 corner tile of (tsdf, weight) goes to LDS, every tile
//                  voxel loaded once from the window's arrays or from its pool brick (chosen per
//                  voxel: a window edge can cut a brick), x fastest, all of a thread's loads issued
//                  before any value is looked at; then the 512 cubes form their configuration byte
//                  from LDS and the block's triangle total goes to block_sums[brick].
//   k_mesh_scan    (k_dense.hip) the bricks' first triangles and the mesh's triangle count.
//   k_wmesh_emit   stages the same tile (with the colour layer 3 more words per voxel: 14,580 B of
//                  LDS), forms the configuration bytes again, scans the 512 counts in the block and
//                  writes 9 f32 per triangle (and 9 f32 of colours) at block_off[brick] + the cube's
//                  local offset, bounded by the buffer's capacity as k_mesh_emit is.
//   The configuration bytes are recomputed rather than stored: the emit needs the tile in LDS for
//   the interpolation anyway, and 8 LDS reads per cube cost less than 512 B per brick written,
//   read back and kept in one more buffer.
//
// The mesh only READS the store.  It runs in stream order after any move, so no insert is in flight
// while it runs: the table's keys, slots and occupancy are plain loads here.  Nothing spins, nothing
// waits on another wave's store, and the list's append is the only atomic.
//   Roofline: HBM / L2 — 729 x 2 (5 with colour) words per brick and pass, each read once, against
//   512 cubes; 36 (72) B written per triangle.
#include "tslam_common.h"
#include "tslam_mc_table.h"
#include "tslam_tsdf_store_mesh.h"

#define WMESH_THREADS 512
#define WMESH_LIST_THREADS 256

// the window as the record has it now (shift includes the last move's delta)
__device__ __forceinline__ void wmesh_window(const WmeshArgs& a, int32_t lo[3], int32_t n[3]) {
    lo[0] = a.win->shift[0], lo[1] = a.win->shift[1], lo[2] = a.win->shift[2];
    n[0] = a.nx, n[1] = a.ny, n[2] = a.nz;
}

// the key's slot or -1; no kernel inserts while the mesh runs
__device__ static int wmesh_find(const TsdfStore& st, uint64_t key) {
    uint32_t c = store_hash(key, st.mask);
    for (uint32_t p = 0; p <= st.mask; ++p, c = (c + 1) & st.mask) {
        const unsigned long long k = st.keys[c];
        if (k == key) {
            const int slot = st.vals[c];
            return slot >= 0 && slot < st.capacity ? slot : -1;
        }
        if (k == 0) return -1;
    }
    return -1;
}

// threads 0 .. cells - 1 take a cell each, threads cells .. cells + max_window - 1 a brick of the
// window's range (max_window: what the host knows the range cannot exceed).  *count goes past `cap`
// when the list is too short; the host grows it and lists again.
__global__ __launch_bounds__(WMESH_LIST_THREADS) void k_wmesh_list(WmeshArgs a, int64_t cells, int64_t max_window,
                                                                   unsigned long long* list, int64_t cap, uint32_t* count) {
    const int64_t t = (int64_t)blockIdx.x * WMESH_LIST_THREADS + threadIdx.x;
    if (t >= cells + max_window) return;
    int32_t lo[3], n[3], b[3];
    wmesh_window(a, lo, n);
    const WmeshRange r = wmesh_window_range(lo, n);
    unsigned long long key = 0;
    if (t < cells) {
        const unsigned long long k = a.st.keys[t];
        if (k == 0) return;
        const int slot = a.st.vals[t];
        if (slot < 0 || slot >= a.st.capacity || a.st.occ[slot] <= 0) return;
        store_key_coords(k, b);
        if (!wmesh_outside(r, b)) return;
        key = k;
    } else {
        const int64_t w = t - cells;
        if (w >= wmesh_range_count(r)) return;
        wmesh_range_brick(r, w, b);
        if (!wmesh_brick_ok(b)) return;   // no key: the store could not hold it either
        key = store_key(b[0], b[1], b[2]);
    }
    const uint32_t at = atomicAdd(count, 1u);
    if ((int64_t)at < cap) list[at] = key;
}

// The tile in LDS: [word][tz][ty][tx], words 0 tsdf, 1 weight, 2..4 colour.
template <bool COL>
struct WmeshTile {
    uint32_t w[COL ? 5 : 2][WMESH_TV];
    int slot[8];
};

// Block: find the 8 source bricks, then load the tile.  A thread holds tile voxels threadIdx.x and
// threadIdx.x + 512 (< 729): consecutive threads, consecutive x.
template <bool COL>
__device__ __forceinline__ void wmesh_stage(const WmeshArgs& a, const int32_t b[3], WmeshTile<COL>& s) {
    int32_t lo[3], n[3];
    wmesh_window(a, lo, n);
    if (threadIdx.x < 8) {
        const int32_t sb[3] = {b[0] + (int)(threadIdx.x & 1), b[1] + (int)((threadIdx.x >> 1) & 1), b[2] + (int)(threadIdx.x >> 2)};
        int slot = -1;
        if (wmesh_brick_in_window(sb, lo, n)) slot = WMESH_IN_WINDOW;
        else if (wmesh_brick_ok(sb)) slot = wmesh_find(a.st, store_key(sb[0], sb[1], sb[2]));
        s.slot[threadIdx.x] = slot;
    }
    __syncthreads();
    constexpr int NW = COL ? 5 : 2;
    uint32_t v[2][NW];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int c = 0; c < NW; ++c) v[r][c] = 0u;
        const int ti = (int)threadIdx.x + r * WMESH_THREADS;
        if (ti >= WMESH_TV) continue;
        const int tx = ti % WMESH_T, ty = (ti / WMESH_T) % WMESH_T, tz = ti / (WMESH_T * WMESH_T);
        const WmeshSource src = wmesh_source(b, tx, ty, tz, lo, n);
        if (src.window) {
            v[r][0] = __float_as_uint(a.tsdf[src.index]);
            v[r][1] = __float_as_uint(a.weight[src.index]);
            if constexpr (COL) {
                v[r][2] = __float_as_uint(a.color[3 * src.index]);
                v[r][3] = __float_as_uint(a.color[3 * src.index + 1]);
                v[r][4] = __float_as_uint(a.color[3 * src.index + 2]);
            }
        } else {
            const int slot = s.slot[src.brick];
            if (slot < 0) continue;
            const uint32_t* brick = a.st.pool + (int64_t)slot * a.st.wpv * TSDF_STORE_BV;
            v[r][0] = brick[src.index];
            v[r][1] = brick[TSDF_STORE_BV + src.index];
            if constexpr (COL) {
                v[r][2] = brick[3 * TSDF_STORE_BV + 3 * src.index];
                v[r][3] = brick[3 * TSDF_STORE_BV + 3 * src.index + 1];
                v[r][4] = brick[3 * TSDF_STORE_BV + 3 * src.index + 2];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int ti = (int)threadIdx.x + r * WMESH_THREADS;
        if (ti >= WMESH_TV) continue;
#pragma unroll
        for (int c = 0; c < NW; ++c) s.w[c][ti] = v[r][c];
    }
    __syncthreads();
}

// tile index of cube threadIdx.x's base corner: cube (i, j, k) = (t & 7, t >> 3 & 7, t >> 6)
__device__ __forceinline__ int wmesh_cube_base() {
    const int t = (int)threadIdx.x;
    return ((t >> 6) * WMESH_T + ((t >> 3) & 7)) * WMESH_T + (t & 7);
}

// configuration byte of the thread's cube (0 when a corner is unobserved), as k_dense.hip's cube_config
template <bool COL>
__device__ __forceinline__ uint32_t wmesh_config(const WmeshTile<COL>& s, float min_weight) {
    const int v = wmesh_cube_base();
    uint32_t cfg = 0;
    bool obs = true;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int o = v + (n & 1) + ((n >> 1) & 1) * WMESH_T + ((n >> 2) & 1) * WMESH_T * WMESH_T;
        obs &= __uint_as_float(s.w[1][o]) >= min_weight;
        cfg |= (__uint_as_float(s.w[0][o]) < 0.0f ? 1u : 0u) << n;
    }
    return obs ? cfg : 0u;
}

__device__ __forceinline__ void wmesh_brick(const unsigned long long* list, int32_t b[3]) { store_key_coords(list[blockIdx.x], b); }

__global__ __launch_bounds__(WMESH_THREADS) void k_wmesh_count(WmeshArgs a, const unsigned long long* list, uint32_t* block_sums) {
    __shared__ WmeshTile<false> s;   // the count needs no colour
    __shared__ uint32_t s_w[WMESH_THREADS / 64];
    int32_t b[3];
    wmesh_brick(list, b);
    wmesh_stage<false>(a, b, s);
    uint32_t n = TSLAM_MC_COUNT[wmesh_config<false>(s, a.min_weight)];
    n = (uint32_t)wave_sum_i32((int)n);
    if (wave_lane() == 0) s_w[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < WMESH_THREADS / 64; ++w) t += s_w[w];
        block_sums[blockIdx.x] = t;
    }
}

template <bool COL>
__global__ __launch_bounds__(WMESH_THREADS) void k_wmesh_emit(WmeshArgs a, const unsigned long long* list, const uint64_t* block_off,
                                                              float* tris, float* cols, int64_t cap) {
    __shared__ WmeshTile<COL> s;
    __shared__ uint32_t s_w[WMESH_THREADS / 64];
    int32_t b[3];
    wmesh_brick(list, b);
    wmesh_stage<COL>(a, b, s);
    const uint32_t cfg = wmesh_config<COL>(s, a.min_weight);
    const uint32_t n = TSLAM_MC_COUNT[cfg];
    // block-local exclusive scan of the counts, in cube order [k][j][i]
    const int lane = wave_lane(), w = threadIdx.x >> 6;
    uint32_t inc = n;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += y;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t before = 0;
    for (int k = 0; k < w; ++k) before += s_w[k];
    if (n == 0) return;
    const int vbase = wmesh_cube_base();
    const int cube[3] = {(int)(threadIdx.x & 7), (int)((threadIdx.x >> 3) & 7), (int)(threadIdx.x >> 6)};
    const int64_t first = (int64_t)block_off[blockIdx.x] + before + inc - n;
    const int stride[3] = {1, WMESH_T, WMESH_T * WMESH_T};
    const double o0[3] = {a.ox, a.oy, a.oz};
    for (uint32_t t = 0; t < n; ++t) {
        const int64_t tri = first + t;
        if (tri >= cap) return;
        float* out = tris + tri * 9;
        for (int vtx = 0; vtx < 3; ++vtx) {
            const int e = TSLAM_MC_TRIS[(cfg * TSLAM_MC_MAX_TRIS + t) * 3 + vtx];
            const int ax = e >> 2, m = e & 3;
            const int a0 = ax == 0 ? 1 : 0, a1 = ax == 2 ? 1 : 2;   // the other two axes, low first
            int off[3] = {0, 0, 0};
            off[a0] = m & 1;
            off[a1] = m >> 1;
            const int vb = vbase + off[0] * stride[0] + off[1] * stride[1] + off[2] * stride[2];
            const float va = __uint_as_float(s.w[0][vb]), ve = __uint_as_float(s.w[0][vb + stride[ax]]);
            const float tt = va / (va - ve);   // IEEE f32 division (no fast-math, no contraction)
            float p[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)   // the absolute voxel's centre from the unshifted origin, f64
                p[c] = (float)(o0[c] + a.s * (((int64_t)TSDF_STORE_B * b[c] + cube[c] + off[c]) + 0.5));
            p[ax] = p[ax] + tt * a.sf;
            out[3 * vtx + 0] = p[0];
            out[3 * vtx + 1] = p[1];
            out[3 * vtx + 2] = p[2];
            if constexpr (COL) {   // the colour of the edge's voxel nearer to the vertex
                const int cv = tt < 0.5f ? vb : vb + stride[ax];
                float* oc = cols + tri * 9 + 3 * vtx;
                oc[0] = __uint_as_float(s.w[2][cv]);
                oc[1] = __uint_as_float(s.w[3][cv]);
                oc[2] = __uint_as_float(s.w[4][cv]);
            }
        }
    }
}

void launch_wmesh_list(const WmeshArgs& a, int64_t cells, int64_t max_window, uint64_t* list, int64_t cap, uint32_t* count, hipStream_t s) {
    const int64_t blocks = (cells + max_window + WMESH_LIST_THREADS - 1) / WMESH_LIST_THREADS;
    hipLaunchKernelGGL(k_wmesh_list, dim3((unsigned)blocks), dim3(WMESH_LIST_THREADS), 0, s, a, cells, max_window,
                       reinterpret_cast<unsigned long long*>(list), cap, count);
}

void launch_wmesh_count(const WmeshArgs& a, const uint64_t* list, int64_t n_bricks, uint32_t* block_sums, hipStream_t s) {
    hipLaunchKernelGGL(k_wmesh_count, dim3((unsigned)n_bricks), dim3(WMESH_THREADS), 0, s, a,
                       reinterpret_cast<const unsigned long long*>(list), block_sums);
}

void launch_wmesh_emit(const WmeshArgs& a, const uint64_t* list, int64_t n_bricks, const uint64_t* block_off, float* tris, float* cols,
                       int64_t cap, hipStream_t s) {
    const dim3 g((unsigned)n_bricks), b(WMESH_THREADS);
    const unsigned long long* l = reinterpret_cast<const unsigned long long*>(list);
    if (a.color) hipLaunchKernelGGL(k_wmesh_emit<true>, g, b, 0, s, a, l, block_off, tris, cols, cap);
    else hipLaunchKernelGGL(k_wmesh_emit<false>, g, b, 0, s, a, l, block_off, tris, cols, cap);
}
