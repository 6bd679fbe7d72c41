// k_tsdf_store.hip — the dense map's brick store (thor_slam_amd/dense_store.py is the spec;
// tests/ref_tsdf_store.py restates it): what leaves the rolling window is kept, what enters comes back.
//
//   k_tsdf_store_out  before k_tsdf_move: every window voxel the move has no place for, with a
//                     non-zero word, goes to its absolute coordinate in the pool;
//   k_tsdf_store_in   after it: every window voxel the move had no source for takes its words from
//                     the pool, where they are zeroed.
//
// Both read delta and shift from the TsdfWindow record (uniform loads) and return at once when delta
// is zero, so a call that does not move pays two empty launches and no host synchronise.
//
// One wave per store brick (8 x 8 x 8 absolute voxels) that overlaps the window's extent, bricks
// grid-strided over a bounded grid; lane l holds voxels (x = l & 7, y = l >> 3, z = 0..7).  A brick
// whose clipped index range cannot hold a leaving (entering) voxel is skipped before any load.
// A lane loads the words of all its voxels before it looks at any, so a brick costs a few memory
// round trips, not one per voxel and layer.
// Lane 0 finds or inserts the brick's key and the slot goes to the wave by a shuffle.  A brick is
// the business of exactly one wave of a launch, so no wave reads a slot that another one is still
// publishing, and nothing here waits on a value another lane or wave has yet to write: the only
// shared steps are one atomicCAS per probed empty cell and one atomicAdd per new brick.
//
// The table: open addressing, linear probing, 64-bit keys (tslam_tsdf_store.h), cells = a power of
// two >= 2 x capacity, so a probe always meets an empty cell.  A slot is taken from the counter
// before its key is inserted; with the counter at capacity nothing is inserted and the brick's
// leaving voxels are counted as dropped.
#include <algorithm>

#include "tslam_common.h"
#include "tslam_tsdf_store.h"

#define STORE_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the key's slot, or -1 (no launch inserts while this runs on a key of its own brick)
__device__ static int store_find(const TsdfStore& st, uint64_t key) {
    uint32_t c = store_hash(key, st.mask);
    for (uint32_t p = 0; p <= st.mask; ++p, c = (c + 1) & st.mask) {
        const unsigned long long k = __hip_atomic_load(&st.keys[c], STORE_AGENT);
        if (k == key) return st.vals[c];
        if (k == 0) return -1;
    }
    return -1;
}

// the key's slot, a new one if the key is absent, -1 when the pool is full
__device__ static int store_find_or_insert(const TsdfStore& st, uint64_t key) {
    uint32_t c = store_hash(key, st.mask);
    int slot = -1;
    for (uint32_t p = 0; p <= st.mask; ++p, c = (c + 1) & st.mask) {
        const unsigned long long k = __hip_atomic_load(&st.keys[c], STORE_AGENT);
        if (k == key) return st.vals[c];   // from an earlier move: this launch has one wave per brick
        if (k != 0) continue;
        if (slot < 0) {   // the slot first, so a key in the table always has one
            slot = atomicAdd(&st.ctr->bricks, 1);
            if (slot >= st.capacity) {
                atomicSub(&st.ctr->bricks, 1);
                return -1;
            }
        }
        if (atomicCAS(&st.keys[c], 0ULL, (unsigned long long)key) == 0ULL) {
            st.vals[c] = slot;
            return slot;
        }
        // another brick's key took the cell meanwhile: on to the next one
    }
    return -1;
}

// |shift| and |delta| stay below 2^30 (TSDF_SHIFT_LIMIT), so the window's first absolute voxel, the
// brick coordinates and the window indices of a brick's voxels are 32-bit; only a voxel's linear
// index needs 64.  delta is clamped to +-dim per axis first (beyond that every voxel leaves or
// enters on that axis anyway), so index - delta stays in range as well.
//
// what a wave knows of its brick: the window index of local voxel (0, 0, 0) and whether the brick
// can hold a voxel without a place (OUT: sign -1) or without a source (IN: sign +1) in the move
struct StoreBrick {
    int bx, by, bz;   // absolute brick coordinates
    int i0, j0, k0;   // window index of the brick's first voxel (may be negative)
    bool touched;
};

// is index i + m outside [0, n)?  i in [0, n), |m| <= min(n, 2^30), n <= 2^31: the sum lies in
// (-2^31, 2^32 - 2^31), so modulo 2^32 a negative sum is a large unsigned number and one compare does
__device__ __forceinline__ bool store_outside(int i, int m, int n) { return (uint32_t)i + (uint32_t)m >= (uint32_t)n; }

// loc: the local index of the window's first voxel in brick b0, so brick b0 + (tx, ty, tz) starts at
// window index 8 (tx, ty, tz) - loc
__device__ static StoreBrick store_brick(int64_t t, const int b0[3], const int nb[3], const int loc[3], const int n[3],
                                         const int d[3], int sign) {
    StoreBrick b;
    const int tx = (int)(t % nb[0]), ty = (int)((t / nb[0]) % nb[1]), tz = (int)(t / ((int64_t)nb[0] * nb[1]));
    b.bx = b0[0] + tx;
    b.by = b0[1] + ty;
    b.bz = b0[2] + tz;
    const int tt[3] = {tx, ty, tz};
    int w0[3];
    b.touched = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w0[a] = TSDF_STORE_B * tt[a] - loc[a];   // in [-7, n - 1]: the brick overlaps the window
        const int i0 = max(w0[a], 0), i1 = (int)min((int64_t)w0[a] + TSDF_STORE_B - 1, (int64_t)n[a] - 1);
        if (store_outside(i0, sign * d[a], n[a]) || store_outside(i1, sign * d[a], n[a])) b.touched = true;
    }
    b.i0 = w0[0], b.j0 = w0[1], b.k0 = w0[2];
    return b;
}

// the window's extent in absolute voxels and the bricks it overlaps
__device__ static int64_t store_extent(const int lo[3], const int n[3], int b0[3], int nb[3], int loc[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        b0[a] = (int)store_brick_of(lo[a]);
        loc[a] = store_local_of(lo[a]);
        nb[a] = (int)(store_brick_of((int64_t)lo[a] + n[a] - 1) - b0[a] + 1);
    }
    return (int64_t)nb[0] * nb[1] * nb[2];
}

// delta of the record, clamped to +-dim per axis
__device__ __forceinline__ int store_clamp(int d, int n) { return d > n ? n : (d < -n ? -n : d); }

// voxels of the wave whose bit r of `bits` is set, over r = 0..7
__device__ static int store_count(unsigned bits) {
    int n = 0;
#pragma unroll
    for (int r = 0; r < TSDF_STORE_B; ++r) n += __popcll(__ballot((bits >> r) & 1u));
    return n;
}

// The layers as the store's kernels address them.  TsdfLayers' order is fixed (tsdf, weight, then
// colour weight and colour when the colour layer is on, then the free-space words when that layer
// is on), so n = 2, 3, 4, 5 says which layers exist (one instantiation <COL, FS> each, chosen by the
// launcher and checked by store_view), and a voxel's words have fixed places in
// registers: 0 tsdf, 1 weight, 2 colour weight, 3..5 colour, 6 free-space.  A brick's words of all
// 8 z are loaded before any is looked at, so a wave's loads are in flight together.
struct StoreView {
    uint32_t *t, *w, *cw, *c, *f;   // the window's layers as words (cw, c / f null without the layer)
    int fs_off;                     // the free-space word's place among a pool brick's words
    int wpv;
    bool ok;                        // the layers are laid out as above and fit the pool's bricks
};

template <bool COL, bool FS>
__device__ static StoreView store_view(const TsdfLayers& l, const TsdfStore& st) {
    StoreView s{};
    const bool col = COL, fs = FS;
    s.ok = l.n == 2 + (COL ? 2 : 0) + (FS ? 1 : 0) && l.comp[0] == 1 && l.comp[1] == 1 && (!col || (l.comp[2] == 1 && l.comp[3] == 3)) &&
           (!fs || l.comp[l.n - 1] == 1);
    s.fs_off = col ? 6 : 2;
    s.wpv = s.fs_off + (fs ? 1 : 0);
    s.ok = s.ok && s.wpv <= st.wpv;   // the host refuses a layer the pool was not sized for
    if (!s.ok) return s;
    s.t = reinterpret_cast<uint32_t*>(l.vol[0]);
    s.w = reinterpret_cast<uint32_t*>(l.vol[1]);
    if (col) {
        s.cw = reinterpret_cast<uint32_t*>(l.vol[2]);
        s.c = reinterpret_cast<uint32_t*>(l.vol[3]);
    }
    if (fs) s.f = reinterpret_cast<uint32_t*>(l.vol[l.n - 1]);
    return s;
}

// window voxel v -> registers
template <bool COL, bool FS>
__device__ __forceinline__ void store_load_window(const StoreView& s, int64_t v, uint32_t (&w)[TSDF_STORE_MAX_WORDS]) {
    w[0] = s.t[v];
    w[1] = s.w[v];
    if constexpr (COL) {
        w[2] = s.cw[v];
        w[3] = s.c[3 * v];
        w[4] = s.c[3 * v + 1];
        w[5] = s.c[3 * v + 2];
    }
    if constexpr (FS) w[6] = s.f[v];
}

template <bool COL, bool FS>
__device__ __forceinline__ void store_save_window(const StoreView& s, int64_t v, const uint32_t (&w)[TSDF_STORE_MAX_WORDS]) {
    s.t[v] = w[0];
    s.w[v] = w[1];
    if constexpr (COL) {
        s.cw[v] = w[2];
        s.c[3 * v] = w[3];
        s.c[3 * v + 1] = w[4];
        s.c[3 * v + 2] = w[5];
    }
    if constexpr (FS) s.f[v] = w[6];
}

// a pool brick's local voxel lv (0..511): per layer [8][8][8][comp] words
template <bool COL, bool FS>
__device__ __forceinline__ void store_load_pool(const StoreView& s, const uint32_t* brick, int lv, uint32_t (&w)[TSDF_STORE_MAX_WORDS]) {
    w[0] = brick[lv];
    w[1] = brick[TSDF_STORE_BV + lv];
    if constexpr (COL) {
        w[2] = brick[2 * TSDF_STORE_BV + lv];
        w[3] = brick[3 * TSDF_STORE_BV + 3 * lv];
        w[4] = brick[3 * TSDF_STORE_BV + 3 * lv + 1];
        w[5] = brick[3 * TSDF_STORE_BV + 3 * lv + 2];
    }
    if constexpr (FS) w[6] = brick[(COL ? 6 : 2) * TSDF_STORE_BV + lv];
}

template <bool COL, bool FS>
__device__ __forceinline__ void store_save_pool(const StoreView& s, uint32_t* brick, int lv, const uint32_t (&w)[TSDF_STORE_MAX_WORDS]) {
    brick[lv] = w[0];
    brick[TSDF_STORE_BV + lv] = w[1];
    if constexpr (COL) {
        brick[2 * TSDF_STORE_BV + lv] = w[2];
        brick[3 * TSDF_STORE_BV + 3 * lv] = w[3];
        brick[3 * TSDF_STORE_BV + 3 * lv + 1] = w[4];
        brick[3 * TSDF_STORE_BV + 3 * lv + 2] = w[5];
    }
    if constexpr (FS) brick[(COL ? 6 : 2) * TSDF_STORE_BV + lv] = w[6];
}

__device__ __forceinline__ uint32_t store_any(const uint32_t (&w)[TSDF_STORE_MAX_WORDS]) {
    return ((w[0] | w[1]) | (w[2] | w[3])) | ((w[4] | w[5]) | w[6]);
}

template <bool COL, bool FS>
__global__ __launch_bounds__(256) void k_tsdf_store_out(TsdfLayers l, const TsdfWindow* __restrict__ win, TsdfStore st) {
    int d[3] = {win->delta[0], win->delta[1], win->delta[2]};
    if ((d[0] | d[1] | d[2]) == 0) return;
    const StoreView sv = store_view<COL, FS>(l, st);
    if (!sv.ok) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) st.ctr->moves += 1;
    const int n[3] = {l.nx, l.ny, l.nz};
    // shift already includes delta: the window before the move
    const int lo[3] = {win->shift[0] - d[0], win->shift[1] - d[1], win->shift[2] - d[2]};
    d[0] = store_clamp(d[0], n[0]), d[1] = store_clamp(d[1], n[1]), d[2] = store_clamp(d[2], n[2]);
    int b0[3], nb[3], loc[3];
    const int64_t total = store_extent(lo, n, b0, nb, loc);
    const int lane = threadIdx.x & 63, x = lane & 7, y = lane >> 3;
    const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), wn = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t t = w0; t < total; t += wn) {
        const StoreBrick b = store_brick(t, b0, nb, loc, n, d, -1);
        if (!b.touched) continue;
        const int i = b.i0 + x, j = b.j0 + y;
        const bool in_xy = i >= 0 && i < n[0] && j >= 0 && j < n[1];
        const bool out_xy = in_xy && (store_outside(i, -d[0], n[0]) || store_outside(j, -d[1], n[1]));
        uint32_t w[TSDF_STORE_B][TSDF_STORE_MAX_WORDS] = {};
#pragma unroll
        for (int r = 0; r < TSDF_STORE_B; ++r) {   // the leaving voxels' words, all loads before the first use
            const int k = b.k0 + r;
            if (in_xy && k >= 0 && k < n[2] && (out_xy || store_outside(k, -d[2], n[2])))
                store_load_window<COL, FS>(sv, ((int64_t)k * n[1] + j) * n[0] + i, w[r]);
        }
        unsigned bits = 0;   // bit r: voxel (x, y, r) leaves and has a non-zero word
#pragma unroll
        for (int r = 0; r < TSDF_STORE_B; ++r)
            if (store_any(w[r])) bits |= 1u << r;
        const int count = store_count(bits);
        if (count == 0) continue;
        int slot = -1;
        if (lane == 0 && store_coord_ok(b.bx) && store_coord_ok(b.by) && store_coord_ok(b.bz))
            slot = store_find_or_insert(st, store_key(b.bx, b.by, b.bz));
        slot = __shfl(slot, 0);
        if (slot < 0) {
            if (lane == 0) atomicAdd(&st.ctr->dropped, (unsigned long long)count);
            continue;
        }
        uint32_t* brick = st.pool + (int64_t)slot * st.wpv * TSDF_STORE_BV;
#pragma unroll
        for (int r = 0; r < TSDF_STORE_B; ++r)
            if ((bits >> r) & 1u) store_save_pool<COL, FS>(sv, brick, r * 64 + lane, w[r]);
        if (lane == 0) st.occ[slot] += count;
    }
}

template <bool COL, bool FS>
__global__ __launch_bounds__(256) void k_tsdf_store_in(TsdfLayers l, const TsdfWindow* __restrict__ win, TsdfStore st) {
    int d[3] = {win->delta[0], win->delta[1], win->delta[2]};
    if ((d[0] | d[1] | d[2]) == 0) return;
    const StoreView sv = store_view<COL, FS>(l, st);
    if (!sv.ok) return;
    const int n[3] = {l.nx, l.ny, l.nz};
    const int lo[3] = {win->shift[0], win->shift[1], win->shift[2]};   // the window after the move
    d[0] = store_clamp(d[0], n[0]), d[1] = store_clamp(d[1], n[1]), d[2] = store_clamp(d[2], n[2]);
    int b0[3], nb[3], loc[3];
    const int64_t total = store_extent(lo, n, b0, nb, loc);
    const int lane = threadIdx.x & 63, x = lane & 7, y = lane >> 3;
    const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), wn = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t t = w0; t < total; t += wn) {
        const StoreBrick b = store_brick(t, b0, nb, loc, n, d, +1);
        if (!b.touched) continue;
        int slot = -1;
        if (lane == 0 && store_coord_ok(b.bx) && store_coord_ok(b.by) && store_coord_ok(b.bz)) {
            slot = store_find(st, store_key(b.bx, b.by, b.bz));
            if (slot >= 0 && st.occ[slot] <= 0) slot = -1;   // an empty brick has nothing to give
        }
        slot = __shfl(slot, 0);
        if (slot < 0) continue;
        uint32_t* brick = st.pool + (int64_t)slot * st.wpv * TSDF_STORE_BV;
        const int i = b.i0 + x, j = b.j0 + y;
        const bool in_xy = i >= 0 && i < n[0] && j >= 0 && j < n[1];
        const bool new_xy = in_xy && (store_outside(i, d[0], n[0]) || store_outside(j, d[1], n[1]));
        uint32_t w[TSDF_STORE_B][TSDF_STORE_MAX_WORDS] = {};
#pragma unroll
        for (int r = 0; r < TSDF_STORE_B; ++r) {   // the entering voxels' stored words
            const int k = b.k0 + r;
            if (in_xy && k >= 0 && k < n[2] && (new_xy || store_outside(k, d[2], n[2]))) store_load_pool<COL, FS>(sv, brick, r * 64 + lane, w[r]);
        }
        unsigned bits = 0;   // bit r: voxel (x, y, r) entered and the pool had a non-zero word for it
#pragma unroll
        for (int r = 0; r < TSDF_STORE_B; ++r) {
            if (!store_any(w[r])) continue;
            bits |= 1u << r;
            store_save_window<COL, FS>(sv, ((int64_t)(b.k0 + r) * n[1] + j) * n[0] + i, w[r]);   // the window's voxel is zero after the move
            const uint32_t zero[TSDF_STORE_MAX_WORDS] = {};
            store_save_pool<COL, FS>(sv, brick, r * 64 + lane, zero);
        }
        const int count = store_count(bits);
        if (lane == 0 && count) st.occ[slot] -= count;
    }
}

// a bounded grid, as the move's: one wave per brick the window can overlap, at most 2048 blocks
#define TSDF_STORE_BLOCKS 2048
static unsigned store_blocks(const TsdfLayers& l) {
    const int64_t bricks = store_bricks_along(l.nx) * store_bricks_along(l.ny) * store_bricks_along(l.nz);
    return (unsigned)std::min<int64_t>((bricks + 3) / 4, TSDF_STORE_BLOCKS);
}

// the instantiation for the layers of the call: n = 2 (tsdf, weight), 3 (+ free-space), 4 (+ colour), 5 (both)
#define STORE_LAUNCH(K)                                                                                        \
    do {                                                                                                       \
        const dim3 g(store_blocks(l)), b(256);                                                                 \
        switch (l.n) {                                                                                         \
            case 2: hipLaunchKernelGGL((K<false, false>), g, b, 0, s, l, win, st); break;                     \
            case 3: hipLaunchKernelGGL((K<false, true>), g, b, 0, s, l, win, st); break;                      \
            case 4: hipLaunchKernelGGL((K<true, false>), g, b, 0, s, l, win, st); break;                      \
            default: hipLaunchKernelGGL((K<true, true>), g, b, 0, s, l, win, st); break;                      \
        }                                                                                                      \
    } while (0)

void launch_tsdf_store_out(const TsdfLayers& l, const TsdfWindow* win, const TsdfStore& st, hipStream_t s) { STORE_LAUNCH(k_tsdf_store_out); }

void launch_tsdf_store_in(const TsdfLayers& l, const TsdfWindow* win, const TsdfStore& st, hipStream_t s) { STORE_LAUNCH(k_tsdf_store_in); }
