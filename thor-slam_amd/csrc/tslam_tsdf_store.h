// tslam_tsdf_store.h — the brick store's arithmetic (thor_slam_amd/dense_store.py), shared by the
// kernels (k_tsdf_store.hip), the host side (tslam_api_store.cpp) and the sanitized host check
// (tests/c/store_check.cpp): absolute voxel -> store brick and local index, the table's 64-bit keys,
// the probe's first cell, and the read-out's order.  No HIP types: it compiles as plain C++.
#ifndef TSLAM_TSDF_STORE_H
#define TSLAM_TSDF_STORE_H

#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define TS_STORE_HD __host__ __device__
#else
#define TS_STORE_HD
#endif

#define TSDF_STORE_B 8                        // store bricks are 8 x 8 x 8 voxels
#define TSDF_STORE_BV 512                     // voxels of a brick
#define TSDF_STORE_COORD_LIMIT (1 << 20)      // a brick coordinate b is stored for -2^20 <= b < 2^20
#define TSDF_STORE_MAX_WORDS 7                // tsdf, weight, colour weight, colour (3), free-space

// floor(a / 8) and a - 8 floor(a / 8), for negative a too (an arithmetic shift and a mask)
TS_STORE_HD static inline int64_t store_brick_of(int64_t a) { return a >> 3; }
TS_STORE_HD static inline int store_local_of(int64_t a) { return (int)(a & 7); }

TS_STORE_HD static inline bool store_coord_ok(int64_t b) { return b >= -(int64_t)TSDF_STORE_COORD_LIMIT && b < (int64_t)TSDF_STORE_COORD_LIMIT; }

// three 21-bit biased coordinates and the occupied bit (63): never 0, which is an empty cell
TS_STORE_HD static inline uint64_t store_key(int64_t bx, int64_t by, int64_t bz) {
    const uint64_t x = (uint64_t)(bx + TSDF_STORE_COORD_LIMIT), y = (uint64_t)(by + TSDF_STORE_COORD_LIMIT),
                   z = (uint64_t)(bz + TSDF_STORE_COORD_LIMIT);
    return ((uint64_t)1 << 63) | (z << 42) | (y << 21) | x;
}

TS_STORE_HD static inline void store_key_coords(uint64_t key, int32_t b[3]) {
    b[0] = (int32_t)(key & 0x1fffff) - TSDF_STORE_COORD_LIMIT;
    b[1] = (int32_t)((key >> 21) & 0x1fffff) - TSDF_STORE_COORD_LIMIT;
    b[2] = (int32_t)((key >> 42) & 0x1fffff) - TSDF_STORE_COORD_LIMIT;
}

// the probe's first cell (a 64-bit finaliser; `mask` = cells - 1, cells a power of two)
TS_STORE_HD static inline uint32_t store_hash(uint64_t key, uint32_t mask) {
    key ^= key >> 33;
    key *= 0xff51afd7ed558ccdULL;
    key ^= key >> 33;
    key *= 0xc4ceb9fe1a85ec53ULL;
    key ^= key >> 33;
    return (uint32_t)key & mask;
}

// cells of the table for a pool of `capacity` bricks: the power of two >= 2 * capacity (at least 2),
// so at most half the cells are ever taken and a probe always ends at an empty cell
static inline int64_t store_cells(int64_t capacity) {
    int64_t c = 2;
    while (c < 2 * capacity) c <<= 1;
    return c;
}

// bricks along one axis that an interval of `dim` voxels can overlap, wherever it lies
static inline int64_t store_bricks_along(int64_t dim) { return (dim + 6) / 8 + 1; }

// The read-out: the table's cells whose brick holds a voxel (occ[slot] > 0), in ascending
// (bz, by, bx) — which is the keys' numeric order.  -> (key, slot) pairs.
struct StoreEntry {
    uint64_t key;
    int32_t slot;
};
static inline std::vector<StoreEntry> store_content(const uint64_t* keys, const int32_t* vals, int64_t cells,
                                                    const int32_t* occ, int64_t allocated) {
    std::vector<StoreEntry> out;
    for (int64_t c = 0; c < cells; ++c) {
        if (!keys[c]) continue;
        const int32_t slot = vals[c];
        if (slot < 0 || slot >= allocated || occ[slot] <= 0) continue;
        out.push_back({keys[c], slot});
    }
    std::sort(out.begin(), out.end(), [](const StoreEntry& a, const StoreEntry& b) { return a.key < b.key; });
    return out;
}

#endif
