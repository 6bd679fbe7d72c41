// tslam_tsdf_store_mesh.h — the arithmetic of the whole-map mesh (thor_slam_amd/dense_store.py,
// "The mesh of the whole map"), shared by the kernels (k_tsdf_store_mesh.hip), the host side
// (tslam_api_store_mesh.cpp) and the sanitized host check (tests/c/store_mesh_check.cpp): the store
// bricks the window's extent overlaps, the "outside that range" test of a table entry, where an
// absolute voxel's value comes from (a window index, a place in one of the 8 source bricks of a
// 9 x 9 x 9 corner tile, or nowhere), and the order of the brick list.  No HIP types: plain C++.
#ifndef TSLAM_TSDF_STORE_MESH_H
#define TSLAM_TSDF_STORE_MESH_H

#include "tslam_tsdf_store.h"

#define WMESH_T 9                // a brick's cubes read a 9 x 9 x 9 tile of corners
#define WMESH_TV 729             // voxels of the tile
#define WMESH_IN_WINDOW (-2)     // a source brick that lies in the window whole: no table look-up

// the bricks the window [lo, lo + n) overlaps: b0 .. b0 + nb - 1 per axis (n >= 1)
struct WmeshRange {
    int32_t b0[3], nb[3];
};

TS_STORE_HD static inline WmeshRange wmesh_window_range(const int32_t lo[3], const int32_t n[3]) {
    WmeshRange r;
    for (int a = 0; a < 3; ++a) {
        r.b0[a] = (int32_t)store_brick_of(lo[a]);
        r.nb[a] = (int32_t)(store_brick_of((int64_t)lo[a] + n[a] - 1) - r.b0[a] + 1);
    }
    return r;
}

TS_STORE_HD static inline int64_t wmesh_range_count(const WmeshRange& r) { return (int64_t)r.nb[0] * r.nb[1] * r.nb[2]; }

// brick t of the range, x fastest (0 <= t < wmesh_range_count)
TS_STORE_HD static inline void wmesh_range_brick(const WmeshRange& r, int64_t t, int32_t b[3]) {
    b[0] = r.b0[0] + (int32_t)(t % r.nb[0]);
    b[1] = r.b0[1] + (int32_t)((t / r.nb[0]) % r.nb[1]);
    b[2] = r.b0[2] + (int32_t)(t / ((int64_t)r.nb[0] * r.nb[1]));
}

// is brick b outside the window's brick range?  (a live table entry is listed when it is: the range's
// own bricks are listed by arithmetic, so no brick comes twice)
TS_STORE_HD static inline bool wmesh_outside(const WmeshRange& r, const int32_t b[3]) {
    for (int a = 0; a < 3; ++a)
        if (b[a] < r.b0[a] || (int64_t)b[a] >= (int64_t)r.b0[a] + r.nb[a]) return true;
    return false;
}

// a brick can be listed (and found in the table) when its key exists
TS_STORE_HD static inline bool wmesh_brick_ok(const int32_t b[3]) { return store_coord_ok(b[0]) && store_coord_ok(b[1]) && store_coord_ok(b[2]); }

// does brick b lie in the window whole?  Then none of its voxels is looked up in the store.
TS_STORE_HD static inline bool wmesh_brick_in_window(const int32_t b[3], const int32_t lo[3], const int32_t n[3]) {
    for (int a = 0; a < 3; ++a) {
        const int64_t a0 = (int64_t)TSDF_STORE_B * b[a];
        if (a0 < lo[a] || a0 + TSDF_STORE_B > (int64_t)lo[a] + n[a]) return false;
    }
    return true;
}

// Where tile voxel (tx, ty, tz), each 0..8, of listed brick b takes its value from: absolute voxel
// a = 8 b + t.  In the window (lo <= a < lo + n on every axis): `index` is its linear window index
// [k][j][i].  Otherwise: `brick` 0..7 says which of the source bricks b + (brick & 1, brick >> 1 & 1,
// brick >> 2) holds it (a window edge can cut a brick, so this is decided per voxel), `index` its
// local voxel [z][y][x] there, 0..511.
struct WmeshSource {
    bool window;
    int brick;
    int64_t index;
};

TS_STORE_HD static inline WmeshSource wmesh_source(const int32_t b[3], int tx, int ty, int tz, const int32_t lo[3], const int32_t n[3]) {
    const int t[3] = {tx, ty, tz};
    int64_t w[3];
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        w[a] = (int64_t)TSDF_STORE_B * b[a] + t[a] - lo[a];
        in = in && w[a] >= 0 && w[a] < n[a];
    }
    WmeshSource s;
    s.window = in;
    if (in) {
        s.brick = -1;
        s.index = (w[2] * n[1] + w[1]) * n[0] + w[0];
    } else {
        s.brick = (tx >> 3) | ((ty >> 3) << 1) | ((tz >> 3) << 2);
        s.index = (((tz & 7) * TSDF_STORE_B) + (ty & 7)) * TSDF_STORE_B + (tx & 7);
    }
    return s;
}

// the list's order: ascending keys, which is ascending (bz, by, bx)
static inline void wmesh_sort(uint64_t* keys, int64_t n) { std::sort(keys, keys + n); }

#endif
