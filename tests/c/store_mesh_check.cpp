// store_mesh_check.cpp — the whole-map mesh's host arithmetic
// (thor-slam_amd/csrc/tslam_tsdf_store_mesh.h) in an executable of its own, built with
// AddressSanitizer + UBSan (`make sanitize`, or `make build-asan/store_mesh_check`): the window's brick
// range, the "outside that range" test, the per-voxel source of a brick's 9 x 9 x 9 corner tile and
// the list's order, each against a per-voxel brute force, over windows that lie below zero, whose
// edges cut bricks on each axis, and that are narrower than a brick.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <tuple>
#include <vector>

#include "../../thor-slam_amd/csrc/tslam_tsdf_store_mesh.h"

static long cases = 0;

#define CHECK(c)                                                               \
    do {                                                                       \
        ++cases;                                                               \
        if (!(c)) {                                                            \
            std::fprintf(stderr, "store_mesh_check %d: %s\n", __LINE__, #c);   \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

// floor division the slow way
static int64_t floor8(int64_t a) {
    int64_t b = 0;
    while (8 * b > a) --b;
    while (8 * (b + 1) <= a) ++b;
    return b;
}

typedef std::tuple<int64_t, int64_t, int64_t> Brick;   // (bz, by, bx): the list's order

// one window: every function of the header against the voxels themselves
static void check_window(const int32_t lo[3], const int32_t n[3]) {
    const WmeshRange r = wmesh_window_range(lo, n);
    // the range: exactly the bricks of the window's voxels
    std::set<Brick> want;
    for (int64_t z = lo[2]; z < (int64_t)lo[2] + n[2]; ++z)
        for (int64_t y = lo[1]; y < (int64_t)lo[1] + n[1]; ++y)
            for (int64_t x = lo[0]; x < (int64_t)lo[0] + n[0]; ++x) want.insert(Brick(floor8(z), floor8(y), floor8(x)));
    CHECK(wmesh_range_count(r) == (int64_t)want.size());
    for (int a = 0; a < 3; ++a) CHECK(r.nb[a] >= 1 && r.nb[a] <= store_bricks_along(n[a]));
    std::set<Brick> got;
    std::vector<uint64_t> keys;
    for (int64_t t = 0; t < wmesh_range_count(r); ++t) {
        int32_t b[3];
        wmesh_range_brick(r, t, b);
        CHECK(got.insert(Brick(b[2], b[1], b[0])).second);
        CHECK(!wmesh_outside(r, b) && wmesh_brick_ok(b));
        keys.push_back(store_key(b[0], b[1], b[2]));
    }
    CHECK(got == want);
    // outside: every brick around the range that is not one of its own
    for (int32_t bz = r.b0[2] - 2; bz < r.b0[2] + r.nb[2] + 2; ++bz)
        for (int32_t by = r.b0[1] - 2; by < r.b0[1] + r.nb[1] + 2; ++by)
            for (int32_t bx = r.b0[0] - 2; bx < r.b0[0] + r.nb[0] + 2; ++bx) {
                const int32_t b[3] = {bx, by, bz};
                const bool own = want.count(Brick(bz, by, bx)) != 0;
                CHECK(wmesh_outside(r, b) == !own);
                if (!own) keys.push_back(store_key(bx, by, bz));
                // whole in the window: all 512 voxels are
                bool whole = true;
                for (int a = 0; a < 3; ++a)
                    for (int v = 0; v < 8; ++v) whole = whole && 8 * (int64_t)b[a] + v >= lo[a] && 8 * (int64_t)b[a] + v < (int64_t)lo[a] + n[a];
                CHECK(wmesh_brick_in_window(b, lo, n) == whole);
            }
    // the list's order: shuffled keys come back in ascending (bz, by, bx), none lost
    std::vector<uint64_t> sorted = keys;
    for (size_t i = sorted.size(); i > 1; --i) std::swap(sorted[i - 1], sorted[(size_t)std::rand() % i]);
    wmesh_sort(sorted.data(), (int64_t)sorted.size());
    CHECK(sorted.size() == keys.size());
    for (size_t i = 1; i < sorted.size(); ++i) {
        int32_t p[3], q[3];
        store_key_coords(sorted[i - 1], p);
        store_key_coords(sorted[i], q);
        CHECK(Brick(p[2], p[1], p[0]) < Brick(q[2], q[1], q[0]));
    }
    wmesh_sort(sorted.data(), 0);
    // the per-voxel source of the tiles of the range's bricks and of their neighbours below
    for (int32_t bz = r.b0[2] - 1; bz < r.b0[2] + r.nb[2]; ++bz)
        for (int32_t by = r.b0[1] - 1; by < r.b0[1] + r.nb[1]; ++by)
            for (int32_t bx = r.b0[0] - 1; bx < r.b0[0] + r.nb[0]; ++bx) {
                const int32_t b[3] = {bx, by, bz};
                std::set<int64_t> seen;   // a window voxel is the source of one tile voxel
                for (int tz = 0; tz < WMESH_T; ++tz)
                    for (int ty = 0; ty < WMESH_T; ++ty)
                        for (int tx = 0; tx < WMESH_T; ++tx) {
                            const int64_t a[3] = {8 * (int64_t)bx + tx, 8 * (int64_t)by + ty, 8 * (int64_t)bz + tz};
                            bool in = true;
                            for (int c = 0; c < 3; ++c) in = in && a[c] >= lo[c] && a[c] < (int64_t)lo[c] + n[c];
                            const WmeshSource s = wmesh_source(b, tx, ty, tz, lo, n);
                            CHECK(s.window == in);
                            if (in) {
                                CHECK(s.index == ((a[2] - lo[2]) * n[1] + (a[1] - lo[1])) * n[0] + (a[0] - lo[0]));
                                CHECK(s.index >= 0 && s.index < (int64_t)n[0] * n[1] * n[2]);
                                CHECK(seen.insert(s.index).second);
                            } else {
                                CHECK(s.brick >= 0 && s.brick < 8 && s.index >= 0 && s.index < TSDF_STORE_BV);
                                const int64_t sb[3] = {bx + (s.brick & 1), by + ((s.brick >> 1) & 1), bz + (s.brick >> 2)};
                                for (int c = 0; c < 3; ++c) CHECK(sb[c] == floor8(a[c]));
                                const int64_t l[3] = {a[0] - 8 * sb[0], a[1] - 8 * sb[1], a[2] - 8 * sb[2]};
                                CHECK(s.index == (l[2] * 8 + l[1]) * 8 + l[0]);
                                const int32_t sb32[3] = {(int32_t)sb[0], (int32_t)sb[1], (int32_t)sb[2]};
                                CHECK(!wmesh_brick_in_window(sb32, lo, n));   // a brick the window holds whole is never a source
                            }
                        }
            }
}

int main() {
    std::srand(11);
    const int32_t dims[][3] = {{13, 9, 11}, {8, 8, 8}, {3, 1, 5}, {1, 1, 1}, {16, 7, 9}, {21, 13, 19}};
    const int32_t los[][3] = {{0, 0, 0}, {-5, 3, -9}, {-16, -8, -24}, {-1, -7, -8}, {5, -3, 9}, {-37, 12, -2}, {7, 7, 7}};
    for (const auto& n : dims)
        for (const auto& lo : los) check_window(lo, n);
    // an edge on each axis in turn cuts a brick, the others lie on the grid
    for (int a = 0; a < 3; ++a)
        for (int cut = 1; cut < 8; ++cut) {
            int32_t lo[3] = {-8, -16, 8}, n[3] = {16, 8, 8};
            lo[a] += cut;
            check_window(lo, n);
            lo[a] -= cut;
            n[a] += cut;
            check_window(lo, n);
        }
    // far from zero, at the shift limit and at the key's coordinate limit
    const int32_t far_lo[3] = {-(1 << 30) + 1, (1 << 30) - 40, -8 * TSDF_STORE_COORD_LIMIT}, far_n[3] = {5, 37, 9};
    const WmeshRange r = wmesh_window_range(far_lo, far_n);
    CHECK(r.b0[0] == -(1 << 27) && r.nb[0] == 1 && r.b0[2] == -TSDF_STORE_COORD_LIMIT && r.nb[2] == 2);
    int32_t b[3];
    wmesh_range_brick(r, wmesh_range_count(r) - 1, b);
    CHECK(b[0] == r.b0[0] && b[1] == r.b0[1] + r.nb[1] - 1 && b[2] == r.b0[2] + 1);
    CHECK(!wmesh_brick_ok(b));                       // x and y have no key
    const int32_t edge[3] = {TSDF_STORE_COORD_LIMIT - 1, -TSDF_STORE_COORD_LIMIT, 0}, past[3] = {TSDF_STORE_COORD_LIMIT, 0, 0};
    CHECK(wmesh_brick_ok(edge) && !wmesh_brick_ok(past));
    const WmeshSource s = wmesh_source(b, 8, 8, 8, far_lo, far_n);
    CHECK(!s.window && s.brick == 7 && s.index == 0);
    std::printf("store mesh: %ld cases\n", cases);
    return 0;
}
