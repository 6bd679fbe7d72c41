// store_check.cpp — the brick store's host arithmetic (thor-slam_amd/csrc/tslam_tsdf_store.h) in an
// executable of its own, built with AddressSanitizer + UBSan (`make sanitize`, or
// `make build-asan/store_check`): floor division and local indices against a per-voxel brute force,
// the keys' round trip at the coordinate limits, a sequential table with the kernels' probe rule
// (slot before key, nothing inserted at capacity) against a std::map, and the read-out's order.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "../../thor-slam_amd/csrc/tslam_tsdf_store.h"

static long cases = 0;

#define CHECK(c)                                                          \
    do {                                                                  \
        ++cases;                                                          \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "store_check %d: %s\n", __LINE__, #c);   \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

// the table as k_tsdf_store_out's lane 0 fills it, one brick at a time
struct Table {
    std::vector<uint64_t> keys;
    std::vector<int32_t> vals, occ;
    int32_t capacity, bricks = 0;
    uint32_t mask;
    explicit Table(int64_t cap) : keys((size_t)store_cells(cap), 0), vals(keys.size(), 0), occ((size_t)cap, 0), capacity((int32_t)cap),
                                  mask((uint32_t)(keys.size() - 1)) {}
    int find(uint64_t key) const {
        uint32_t c = store_hash(key, mask);
        for (uint32_t p = 0; p <= mask; ++p, c = (c + 1) & mask) {
            if (keys[c] == key) return vals[c];
            if (!keys[c]) return -1;
        }
        return -1;
    }
    int find_or_insert(uint64_t key) {
        uint32_t c = store_hash(key, mask);
        for (uint32_t p = 0; p <= mask; ++p, c = (c + 1) & mask) {
            if (keys[c] == key) return vals[c];
            if (keys[c]) continue;
            if (bricks >= capacity) return -1;
            keys[c] = key;
            vals[c] = bricks;
            return bricks++;
        }
        return -1;
    }
};

static void check_floor() {
    // the brute force: walk the voxels upwards from a brick border far below zero
    int64_t brick = -5, local = 0;
    for (int64_t a = -40; a <= 40; ++a) {
        CHECK(store_brick_of(a) == brick);
        CHECK(store_local_of(a) == local);
        CHECK(8 * store_brick_of(a) + store_local_of(a) == a);
        if (++local == 8) local = 0, ++brick;
    }
    const int64_t far = (int64_t)1 << 31;
    CHECK(store_brick_of(-far - 1) == -(far / 8) - 1 && store_local_of(-far - 1) == 7);
    CHECK(store_brick_of(far + 9) == far / 8 + 1 && store_local_of(far + 9) == 1);
    for (int64_t d = 1; d <= 64; ++d)   // bricks an interval of d voxels overlaps, at every offset
        for (int64_t lo = -16; lo < 16; ++lo) CHECK(store_brick_of(lo + d - 1) - store_brick_of(lo) + 1 <= store_bricks_along(d));
    CHECK(store_bricks_along(1) == 1 && store_bricks_along(2) == 2 && store_bricks_along(9) == 2 && store_bricks_along(10) == 3);
}

static void check_keys() {
    const int64_t L = TSDF_STORE_COORD_LIMIT;
    const int64_t edge[] = {-L, -L + 1, -9, -1, 0, 1, 8, L - 2, L - 1};
    std::map<uint64_t, std::tuple<int64_t, int64_t, int64_t>> seen;
    for (int64_t z : edge)
        for (int64_t y : edge)
            for (int64_t x : edge) {
                CHECK(store_coord_ok(x) && store_coord_ok(y) && store_coord_ok(z));
                const uint64_t k = store_key(x, y, z);
                CHECK(k != 0 && (k >> 63) == 1);
                int32_t b[3];
                store_key_coords(k, b);
                CHECK(b[0] == x && b[1] == y && b[2] == z);
                CHECK(seen.emplace(k, std::make_tuple(z, y, x)).second);
            }
    // the keys' numeric order is (bz, by, bx)
    const std::tuple<int64_t, int64_t, int64_t>* prev = nullptr;
    for (const auto& kv : seen) {
        if (prev) CHECK(*prev < kv.second);
        prev = &kv.second;
    }
    CHECK(!store_coord_ok(L) && !store_coord_ok(-L - 1));
    CHECK(store_cells(1) == 2 && store_cells(8) == 16 && store_cells(9) == 32 && store_cells(65536) == 131072);
}

static void check_table(int64_t cap, int n_bricks, unsigned seed) {
    Table t(cap);
    std::map<uint64_t, int> want;   // key -> slot
    std::srand(seed);
    int refused = 0;
    for (int i = 0; i < n_bricks; ++i) {
        const int64_t x = std::rand() % 7 - 3, y = std::rand() % 5 - 2, z = std::rand() % 9 - 4;
        const uint64_t k = store_key(x, y, z);
        const int slot = t.find_or_insert(k);
        auto it = want.find(k);
        if (it != want.end()) {
            CHECK(slot == it->second);
        } else if ((int64_t)want.size() < cap) {
            CHECK(slot == (int)want.size());
            want[k] = slot;
        } else {
            CHECK(slot == -1);
            ++refused;
        }
        if (slot >= 0) t.occ[(size_t)slot] += 1 + i % 3;
    }
    CHECK(t.bricks == (int)want.size());
    for (const auto& kv : want) CHECK(t.find(kv.first) == kv.second);
    CHECK(t.find(store_key(100, 100, 100)) == -1);
    if (n_bricks > 4 * cap) CHECK(refused > 0);
    // the read-out: bricks that hold a voxel, ascending; emptied bricks are not content
    int emptied = 0;
    for (size_t s = 0; s < t.occ.size(); s += 3)
        if (t.occ[s] > 0) t.occ[s] = 0, ++emptied;
    const std::vector<StoreEntry> got = store_content(t.keys.data(), t.vals.data(), (int64_t)t.keys.size(), t.occ.data(), t.bricks);
    CHECK((int)got.size() == t.bricks - emptied);
    size_t r = 0;
    for (const auto& kv : want) {   // std::map walks the keys in ascending order
        if (t.occ[(size_t)kv.second] <= 0) continue;
        CHECK(r < got.size() && got[r].key == kv.first && got[r].slot == kv.second);
        ++r;
    }
    CHECK(r == got.size());
}

int main() {
    check_floor();
    check_keys();
    check_table(8, 200, 1);        // 16 cells: collisions and a full pool
    check_table(1, 10, 2);
    check_table(64, 150, 3);
    check_table(1024, 4000, 4);
    std::printf("store: %ld cases\n", cases);
    return 0;
}
