// tslam_api_store.cpp — the dense map's brick store on the host side (tslam_tsdf_store_*;
// k_tsdf_store.hip; thor_slam_amd/dense_store.py): the table, the pool and the counters are
// allocated here and live on the device; the moves (tslam_api_tsdf.cpp) hand them to the kernels.
// Only the two readers synchronise.
#include <climits>
#include <vector>

#include "tslam_handle.h"
#include "tslam_tsdf_store.h"

static const char* const NO_STORE = "no brick store (tslam_tsdf_store_init)";

// words per voxel of the layers the volume has now, in TsdfLayers' order
static int store_layer_words(const tslam_handle* h, int comp[5], int* n_layers) {
    int n = 0, w = 0;
    auto add = [&](int c) {
        comp[n++] = c;
        w += c;
    };
    add(1);
    add(1);
    if (h->tsdf.col) {
        add(1);
        add(3);
    }
    if (h->d_fs_words) add(1);
    *n_layers = n;
    return w;
}

static void store_free(tslam_handle* h) {
    TsdfStore& st = h->store;
    dev_release(h, (void**)&st.keys);
    dev_release(h, (void**)&st.vals);
    dev_release(h, (void**)&st.occ);
    dev_release(h, (void**)&st.pool);
    dev_release(h, (void**)&st.ctr);
    st = TsdfStore{};
    h->store_on = false;
    h->store_cells = 0;
    h->store_pool_bytes = 0;
}

// every stream is idle (the callers have quiesced): table, pool and counters to zero, and the
// bricks' layout from the layers of now.  A volume with more words per voxel than the pool was
// sized for (it cannot happen through the C ABI, which refuses to add a layer) ends the store.
int store_clear(tslam_handle* h) {
    if (!h->store_on) return TSLAM_OK;
    TsdfStore& st = h->store;
    int comp[5], nl;
    const int wpv = store_layer_words(h, comp, &nl);
    if (sizeof(uint32_t) * TSDF_STORE_BV * (size_t)wpv * (size_t)st.capacity > h->store_pool_bytes) {
        store_free(h);
        return TSLAM_OK;
    }
    st.wpv = wpv;
    HIPCHK(hipMemset(st.keys, 0, sizeof(unsigned long long) * (size_t)h->store_cells));
    HIPCHK(hipMemset(st.vals, 0, sizeof(int32_t) * (size_t)h->store_cells));
    HIPCHK(hipMemset(st.occ, 0, sizeof(int32_t) * (size_t)st.capacity));
    HIPCHK(hipMemset(st.pool, 0, h->store_pool_bytes));
    HIPCHK(hipMemset(st.ctr, 0, sizeof(TsdfStoreCounters)));
    HIPCHK(hipDeviceSynchronize());   // the null stream's memsets before any other stream's move
    return TSLAM_OK;
}

// the table, the occupancy and the counters as the device has them (everything has drained)
struct StoreHost {
    std::vector<uint64_t> keys;
    std::vector<int32_t> vals, occ;
    TsdfStoreCounters ctr{};
    int64_t allocated = 0;
};
static int store_fetch(tslam_handle* h, StoreHost& s) {
    const TsdfStore& st = h->store;
    HIPCHK(hipMemcpy(&s.ctr, st.ctr, sizeof(TsdfStoreCounters), hipMemcpyDeviceToHost));
    s.allocated = std::min<int64_t>(std::max<int64_t>(s.ctr.bricks, 0), st.capacity);
    s.keys.resize((size_t)h->store_cells);
    s.vals.resize((size_t)h->store_cells);
    s.occ.resize((size_t)std::max<int64_t>(s.allocated, 1));
    HIPCHK(hipMemcpy(s.keys.data(), st.keys, sizeof(uint64_t) * s.keys.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(s.vals.data(), st.vals, sizeof(int32_t) * s.vals.size(), hipMemcpyDeviceToHost));
    if (s.allocated) HIPCHK(hipMemcpy(s.occ.data(), st.occ, sizeof(int32_t) * (size_t)s.allocated, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

extern "C" {

int tslam_tsdf_store_init(tslam_handle* h, int64_t capacity_bricks) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_store_init"); rc != TSLAM_OK) return rc;
    if (capacity_bricks < 0) return fail(TSLAM_EINVAL, "capacity_bricks must be >= 0");
    if (capacity_bricks > 0 && h->arc_on) return fail(TSLAM_ESTATE, "the brick store does not run with the depth archive (tslam_tsdf_archive_init)");
    int comp[5], nl;
    const int wpv = store_layer_words(h, comp, &nl);
    // slots are int32 and the table's cell index is 32 bits: at most 2^30 bricks, 2^31 cells
    if (capacity_bricks > ((int64_t)1 << 30)) return fail(TSLAM_EINVAL, "capacity_bricks must be at most 2^30");
    HIPCHK(hipSetDevice(h->device));
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    store_free(h);
    if (capacity_bricks == 0) return TSLAM_OK;
    if (const int rc = window_alloc(h); rc != TSLAM_OK) return rc;   // the moves' record and scratch
    TsdfStore& st = h->store;
    const int64_t cells = store_cells(capacity_bricks);
    const size_t pool_bytes = sizeof(uint32_t) * TSDF_STORE_BV * (size_t)wpv * (size_t)capacity_bricks;
    int rc = dev_alloc(h, (void**)&st.keys, sizeof(unsigned long long) * (size_t)cells);   // dev_alloc zeroes
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&st.vals, sizeof(int32_t) * (size_t)cells);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&st.occ, sizeof(int32_t) * (size_t)capacity_bricks);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&st.pool, pool_bytes);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&st.ctr, sizeof(TsdfStoreCounters));
    if (rc != TSLAM_OK) {
        store_free(h);
        return rc;
    }
    st.capacity = (int32_t)capacity_bricks;
    st.mask = (uint32_t)(cells - 1);
    st.wpv = wpv;
    h->store_cells = cells;
    h->store_pool_bytes = pool_bytes;
    h->store_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_store_stats(tslam_handle* h, int64_t* out8) {
    if (!h || !out8) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = dense_open(h, "tslam_tsdf_store_stats", h->store_on, NO_STORE); rc != TSLAM_OK) return rc;
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    StoreHost s;
    if (const int rc = store_fetch(h, s); rc != TSLAM_OK) return rc;
    int64_t bricks = 0, voxels = 0;
    for (int64_t i = 0; i < s.allocated; ++i)
        if (s.occ[(size_t)i] > 0) {
            ++bricks;
            voxels += s.occ[(size_t)i];
        }
    out8[0] = h->store.capacity;
    out8[1] = s.allocated;
    out8[2] = bricks;
    out8[3] = voxels;
    out8[4] = (int64_t)s.ctr.dropped;
    out8[5] = (int64_t)s.ctr.moves;
    out8[6] = h->store.wpv;
    out8[7] = 0;
    return TSLAM_OK;
}

int tslam_tsdf_store_read(tslam_handle* h, int64_t max_bricks, int32_t* brick_xyz, uint32_t* words, int64_t* n_bricks) {
    if (!h || !n_bricks) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = dense_open(h, "tslam_tsdf_store_read", h->store_on, NO_STORE); rc != TSLAM_OK) return rc;
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    StoreHost s;
    if (const int rc = store_fetch(h, s); rc != TSLAM_OK) return rc;
    const std::vector<StoreEntry> content = store_content(s.keys.data(), s.vals.data(), h->store_cells, s.occ.data(), s.allocated);
    const int64_t n = (int64_t)content.size();
    *n_bricks = n;
    if (!brick_xyz && !words) return TSLAM_OK;   // the count only
    if (n > max_bricks) return fail(TSLAM_EINVAL, "max_bricks is below the store's content (*n_bricks)");
    if (brick_xyz)
        for (int64_t r = 0; r < n; ++r) store_key_coords(content[(size_t)r].key, brick_xyz + 3 * r);
    if (!words || n == 0) return TSLAM_OK;
    // slots are read in runs of 256 (one copy each); every brick goes to its rank, layer by layer
    // from [z][y][x][comp] to one [z][y][x] block per component
    int comp[5], nl;
    const int wpv = h->store.wpv;
    store_layer_words(h, comp, &nl);
    std::vector<int64_t> rank_of((size_t)s.allocated, -1);
    for (int64_t r = 0; r < n; ++r) rank_of[(size_t)content[(size_t)r].slot] = r;
    const size_t brick_words = (size_t)TSDF_STORE_BV * wpv;
    const int64_t RUN = 256;
    std::vector<uint32_t> stage((size_t)RUN * brick_words);
    for (int64_t s0 = 0; s0 < s.allocated; s0 += RUN) {
        const int64_t m = std::min(RUN, s.allocated - s0);
        bool any = false;
        for (int64_t i = 0; i < m; ++i) any = any || rank_of[(size_t)(s0 + i)] >= 0;
        if (!any) continue;
        HIPCHK(hipMemcpy(stage.data(), h->store.pool + (size_t)s0 * brick_words, sizeof(uint32_t) * (size_t)m * brick_words,
                         hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < m; ++i) {
            const int64_t r = rank_of[(size_t)(s0 + i)];
            if (r < 0) continue;
            const uint32_t* src = stage.data() + (size_t)i * brick_words;
            uint32_t* dst = words + (size_t)r * brick_words;
            int off = 0;
            for (int a = 0; a < nl; ++a) {
                for (int c = 0; c < comp[a]; ++c)
                    for (int v = 0; v < TSDF_STORE_BV; ++v)
                        dst[(size_t)(off + c) * TSDF_STORE_BV + v] = src[(size_t)off * TSDF_STORE_BV + (size_t)v * comp[a] + c];
                off += comp[a];
            }
        }
    }
    return TSLAM_OK;
}

}  // extern "C"
