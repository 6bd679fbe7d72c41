// tslam_api_store_mesh.cpp — the mesh of the whole dense map on the host side
// (tslam_mesh_extract_whole; k_tsdf_store_mesh.hip; thor_slam_amd/dense_store.py): the brick list is
// made and sorted here, the kernels' scratch lives in handle-owned buffers that grow on demand, and
// the triangles go to the buffers tslam_mesh_extract writes too.  Voxels and the table stay on the
// device: what crosses is the list's length, 8 B per listed brick each way, and the triangle count.
#include <algorithm>
#include <climits>

#include "tslam_handle.h"
#include "tslam_tsdf_store_mesh.h"

extern "C" {

int tslam_mesh_extract_whole(tslam_handle* h, double min_weight, int64_t* n_tris, int64_t* n_bricks, void* stream) {
    if (!h) return no_volume();
    if (const int rc = dense_open(h, "tslam_mesh_extract_whole", h->store_on, "no brick store (tslam_tsdf_store_init)"); rc != TSLAM_OK)
        return rc;
    if (!(min_weight >= 0.0)) return fail(TSLAM_EINVAL, "min_weight must be >= 0");
    const TsdfArgs& t = h->tsdf;
    const bool color = h->tsdf_color && t.col;
    if (!h->d_tsdf_win || h->store.wpv < (color ? 6 : 2)) return fail(TSLAM_ESTATE, "the brick store does not hold the volume's layers");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    WmeshArgs a{};
    a.tsdf = t.tsdf;
    a.weight = t.weight;
    a.color = color ? t.col : nullptr;
    a.nx = t.nx;
    a.ny = t.ny;
    a.nz = t.nz;
    a.ox = t.ox;   // the configured origin: the window's shift is not in it
    a.oy = t.oy;
    a.oz = t.oz;
    a.s = t.s;
    a.sf = (float)t.s;
    a.min_weight = (float)min_weight;
    a.win = h->d_tsdf_win;
    a.st = h->store;
    h->mesh_n = 0;
    if (n_tris) *n_tris = 0;
    if (n_bricks) *n_bricks = 0;

    // 1. the list: live bricks outside the window's range and the range's own bricks
    const int64_t max_window = store_bricks_along(t.nx) * store_bricks_along(t.ny) * store_bricks_along(t.nz);
    if (!h->d_wmesh_count)
        if (const int rc = dev_alloc(h, (void**)&h->d_wmesh_count, sizeof(uint32_t)); rc != TSLAM_OK) return rc;
    uint32_t n = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t want = pass == 0 ? max_window + 1024 : (int64_t)n + (int64_t)n / 4 + 1024;
        if (h->wmesh_list_cap < want) {
            if (const int rc = dev_grow(h, (void**)&h->d_wmesh_list, sizeof(uint64_t) * (size_t)want); rc != TSLAM_OK) {
                h->wmesh_list_cap = 0;
                return rc;
            }
            h->wmesh_list_cap = want;
        }
        HIPCHK(hipMemsetAsync(h->d_wmesh_count, 0, sizeof(uint32_t), s));
        launch_wmesh_list(a, h->store_cells, max_window, h->d_wmesh_list, h->wmesh_list_cap, h->d_wmesh_count, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&n, h->d_wmesh_count, sizeof(n), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if ((int64_t)n <= h->wmesh_list_cap) break;   // else the list was too short: once more, with room
    }
    if ((int64_t)n > h->wmesh_list_cap || n > (uint32_t)INT_MAX) return fail(TSLAM_EHIP, "the whole-map mesh's brick list did not settle");
    if (n == 0) return TSLAM_OK;
    if (const int rc = pinned_reserve(h, (void**)&h->wmesh_host, &h->wmesh_host_cap, sizeof(uint64_t) * (size_t)n); rc != TSLAM_OK) return rc;
    HIPCHK(hipMemcpyAsync(h->wmesh_host, h->d_wmesh_list, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    wmesh_sort(h->wmesh_host, (int64_t)n);
    HIPCHK(hipMemcpyAsync(h->d_wmesh_list, h->wmesh_host, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, s));

    // 2. the bricks' triangle totals and first triangles
    if (h->wmesh_bricks_cap < (int64_t)n) {
        const int64_t want = (int64_t)n + (int64_t)n / 4 + 1024;
        h->wmesh_bricks_cap = 0;
        int rc = dev_grow(h, (void**)&h->d_wmesh_bsum, sizeof(uint32_t) * (size_t)want);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_wmesh_boff, sizeof(uint64_t) * (size_t)(want + 1));
        if (rc != TSLAM_OK) return rc;
        h->wmesh_bricks_cap = want;
    }
    launch_wmesh_count(a, h->d_wmesh_list, n, h->d_wmesh_bsum, s);
    launch_mesh_scan(h->d_wmesh_bsum, (int)n, h->d_wmesh_boff, h->d_wmesh_boff + n, s);
    HIPCHK(hipGetLastError());
    uint64_t total = 0;   // the buffer is sized to the count: one small read back
    HIPCHK(hipMemcpyAsync(&total, h->d_wmesh_boff + n, sizeof(total), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));

    // 3. the triangles, into the buffers tslam_mesh_extract writes too
    if ((int64_t)total > h->mesh_tris_cap || !h->d_mesh_tris || (a.color && !h->d_mesh_cols)) {
        const int64_t want = std::max((int64_t)total + (int64_t)total / 4 + 1024, h->mesh_tris_cap);
        int rc = dev_grow(h, (void**)&h->d_mesh_tris, sizeof(float) * 9 * (size_t)want);
        if (rc == TSLAM_OK && a.color) rc = dev_grow(h, (void**)&h->d_mesh_cols, sizeof(float) * 9 * (size_t)want);
        if (rc != TSLAM_OK) return rc;
        h->mesh_tris_cap = want;
    }
    launch_wmesh_emit(a, h->d_wmesh_list, n, h->d_wmesh_boff, h->d_mesh_tris, h->d_mesh_cols, h->mesh_tris_cap, s);
    HIPCHK(hipGetLastError());
    h->mesh_n = (int64_t)total;
    if (n_tris) *n_tris = (int64_t)total;
    if (n_bricks) *n_bricks = (int64_t)n;
    return TSLAM_OK;
}

}  // extern "C"
