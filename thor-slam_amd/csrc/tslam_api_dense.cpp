// tslam_api_dense.cpp — the outputs of the dense map on the host side: marching-cubes mesh, ESDF and
// ESDF slice of the TSDF volume (tslam_api_tsdf.cpp).
#include <algorithm>
#include <cmath>
#include <vector>

#include "tslam_handle.h"

extern "C" {

// -- dense-map outputs: marching-cubes mesh, ESDF, 2-D ESDF slice (k_dense.hip) ------------------
static DenseArgs dense_args(const tslam_handle* h, double min_weight) {
    const TsdfArgs& t = h->tsdf;
    DenseArgs a{};
    a.tsdf = t.tsdf;
    a.weight = t.weight;
    a.nx = t.nx;
    a.ny = t.ny;
    a.nz = t.nz;
    a.n_cubes = (t.nx > 1 && t.ny > 1 && t.nz > 1) ? (uint32_t)((int64_t)(t.nx - 1) * (t.ny - 1) * (t.nz - 1)) : 0u;
    a.n_voxels = (int64_t)t.nx * t.ny * t.nz;
    a.ox = t.ox;
    a.oy = t.oy;
    a.oz = t.oz;
    a.s = t.s;
    a.sf = (float)t.s;
    a.min_weight = (float)min_weight;
    a.color = h->tsdf_color ? t.col : nullptr;
    return a;
}

int tslam_mesh_extract(tslam_handle* h, double min_weight, int64_t* n_tris, void* stream) {
    if (!h || !h->tsdf_on) return no_volume();
    BA_FLUSH(h);
    if (!(min_weight >= 0.0)) return fail(TSLAM_EINVAL, "min_weight must be >= 0");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    DenseArgs a = dense_args(h, min_weight);
    if (h->d_tsdf_win) {   // vertices in the tracking world: the window's corner as the device has it
        int32_t sh[3];
        double o[3];
        if (const int rc = window_read(h, s, sh, o); rc != TSLAM_OK) return rc;
        a.ox = o[0];
        a.oy = o[1];
        a.oz = o[2];
    }
    h->mesh_n = 0;
    if (a.n_cubes == 0) {
        if (n_tris) *n_tris = 0;
        return TSLAM_OK;
    }
    const size_t nb = (a.n_cubes + 255) / 256;
    size_t cap = h->mesh_cubes_cap;
    if (cap < a.n_cubes) {   // the three scratch arrays follow the cube count
        int rc = dev_grow(h, (void**)&h->d_mesh_cfg, a.n_cubes);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_mesh_bsum, sizeof(uint32_t) * nb);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_mesh_boff, sizeof(uint64_t) * (nb + 1));
        if (rc != TSLAM_OK) return rc;
        h->mesh_cubes_cap = a.n_cubes;
    }
    launch_mesh_count(a, h->d_mesh_cfg, h->d_mesh_bsum, h->d_mesh_boff, h->d_mesh_boff + nb, s);
    HIPCHK(hipGetLastError());
    uint64_t total = 0;   // the buffer is sized to the count: one small read back
    HIPCHK(hipMemcpyAsync(&total, h->d_mesh_boff + nb, sizeof(total), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if ((int64_t)total > h->mesh_tris_cap || (a.color && !h->d_mesh_cols)) {
        const int64_t want = std::max((int64_t)total + (int64_t)total / 4 + 1024, h->mesh_tris_cap);
        int rc = dev_grow(h, (void**)&h->d_mesh_tris, sizeof(float) * 9 * (size_t)want);
        if (rc == TSLAM_OK && a.color) rc = dev_grow(h, (void**)&h->d_mesh_cols, sizeof(float) * 9 * (size_t)want);
        if (rc != TSLAM_OK) return rc;
        h->mesh_tris_cap = want;
    }
    launch_mesh_emit(a, h->d_mesh_cfg, h->d_mesh_boff, h->d_mesh_tris, h->d_mesh_cols, h->mesh_tris_cap, s);
    HIPCHK(hipGetLastError());
    h->mesh_n = (int64_t)total;
    if (n_tris) *n_tris = (int64_t)total;
    return TSLAM_OK;
}

int tslam_mesh_read_colors(tslam_handle* h, float* colors, int64_t max_tris) {
    if (!h || !h->tsdf_on || !h->tsdf_color || !h->d_mesh_cols) return fail(TSLAM_ESTATE, "no colour layer mesh");
    if (max_tris < 0 || (max_tris > 0 && !colors)) return fail(TSLAM_EINVAL, "bad buffer");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const int64_t n = std::min(max_tris, h->mesh_n);
    if (n > 0) HIPCHK(hipMemcpy(colors, h->d_mesh_cols, sizeof(float) * 9 * (size_t)n, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_mesh_read(tslam_handle* h, float* tris, int64_t max_tris) {
    if (!h || !h->tsdf_on) return no_volume();
    if (max_tris < 0 || (max_tris > 0 && !tris)) return fail(TSLAM_EINVAL, "bad buffer");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const int64_t n = std::min(max_tris, h->mesh_n);
    if (n > 0) HIPCHK(hipMemcpy(tris, h->d_mesh_tris, sizeof(float) * 9 * (size_t)n, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

// f32 distance of every squared voxel distance 0..R^2 (sqrt in f32, times s in f32, IEEE on the host)
static int dist_table(tslam_handle* h, int R, double s) {
    if (h->dist_tab_R == R && h->dist_tab_s == s && h->d_dist_tab) return TSLAM_OK;
    const size_t n = (size_t)R * R + 1;
    std::vector<float> tab(n);
    const float sf = (float)s;
    for (size_t d = 0; d < n; ++d) tab[d] = std::sqrt((float)d) * sf;
    const int rc = dev_grow(h, (void**)&h->d_dist_tab, sizeof(float) * n);
    if (rc != TSLAM_OK) return rc;
    HIPCHK(hipMemcpy(h->d_dist_tab, tab.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    h->dist_tab_R = R;
    h->dist_tab_s = s;
    return TSLAM_OK;
}

static int esdf_setup(tslam_handle* h, double max_dist, double site_vox, double min_weight, size_t cells, DenseArgs* a,
                      int* R) {
    if (!h || !h->tsdf_on) return no_volume();
    if (!(max_dist > 0.0) || !(site_vox >= 0.0) || !(min_weight >= 0.0))
        return fail(TSLAM_EINVAL, "max_dist must be > 0, site_vox and min_weight >= 0");
    const double r = std::floor(max_dist / h->tsdf.s + 1e-9);
    if (r < 0.0 || r > 2048.0) return fail(TSLAM_EINVAL, "max_dist / voxel_size must be at most 2048 voxels");
    HIPCHK(hipSetDevice(h->device));
    *R = (int)r;
    *a = dense_args(h, min_weight);
    a->site_dist = (float)(site_vox * h->tsdf.s);
    a->max_dist = (float)max_dist;
    a->cap = *R * *R + 1;
    int rc = dist_table(h, *R, h->tsdf.s);
    if (rc == TSLAM_OK && h->edt_cap < cells) {
        rc = dev_grow(h, (void**)&h->d_edt[0], sizeof(int32_t) * cells);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_edt[1], sizeof(int32_t) * cells);
        h->edt_cap = rc == TSLAM_OK ? cells : 0;
    }
    return rc;
}

int tslam_esdf_compute(tslam_handle* h, double max_dist, double site_vox, double min_weight, void* stream) {
    DenseArgs a;
    int R = 0;
    const size_t nv = h && h->tsdf_on ? tsdf_voxels(h) : 0;
    int rc = esdf_setup(h, max_dist, site_vox, min_weight, nv, &a, &R);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_esdf, sizeof(float) * nv, &h->esdf_cap);
    if (rc != TSLAM_OK) return rc;
    hipStream_t s = call_stream(h, stream);
    launch_esdf(a, R, h->d_dist_tab, h->d_edt[0], h->d_edt[1], h->d_esdf, s);
    HIPCHK(hipGetLastError());
    h->esdf_valid = true;
    return TSLAM_OK;
}

int tslam_esdf_read(tslam_handle* h, float* esdf) {
    if (!h || !h->tsdf_on || !h->esdf_valid) return fail(TSLAM_ESTATE, "no ESDF (tslam_esdf_compute)");
    if (!esdf) return fail(TSLAM_EINVAL, "null buffer");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = tsdf_voxels(h);
    HIPCHK(hipMemcpy(esdf, h->d_esdf, sizeof(float) * nv, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_esdf_slice(tslam_handle* h, int y0, int y1, double max_dist, double site_vox, double min_weight, float* out) {
    if (!h || !h->tsdf_on) return no_volume();
    if (!out || y0 < 0 || y1 <= y0 || y1 > h->tsdf.ny) return fail(TSLAM_EINVAL, "need 0 <= y0 < y1 <= ny and a buffer");
    DenseArgs a;
    int R = 0;
    const size_t nc = (size_t)h->tsdf.nx * h->tsdf.nz;
    int rc = esdf_setup(h, max_dist, site_vox, min_weight, nc, &a, &R);
    if (rc == TSLAM_OK && h->slice_cap < nc) {
        rc = dev_grow(h, (void**)&h->d_slice_obs, nc);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_slice, sizeof(float) * nc);
        h->slice_cap = rc == TSLAM_OK ? nc : 0;
    }
    if (rc != TSLAM_OK) return rc;
    hipStream_t s = h->last_stream;
    launch_esdf_slice(a, y0, y1, R, h->d_dist_tab, h->d_edt[0], h->d_edt[1], h->d_slice_obs, h->d_slice, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(out, h->d_slice, sizeof(float) * nc, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

}  // extern "C"
