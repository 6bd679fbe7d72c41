// tslam_api_dynamic.cpp — dynamic objects kept out of the dense map on the host side: the free-space
// depth mask (tslam_tsdf_dynamic*; k_tsdf_dynamic.hip; thor_slam_amd/dense_dynamic.py).
#include <cmath>

#include "tslam_handle.h"

static const char* const NO_DYNAMIC = "no dynamic-mask state (tslam_tsdf_dynamic_init)";

// the state's buffers go back to the device (tslam_tsdf_dynamic_init with NULL; a new volume)
void dynamic_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_dyn_poses, (void**)&h->d_dyn_wTc, (void**)&h->d_dyn_bits, (void**)&h->d_dyn_depth,
                     (void**)&h->d_dyn_mask, (void**)&h->d_dyn_stats})
        dev_release(h, p);
    h->dyn_on = false;
    h->dyn_frames = 0;
}

int dynamic_reset(tslam_handle* h) {
    if (!h->dyn_on) return TSLAM_OK;
    const size_t n = (size_t)h->W * h->H * h->dyn_frames;
    HIPCHK(hipMemset(h->d_dyn_depth, 0, sizeof(uint16_t) * n));
    HIPCHK(hipMemset(h->d_dyn_mask, 0, n));
    HIPCHK(hipMemset(h->d_dyn_stats, 0, sizeof(int32_t) * DYNAMIC_STATS * h->dyn_frames));
    return TSLAM_OK;
}

extern "C" {

int tslam_tsdf_dynamic_init(tslam_handle* h, int pair, int rect, const tslam_tsdf_dynamic_params* params, int max_frames) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_dynamic_init"); rc != TSLAM_OK) return rc;
    if (!params) {   // off: the buffers go back
        if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
        dynamic_off(h);
        return TSLAM_OK;
    }
    if (pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad pair");
    const tslam_tsdf_dynamic_params p = *params;
    if (!std::isfinite(p.min_free_weight) || !std::isfinite(p.free_fraction))
        return fail(TSLAM_EINVAL, "dynamic-mask parameters must be finite");
    if (!(p.min_free_weight > 0.0)) return fail(TSLAM_EINVAL, "min_free_weight must be > 0");
    if (!(p.free_fraction > 0.0 && p.free_fraction <= 1.0)) return fail(TSLAM_EINVAL, "free_fraction must be in (0, 1]");
    if (p.open_radius < 0 || p.open_radius > DYNAMIC_MAX_OPEN) return fail(TSLAM_EINVAL, "open_radius must be 0..4");
    if (p.dilate_radius < 0 || p.dilate_radius > DYNAMIC_MAX_DILATE) return fail(TSLAM_EINVAL, "dilate_radius must be 0..8");
    for (const int32_t r : p.reserved)
        if (r != 0) return fail(TSLAM_EINVAL, "reserved must be 0");
    if (max_frames < 1 || max_frames > TSDF_MAX_FRAMES) return fail(TSLAM_EINVAL, "max_frames must be 1..256");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    h->dyn_on = false;
    const size_t px = (size_t)h->W * h->H, n = (size_t)max_frames;
    const size_t words = (size_t)((h->W + 63) / 64) * h->H;
    int rc = TSLAM_OK;
    if (!h->d_dyn_poses) rc = dev_alloc(h, (void**)&h->d_dyn_poses, sizeof(double) * TSDF_MAX_FRAMES * TSDF_POSE);
    if (rc == TSLAM_OK && !h->d_dyn_wTc) rc = dev_alloc(h, (void**)&h->d_dyn_wTc, sizeof(double) * TSDF_MAX_FRAMES * 16);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_dyn_bits, sizeof(uint64_t) * 2 * words * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_dyn_depth, sizeof(uint16_t) * px * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_dyn_mask, px * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_dyn_stats, sizeof(int32_t) * DYNAMIC_STATS * n);
    if (rc != TSLAM_OK) {
        dynamic_off(h);
        return rc;
    }
    h->dyn_prm = p;
    h->dyn_pair = pair;
    h->dyn_rect = rect != 0;
    h->dyn_frames = max_frames;
    h->dyn_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_dynamic(tslam_handle* h, const void* depth, int64_t stride_bytes, int n_frames, int64_t first_frame,
                       const double* world_T_cam, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_dynamic", h->dyn_on, NO_DYNAMIC); rc != TSLAM_OK) return rc;
    if (!depth || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (n_frames < 0 || n_frames > h->dyn_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    int f0;
    if (const int rc = batch_frames(h, world_T_cam, first_frame, n_frames, &f0); rc != TSLAM_OK) return rc;
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const tslam_tsdf_dynamic_params& p = h->dyn_prm;
    const PairCamera k = pair_camera(h, h->dyn_pair, h->dyn_rect);
    const TsdfArgs& t = h->tsdf;
    TsdfDynamicArgs a{};
    a.tsdf = t.tsdf;
    a.weight = t.weight;
    a.nx = t.nx;
    a.ny = t.ny;
    a.nz = t.nz;
    a.ox = t.ox;
    a.oy = t.oy;
    a.oz = t.oz;
    a.s = t.s;
    a.win = h->d_tsdf_win;
    a.depth = static_cast<const uint8_t*>(depth);
    a.stride = stride_bytes;
    a.n = n_frames;
    a.W = h->W;
    a.H = h->H;
    a.fx = k.fx;
    a.fy = k.fy;
    a.cx = k.cx;
    a.cy = k.cy;
    a.map = k.map;
    a.max_dist = t.max_dist;
    a.min_free_weight = p.min_free_weight;
    a.thr = p.free_fraction * t.trunc;   // once, here
    a.open_radius = p.open_radius;
    a.dilate_radius = p.dilate_radius;
    a.layer = h->fs_on ? h->d_fs_words : nullptr;   // the free-space layer as the stream finds it
    a.bits = h->d_dyn_bits;
    a.out_depth = h->d_dyn_depth;
    a.out_mask = h->d_dyn_mask;
    a.stats = h->d_dyn_stats;
    const double* wtc;   // staged on the stream, as tslam_tsdf_render stages its host poses
    if (const int rc = stage_poses(world_T_cam, n_frames, h->d_dyn_wTc, s, &wtc); rc != TSLAM_OK) return rc;
    launch_tsdf_dynamic(make_ctx(h), h->dyn_pair, f0, wtc, a, h->d_dyn_poses, s);
    // after the mask outputs: the layer sees the call's used frames, in frame order, in the raw depth
    freespace_update(h, depth, stride_bytes, n_frames, f0, wtc, s);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_tsdf_dynamic_buffers(tslam_handle* h, void** depth, void** mask, void** stats, int64_t* frame_bytes) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->dyn_on) return fail(TSLAM_ESTATE, NO_DYNAMIC);
    if (depth) *depth = h->d_dyn_depth;
    if (mask) *mask = h->d_dyn_mask;
    if (stats) *stats = h->d_dyn_stats;
    if (frame_bytes) {
        const int64_t px = (int64_t)h->W * h->H;
        frame_bytes[0] = 2 * px;
        frame_bytes[1] = px;
    }
    return TSLAM_OK;
}

int tslam_tsdf_dynamic_read(tslam_handle* h, int frame, uint16_t* depth, uint8_t* mask, int32_t* stats) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->dyn_on) return fail(TSLAM_ESTATE, NO_DYNAMIC);
    if (frame < 0 || frame >= h->dyn_frames) return fail(TSLAM_EINVAL, "frame out of range");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t px = (size_t)h->W * h->H;
    if (depth) HIPCHK(hipMemcpy(depth, h->d_dyn_depth + px * frame, 2 * px, hipMemcpyDeviceToHost));
    if (mask) HIPCHK(hipMemcpy(mask, h->d_dyn_mask + px * frame, px, hipMemcpyDeviceToHost));
    if (stats) HIPCHK(hipMemcpy(stats, h->d_dyn_stats + (size_t)DYNAMIC_STATS * frame, sizeof(int32_t) * DYNAMIC_STATS, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

}  // extern "C"
