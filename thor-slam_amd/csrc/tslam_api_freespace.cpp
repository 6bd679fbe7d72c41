// tslam_api_freespace.cpp — masked objects that come to rest enter the map, on the host side: the
// free-space layer (tslam_tsdf_freespace_*; k_tsdf_freespace.hip; thor_slam_amd/dense_freespace.py).
// tslam_tsdf_dynamic (tslam_api_dynamic.cpp) classifies against the layer and updates it afterwards.
#include <cmath>

#include "tslam_handle.h"

static const char* const NO_FREESPACE = "no free-space layer (tslam_tsdf_freespace_init)";

// the layer goes back to the device (tslam_tsdf_freespace_init with NULL; a new volume)
void freespace_off(tslam_handle* h) {
    dev_release(h, (void**)&h->d_fs_words);
    dev_release(h, (void**)&h->d_fs_poses);
    h->fs_on = false;
    h->fs_band = 0.0;
    h->fs_settle = 0;
}

int freespace_reset(tslam_handle* h) {
    if (!h->fs_on) return TSLAM_OK;
    HIPCHK(hipMemset(h->d_fs_words, 0, sizeof(uint32_t) * tsdf_voxels(h)));
    return TSLAM_OK;
}

void freespace_update(tslam_handle* h, const void* depth, int64_t stride_bytes, int n_frames, int f0, const double* host_wTc_dev,
                      hipStream_t s) {
    if (!h->fs_on) return;
    // the camera of the mask's frames, the volume and the window as every integrate call sees them
    TsdfArgs a = integrate_args(h, pair_camera(h, h->dyn_pair, h->dyn_rect), false);
    a.depth = static_cast<const uint8_t*>(depth);   // the call's raw input, not the filtered copy
    a.stride = stride_bytes;
    a.n = n_frames;
    launch_tsdf_freespace(make_ctx(h), h->dyn_pair, f0, host_wTc_dev, a, h->d_fs_words, h->fs_band, h->fs_settle, h->d_fs_poses, s);
}

extern "C" {

int tslam_tsdf_freespace_init(tslam_handle* h, const tslam_tsdf_freespace_params* params) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_freespace_init"); rc != TSLAM_OK) return rc;
    // the brick store's bricks are sized for the layers it found: the layer is neither added nor freed under it
    if (h->store_on && (params != nullptr) != h->fs_on)
        return fail(TSLAM_ESTATE, "the free-space layer cannot be added or freed while the brick store is on (tslam_tsdf_store_init(0) first)");
    if (!params) {   // off: the layer goes back (the move's scratch keeps its size)
        if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
        freespace_off(h);
        return TSLAM_OK;
    }
    const tslam_tsdf_freespace_params p = *params;
    if (!std::isfinite(p.occupied_band_vox) || !(p.occupied_band_vox > 0.0) || !(p.occupied_band_vox <= h->tsdf_trunc_vox))
        return fail(TSLAM_EINVAL, "occupied_band_vox must be finite and in (0, trunc_vox]");
    if (p.settle_frames < 1 || p.settle_frames > 65535) return fail(TSLAM_EINVAL, "settle_frames must be 1..65535");
    for (const int32_t r : p.reserved)
        if (r != 0) return fail(TSLAM_EINVAL, "reserved must be 0");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    h->fs_on = false;
    int rc = dev_grow(h, (void**)&h->d_fs_words, sizeof(uint32_t) * tsdf_voxels(h));   // a new layer: all zero
    if (rc == TSLAM_OK && !h->d_fs_poses) rc = dev_alloc(h, (void**)&h->d_fs_poses, sizeof(double) * TSDF_MAX_FRAMES * TSDF_POSE);
    if (rc == TSLAM_OK && h->d_tsdf_win) rc = window_alloc(h);   // the move's scratch gains the layer's slot
    if (rc != TSLAM_OK) {
        freespace_off(h);
        return rc;
    }
    h->fs_band = p.occupied_band_vox * h->tsdf.s;   // once, here
    h->fs_settle = p.settle_frames;
    h->fs_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_freespace_read(tslam_handle* h, uint32_t* words) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_freespace_read", h->fs_on, NO_FREESPACE); rc != TSLAM_OK) return rc;
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    if (words) HIPCHK(hipMemcpy(words, h->d_fs_words, sizeof(uint32_t) * tsdf_voxels(h), hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_tsdf_freespace_write(tslam_handle* h, const uint32_t* words) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_freespace_write", h->fs_on, NO_FREESPACE); rc != TSLAM_OK) return rc;
    if (!words) return fail(TSLAM_EINVAL, "null words");
    const size_t nv = tsdf_voxels(h);
    for (size_t v = 0; v < nv; ++v)
        if (words[v] & ~(TSLAM_FREESPACE_RUN_MASK | TSLAM_FREESPACE_SETTLED)) return fail(TSLAM_EINVAL, "bits above 16 must be 0");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    HIPCHK(hipMemcpy(h->d_fs_words, words, sizeof(uint32_t) * nv, hipMemcpyHostToDevice));
    return TSLAM_OK;
}

}  // extern "C"
