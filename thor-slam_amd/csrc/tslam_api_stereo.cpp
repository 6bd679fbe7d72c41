// tslam_api_stereo.cpp — dense stereo depth on the host side (tslam_stereo_depth*): the box matcher,
// semi-global aggregation, the median and speckle filters.
#include <algorithm>

#include "tslam_handle.h"

extern "C" {

// the two checks behind the argument check of an entry point: the buffers, then (with `name`) the batch
static int stereo_open(const tslam_handle* h, const char* name = nullptr) {
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (name && h->in_batch) return fail(TSLAM_ESTATE, std::string(name) + " inside a batch");
    return TSLAM_OK;
}

// the semi-global matcher's scratch (A and S) goes back to the device; the box matcher runs again
static void sgm_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_sd_vol, (void**)&h->d_sd_sum}) dev_release(h, p);
    h->sd_sgm_on = false;
    h->sd_sgm_chunk = 0;
}

// the speckle filter's label and count planes go back to the device; the matcher's output is final again
static void filter_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_sd_label, (void**)&h->d_sd_count}) dev_release(h, p);
    h->sd_flt_on = false;
}

int tslam_stereo_depth_init(tslam_handle* h, const tslam_stereo_depth_params* params, int max_frames) {
    if (!h || !params) return fail(TSLAM_EINVAL, "bad argument");
    if (h->prm.rgbd) return fail(TSLAM_ESTATE, "dense stereo depth needs a stereo handle (this one is RGB-D)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_stereo_depth_init inside a batch");
    tslam_stereo_depth_params p = *params;
    if (p.n_disp == 0) p.n_disp = std::min(256, std::max(4, (int)h->prm.max_disparity));
    if (p.n_disp < 4 || p.n_disp > 256) return fail(TSLAM_EINVAL, "n_disp must be 4..256 (0 = max_disparity)");
    if (p.uniqueness < 0 || p.uniqueness > 99) return fail(TSLAM_EINVAL, "uniqueness must be 0..99");
    if (p.lr_tol < 0 || p.reserved != 0) return fail(TSLAM_EINVAL, "lr_tol must be >= 0 and reserved 0");
    if (max_frames < 1 || max_frames > 65535) return fail(TSLAM_EINVAL, "max_frames must be 1..65535");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    sgm_off(h);   // opt-in per init: n_disp and max_frames size its scratch
    filter_off(h);
    const size_t px = (size_t)max_frames * h->W * h->H;
    int rc = dev_grow(h, (void**)&h->d_sd_depth, 2 * px);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_sd_disp, 2 * px);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_sd_win, 2 * px);
    if (rc != TSLAM_OK) {
        h->sd_on = false;
        return rc;
    }
    h->sd_prm = p;
    h->sd_frames = max_frames;
    h->sd_w = h->W;
    h->sd_h = h->H;
    h->sd_on = true;
    return TSLAM_OK;
}

// rules 9 and 10, then rule 8, on the n frames of W x H that lie in the slots slot0 ..
//
// The median's u16 plane lives in d_sd_win, the matcher's call-scoped winner maps (u8, left half
// then right half, 2 * max_frames planes in all).  The u16 plane of slot s covers the bytes of the
// u8 planes 2s and 2s + 1, so at a slot offset it lies over winner maps of OTHER slots, and for
// s >= max_frames / 2 it reaches into the right-winner half.  That is safe: winner maps are
// written and read inside one matcher call, this filter runs after that call's matcher on the same
// stream, so every winner map is dead by now; and slot s < max_frames ends at byte
// 2 (s + 1) W H <= 2 max_frames W H, the size of the allocation.  Nothing a caller reads back lives
// in d_sd_win; the planes that do (disp32, depth, and the label / count scratch) are indexed by slot.
static int stereo_filter_run(tslam_handle* h, int W, int H, int n, double fxb, hipStream_t s, int slot0 = 0) {
    const tslam_stereo_depth_filter_params& p = h->sd_flt_prm;
    const size_t so = (size_t)slot0 * W * H;
    const StereoFilterArgs f{W, H, n, fxb, p.median, p.speckle_size, p.speckle_range, h->d_sd_disp + so, h->d_sd_depth + so,
                             reinterpret_cast<uint16_t*>(h->d_sd_win) + so, h->d_sd_label ? h->d_sd_label + so : nullptr,
                             h->d_sd_count ? h->d_sd_count + so : nullptr};
    HIPCHK(launch_sd_filter(f, s));
    return TSLAM_OK;
}

// the n frames of `a` into slots slot0 .. slot0 + n - 1: every per-slot plane starts slot0 planes in
static int stereo_depth_run(tslam_handle* h, StereoDepthArgs a, void* stream, int slot0 = 0) {
    const size_t so = (size_t)slot0 * a.W * a.H;
    a.n_disp = h->sd_prm.n_disp;
    a.uniqueness = h->sd_prm.uniqueness;
    a.lr_tol = h->sd_prm.lr_tol;
    a.depth = h->d_sd_depth + so;
    a.disp32 = h->d_sd_disp + so;
    a.win_left = h->d_sd_win + so;
    a.win_right = h->d_sd_win + (size_t)h->sd_frames * h->W * h->H + so;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    if (h->sd_sgm_on) {
        // chunks of the call's frames, one after the other on the stream, share the scratch
        const StereoSgmArgs g{h->sd_sgm_prm.p1, h->sd_sgm_prm.p2, h->sd_sgm_prm.paths, h->d_sd_vol, h->d_sd_sum};
        const size_t px = (size_t)a.W * a.H;
        for (int f0 = 0; f0 < a.n; f0 += h->sd_sgm_chunk) {
            StereoDepthArgs c = a;
            c.n = std::min(h->sd_sgm_chunk, a.n - f0);
            if (a.ring) c.first = a.first + f0;
            else {
                c.left = a.left + (size_t)f0 * a.stride;
                c.right = a.right + (size_t)f0 * a.stride;
            }
            c.depth = a.depth + px * f0;
            c.disp32 = a.disp32 + px * f0;
            c.win_left = a.win_left + px * f0;
            c.win_right = a.win_right + px * f0;
            HIPCHK(launch_stereo_depth_sgm(c, g, s));
        }
    } else {
        HIPCHK(launch_stereo_depth(a, s));
    }
    if (h->sd_flt_on)
        if (const int rc = stereo_filter_run(h, a.W, a.H, a.n, a.fxb, s, slot0); rc != TSLAM_OK) return rc;
    h->sd_w = a.W;
    h->sd_h = a.H;
    return TSLAM_OK;
}

int tslam_stereo_depth_sgm(tslam_handle* h, const tslam_stereo_depth_sgm_params* params) {
    if (!h || !params) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = stereo_open(h, "tslam_stereo_depth_sgm"); rc != TSLAM_OK) return rc;
    const tslam_stereo_depth_sgm_params p = *params;
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0) return fail(TSLAM_EINVAL, "reserved must be 0");
    if (p.enable) {
        if (p.p1 < 0 || p.p1 > p.p2 || p.p2 > 2400) return fail(TSLAM_EINVAL, "penalties must satisfy 0 <= p1 <= p2 <= 2400");
        if (p.paths < 1 || p.paths > 15) return fail(TSLAM_EINVAL, "paths must be a bit mask 1..15");
        if (p.chunk_frames < 0) return fail(TSLAM_EINVAL, "chunk_frames must be >= 0");
    }
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    if (!p.enable) {
        sgm_off(h);
        return TSLAM_OK;
    }
    const size_t frame = (size_t)h->W * h->H * sd_sgm_pitch(h->sd_prm.n_disp) * 2;   // bytes of A (or S) of one frame
    int chunk = p.chunk_frames;
    if (chunk == 0) chunk = (int)std::max<size_t>(1, ((size_t)1 << 30) / (2 * frame));
    chunk = std::min(chunk, h->sd_frames);
    if (chunk != h->sd_sgm_chunk || !h->d_sd_vol || !h->d_sd_sum) {
        sgm_off(h);
        int rc = dev_grow(h, (void**)&h->d_sd_vol, frame * chunk);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_sd_sum, frame * chunk);
        if (rc != TSLAM_OK) {
            sgm_off(h);
            return rc;
        }
    }
    h->sd_sgm_prm = p;
    h->sd_sgm_chunk = chunk;
    h->sd_sgm_on = true;
    return TSLAM_OK;
}

int tslam_stereo_depth_filter(tslam_handle* h, const tslam_stereo_depth_filter_params* params) {
    if (!h || !params) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = stereo_open(h, "tslam_stereo_depth_filter"); rc != TSLAM_OK) return rc;
    const tslam_stereo_depth_filter_params p = *params;
    if (p.reserved[0] != 0 || p.reserved[1] != 0 || p.reserved[2] != 0 || p.reserved[3] != 0)
        return fail(TSLAM_EINVAL, "reserved must be 0");
    if (p.enable) {
        if (p.median != 0 && p.median != 3 && p.median != 5 && p.median != 7) return fail(TSLAM_EINVAL, "median must be 0, 3, 5 or 7");
        if (p.speckle_size < 0 || p.speckle_size > 65535) return fail(TSLAM_EINVAL, "speckle_size must be 0..65535");
        if (p.speckle_range < 0 || p.speckle_range > 8191) return fail(TSLAM_EINVAL, "speckle_range must be 0..8191");
        if (p.median == 0 && p.speckle_size == 0) return fail(TSLAM_EINVAL, "enable needs a median or a speckle size");
    }
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    if (!p.enable) {
        filter_off(h);
        return TSLAM_OK;
    }
    if (p.speckle_size == 0) {
        filter_off(h);   // the median needs no planes of its own
    } else if (!h->d_sd_label || !h->d_sd_count) {
        const bool was_on = h->sd_flt_on;
        const size_t bytes = sizeof(uint32_t) * h->sd_frames * h->W * h->H;
        int rc = dev_grow(h, (void**)&h->d_sd_label, bytes);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_sd_count, bytes);
        if (rc != TSLAM_OK) {
            filter_off(h);
            h->sd_flt_on = was_on;   // a median-only setting needs none of what failed
            return rc;
        }
    }
    h->sd_flt_prm = p;
    h->sd_flt_on = true;
    return TSLAM_OK;
}

int tslam_stereo_depth_filter_apply(tslam_handle* h, const uint16_t* disp32, int width, int height, double fxb, int n_frames,
                                    void* stream) {
    if (!h || !disp32) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = stereo_open(h, "tslam_stereo_depth_filter_apply"); rc != TSLAM_OK) return rc;
    if (!h->sd_flt_on) return fail(TSLAM_ESTATE, "the filters are off (tslam_stereo_depth_filter)");
    if (n_frames < 0 || n_frames > h->sd_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    if (width < 16 || height < 16 || width > h->W || height > h->H)
        return fail(TSLAM_EINVAL, "width / height must be 16 .. the handle's size");
    if (!(fxb > 0.0)) return fail(TSLAM_EINVAL, "fxb must be > 0");
    BA_FLUSH(h);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    HIPCHK(launch_sd_filter_load(disp32, h->d_sd_disp, (size_t)n_frames * width * height, s));
    if (const int rc = stereo_filter_run(h, width, height, n_frames, fxb, s); rc != TSLAM_OK) return rc;
    h->sd_w = width;
    h->sd_h = height;
    return TSLAM_OK;
}

int tslam_stereo_depth_slots(tslam_handle* h, int pair, int64_t first_frame, int n_frames, int first_slot, void* stream) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    if (const int rc = stereo_open(h, "tslam_stereo_depth"); rc != TSLAM_OK) return rc;
    if (n_frames < 0 || n_frames > h->sd_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    if (first_slot < 0 || first_slot + n_frames > h->sd_frames) return fail(TSLAM_EINVAL, "first_slot + n_frames must be within max_frames");
    if (first_frame < h->cur_g0 || first_frame - h->cur_g0 + n_frames > h->cur_n)
        return fail(TSLAM_EINVAL, "frames must belong to the last batch");
    BA_FLUSH(h);
    const uint8_t* pyr = static_cast<const uint8_t*>(h->buf[TSLAM_BUF_PYRAMID].ptr);
    StereoDepthArgs a{};
    a.stride = (int64_t)h->C * h->g.pyr_bytes;
    a.left = pyr + (size_t)(2 * pair) * h->g.pyr_bytes + h->g.pyr_off[0];
    a.right = a.left + h->g.pyr_bytes;
    a.ring = h->R;
    a.first = first_frame;
    a.W = h->W;
    a.H = h->H;
    a.n = n_frames;
    a.fxb = h->calib[pair].fxb;
    return stereo_depth_run(h, a, stream, first_slot);
}

int tslam_stereo_depth(tslam_handle* h, int pair, int64_t first_frame, int n_frames, void* stream) {
    return tslam_stereo_depth_slots(h, pair, first_frame, n_frames, 0, stream);
}

int tslam_stereo_depth_images(tslam_handle* h, const uint8_t* left, const uint8_t* right, int64_t frame_stride, int width,
                              int height, double fxb, int n_frames, void* stream) {
    if (!h || !left || !right) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = stereo_open(h, "tslam_stereo_depth_images"); rc != TSLAM_OK) return rc;
    if (n_frames < 0 || n_frames > h->sd_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    if (width < 16 || height < 16 || width > h->W || height > h->H)
        return fail(TSLAM_EINVAL, "width / height must be 16 .. the handle's size");
    if (n_frames > 1 && frame_stride < (int64_t)width * height) return fail(TSLAM_EINVAL, "frame_stride below one image");
    if (!(fxb > 0.0)) return fail(TSLAM_EINVAL, "fxb must be > 0");
    BA_FLUSH(h);
    StereoDepthArgs a{};
    a.left = left;
    a.right = right;
    a.stride = frame_stride;
    a.W = width;
    a.H = height;
    a.n = n_frames;
    a.fxb = fxb;
    return stereo_depth_run(h, a, stream);
}

int tslam_stereo_depth_buffers(tslam_handle* h, void** depth, void** disp32, int64_t* frame_bytes) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = stereo_open(h); rc != TSLAM_OK) return rc;
    if (depth) *depth = h->d_sd_depth;
    if (disp32) *disp32 = h->d_sd_disp;
    if (frame_bytes) *frame_bytes = 2LL * h->W * h->H;
    return TSLAM_OK;
}

int tslam_stereo_depth_read(tslam_handle* h, int slot, uint16_t* depth, uint16_t* disp32) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = stereo_open(h); rc != TSLAM_OK) return rc;
    if (slot < 0 || slot >= h->sd_frames) return fail(TSLAM_EINVAL, "slot out of range");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t px = (size_t)h->sd_w * h->sd_h;
    if (depth) HIPCHK(hipMemcpy(depth, h->d_sd_depth + px * slot, 2 * px, hipMemcpyDeviceToHost));
    if (disp32) HIPCHK(hipMemcpy(disp32, h->d_sd_disp + px * slot, 2 * px, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

}  // extern "C"
