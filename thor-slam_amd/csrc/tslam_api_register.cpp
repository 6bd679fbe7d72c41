// tslam_api_register.cpp — depth registration on the host side (tslam_depth_register*): the depth of
// a pair's rectified left camera forward-warped into a colour camera (k_depth_register.hip;
// thor_slam_amd/depth_register.py).
#include <cmath>

#include "tslam_handle.h"

static const int REGISTER_MAX_IMAGE = 16384;
static const char* const NO_REGISTER = "no depth registration state for this pair (tslam_depth_register_init)";

void register_destroy(tslam_handle* h) {
    for (hipEvent_t& e : h->dr_ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
}

// the argument check of every entry point but the init: the handle and the pair, then the pair's state
static int register_open(const tslam_handle* h, int pair) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    if (!h->dr[pair].on) return fail(TSLAM_ESTATE, NO_REGISTER);
    return TSLAM_OK;
}

extern "C" {

int tslam_depth_register_init(tslam_handle* h, int pair, const tslam_depth_register_params* params, int max_frames) {
    if (!h || !params) return fail(TSLAM_EINVAL, "bad argument");
    if (pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad pair");
    if (h->prm.rgbd) return fail(TSLAM_ESTATE, "depth registration needs a stereo handle (this one is RGB-D)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_depth_register_init inside a batch");
    const tslam_depth_register_params p = *params;
    if (p.width < 16 || p.height < 16 || p.width > h->W || p.height > h->H)
        return fail(TSLAM_EINVAL, "width / height must be 16 .. the handle's size");
    if (p.color_width < 1 || p.color_height < 1 || p.color_width > REGISTER_MAX_IMAGE || p.color_height > REGISTER_MAX_IMAGE)
        return fail(TSLAM_EINVAL, "color_width and color_height must be 1..16384");
    for (const double v : {p.f_c, p.cxc, p.cyc})
        if (!std::isfinite(v)) return fail(TSLAM_EINVAL, "f_c, cxc, cyc and color_T_rect must be finite");
    for (const double v : p.color_T_rect)
        if (!std::isfinite(v)) return fail(TSLAM_EINVAL, "f_c, cxc, cyc and color_T_rect must be finite");
    if (!(p.f_c > 0.0)) return fail(TSLAM_EINVAL, "f_c must be > 0");
    if (p.max_depth_mm < 1 || p.max_depth_mm > 65535) return fail(TSLAM_EINVAL, "max_depth_mm must be 1..65535");
    if (p.tol_mm < 0 || p.tol_mm > 65535) return fail(TSLAM_EINVAL, "tol_mm must be 0..65535");
    if (p.max_splat < 1 || p.max_splat > 8 || p.reserved != 0) return fail(TSLAM_EINVAL, "max_splat must be 1..8 and reserved 0");
    if (max_frames < 1 || max_frames > 65535) return fail(TSLAM_EINVAL, "max_frames must be 1..65535");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    tslam_handle::DepthReg& d = h->dr[pair];
    d.on = false;   // the buffers are resized below: an allocation failure leaves the pair without a state
    const size_t cpx = (size_t)p.color_width * p.color_height, dpx = (size_t)p.width * p.height;
    int rc = dev_grow(h, (void**)&d.d_z, sizeof(uint32_t) * cpx * max_frames);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&d.d_reg, sizeof(uint16_t) * cpx * max_frames);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&d.d_bgr, 3 * dpx * max_frames);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&d.d_mask, dpx * max_frames);
    if (rc == TSLAM_OK) {
        if (p.map) rc = dev_grow(h, (void**)&d.d_map, sizeof(int32_t) * 2 * cpx);
        else dev_release(h, (void**)&d.d_map);
    }
    if (rc != TSLAM_OK) return rc;
    if (p.map) HIPCHK(hipMemcpy(d.d_map, p.map, sizeof(int32_t) * 2 * cpx, hipMemcpyHostToDevice));
    d.prm = p;
    d.prm.map = d.d_map;
    d.frames = max_frames;
    d.on = true;
    return TSLAM_OK;
}

int tslam_depth_register(tslam_handle* h, int pair, const void* depth, int64_t depth_stride, const void* color,
                         int64_t color_stride, int n_frames, int first_slot, void* stream) {
    if (const int rc = register_open(h, pair); rc != TSLAM_OK) return rc;
    const tslam_handle::DepthReg& d = h->dr[pair];
    const tslam_depth_register_params& p = d.prm;
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_depth_register inside a batch");
    if (!depth || !color) return fail(TSLAM_EINVAL, "null depth or colour images");
    if (n_frames < 0 || n_frames > d.frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    if (first_slot < 0 || first_slot + n_frames > d.frames) return fail(TSLAM_EINVAL, "first_slot + n_frames must be within max_frames");
    if ((depth_stride & 1) || (n_frames > 1 && depth_stride < 2LL * p.width * p.height))
        return fail(TSLAM_EINVAL, "depth_stride must be even and at least one image");
    if (n_frames > 1 && color_stride < 3LL * p.color_width * p.color_height) return fail(TSLAM_EINVAL, "color_stride below one image");
    BA_FLUSH(h);
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const PairCalib& k = h->calib[pair];
    const size_t cpx = (size_t)p.color_width * p.color_height, dpx = (size_t)p.width * p.height;
    DepthRegArgs a{};
    a.W = p.width;
    a.H = p.height;
    a.Wc = p.color_width;
    a.Hc = p.color_height;
    a.n = n_frames;
    a.fx = k.fx;
    a.fy = k.fy;
    a.cx = k.cx;
    a.cy = k.cy;
    a.fc = p.f_c;
    a.cxc = p.cxc;
    a.cyc = p.cyc;
    for (int i = 0; i < 12; ++i) a.T[i] = p.color_T_rect[i];
    a.max_depth_mm = p.max_depth_mm;
    a.tol_mm = p.tol_mm;
    a.max_splat = p.max_splat;
    a.map = d.d_map;
    a.depth = static_cast<const uint8_t*>(depth);
    a.depth_stride = depth_stride;
    a.color = static_cast<const uint8_t*>(color);
    a.color_stride = color_stride;
    a.zbuf = d.d_z;
    a.reg = d.d_reg + cpx * first_slot;
    a.bgr = d.d_bgr + 3 * dpx * first_slot;
    a.mask = d.d_mask + dpx * first_slot;
    if (h->dr_prof)
        for (hipEvent_t& e : h->dr_ev)
            if (!e) HIPCHK(hipEventCreate(&e));
    HIPCHK(launch_depth_register(a, s, h->dr_prof ? h->dr_ev : nullptr));
    h->dr_timed = h->dr_prof;
    return TSLAM_OK;
}

int tslam_depth_register_blank(tslam_handle* h, int pair, int n_frames, int first_slot, void* stream) {
    if (const int rc = register_open(h, pair); rc != TSLAM_OK) return rc;
    const tslam_handle::DepthReg& d = h->dr[pair];
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_depth_register_blank inside a batch");
    if (n_frames < 0 || n_frames > d.frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    if (first_slot < 0 || first_slot + n_frames > d.frames) return fail(TSLAM_EINVAL, "first_slot + n_frames must be within max_frames");
    BA_FLUSH(h);
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const size_t dpx = (size_t)d.prm.width * d.prm.height;
    HIPCHK(hipMemsetAsync(d.d_bgr + 3 * dpx * first_slot, 0, 3 * dpx * n_frames, s));
    HIPCHK(hipMemsetAsync(d.d_mask + dpx * first_slot, 0, dpx * n_frames, s));
    return TSLAM_OK;
}

int tslam_depth_register_buffers(tslam_handle* h, int pair, void** registered_depth, void** bgr, void** mask, int64_t* slot_bytes) {
    if (const int rc = register_open(h, pair); rc != TSLAM_OK) return rc;
    const tslam_handle::DepthReg& d = h->dr[pair];
    if (registered_depth) *registered_depth = d.d_reg;
    if (bgr) *bgr = d.d_bgr;
    if (mask) *mask = d.d_mask;
    if (slot_bytes) {
        const int64_t cpx = (int64_t)d.prm.color_width * d.prm.color_height, dpx = (int64_t)d.prm.width * d.prm.height;
        slot_bytes[0] = 2 * cpx;
        slot_bytes[1] = 3 * dpx;
        slot_bytes[2] = dpx;
    }
    return TSLAM_OK;
}

int tslam_depth_register_read(tslam_handle* h, int pair, int slot, uint16_t* registered_depth, uint8_t* bgr, uint8_t* mask) {
    if (const int rc = register_open(h, pair); rc != TSLAM_OK) return rc;
    const tslam_handle::DepthReg& d = h->dr[pair];
    if (slot < 0 || slot >= d.frames) return fail(TSLAM_EINVAL, "slot out of range");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t cpx = (size_t)d.prm.color_width * d.prm.color_height, dpx = (size_t)d.prm.width * d.prm.height;
    if (registered_depth) HIPCHK(hipMemcpy(registered_depth, d.d_reg + cpx * slot, 2 * cpx, hipMemcpyDeviceToHost));
    if (bgr) HIPCHK(hipMemcpy(bgr, d.d_bgr + 3 * dpx * slot, 3 * dpx, hipMemcpyDeviceToHost));
    if (mask) HIPCHK(hipMemcpy(mask, d.d_mask + dpx * slot, dpx, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_depth_register_profile(tslam_handle* h, int enable, double* pass_ms) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (pass_ms) {
        if (!h->dr_timed) return fail(TSLAM_ESTATE, "no timed tslam_depth_register call");
        HIPCHK(hipEventSynchronize(h->dr_ev[3]));
        for (int i = 0; i < 3; ++i) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, h->dr_ev[i], h->dr_ev[i + 1]));
            pass_ms[i] = (double)ms;
        }
    }
    h->dr_prof = enable != 0;
    return TSLAM_OK;
}

}  // extern "C"
