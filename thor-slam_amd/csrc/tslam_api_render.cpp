// tslam_api_render.cpp — the volume seen from a pose on the host side: TSDF ray casting
// (tslam_tsdf_render*) and the dense frame-to-model alignment that drives it (tslam_tsdf_align*,
// tslam_tsdf_integrate_aligned).
#include <algorithm>
#include <cmath>
#include <vector>

#include "tslam_handle.h"

static const int RENDER_MAX_IMAGE = 16384;
static const char* const NO_RENDER = "no render state (tslam_tsdf_render_init)";
static const char* const NO_ALIGN = "no align state (tslam_tsdf_align_init)";

// rule 1's L of a pinhole camera into L [H][W], on the host: the device takes no square root on the marching path
static void ray_length_table(int W, int H, double fx, double fy, double cx, double cy, double* L) {
    for (int y = 0; y < H; ++y) {
        const double dc1 = ((double)y - cy) / fy;
        for (int x = 0; x < W; ++x) {
            const double dc0 = ((double)x - cx) / fx;
            L[(size_t)y * W + x] = std::sqrt((dc0 * dc0 + dc1 * dc1) + 1.0);
        }
    }
}

// the align state's buffers go back to the device (tslam_tsdf_align_init with NULL; a new volume)
void align_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_aln_L, (void**)&h->d_aln_poses, (void**)&h->d_aln_wTc_in, (void**)&h->d_aln_depth_m,
                     (void**)&h->d_aln_normal, (void**)&h->d_aln_state, (void**)&h->d_aln_part, (void**)&h->d_aln_wTc,
                     (void**)&h->d_aln_stats, (void**)&h->d_aln_resid, (void**)&h->d_aln_neq})
        dev_release(h, p);
    h->aln_on = false;
    h->aln_frames = h->aln_n = 0;
}

extern "C" {

// -- the volume seen from a pose (k_tsdf_render.hip; thor_slam_amd/dense_render.py) ----------------
int tslam_tsdf_render_init(tslam_handle* h, const tslam_tsdf_render_params* params, int max_views) {
    if (!h || !params) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = dense_open(h, "tslam_tsdf_render_init"); rc != TSLAM_OK) return rc;
    const tslam_tsdf_render_params p = *params;
    if (h->tsdf.nx < 2 || h->tsdf.ny < 2 || h->tsdf.nz < 2) return fail(TSLAM_EINVAL, "rendering needs volume dims >= 2");
    if (p.width < 1 || p.height < 1 || p.width > RENDER_MAX_IMAGE || p.height > RENDER_MAX_IMAGE)
        return fail(TSLAM_EINVAL, "width and height must be 1..16384");
    for (const double v : {p.fx, p.fy, p.cx, p.cy, p.min_weight, p.min_depth, p.max_depth, p.step_scale})
        if (!std::isfinite(v)) return fail(TSLAM_EINVAL, "camera and render parameters must be finite");
    if (!(p.fx > 0.0 && p.fy > 0.0)) return fail(TSLAM_EINVAL, "fx and fy must be > 0");
    if (!(p.min_weight >= 0.0)) return fail(TSLAM_EINVAL, "min_weight must be >= 0");
    if (!(p.min_depth >= 0.0 && p.max_depth > p.min_depth)) return fail(TSLAM_EINVAL, "need 0 <= min_depth < max_depth");
    if (!(p.step_scale > 0.0 && p.step_scale <= 1.0)) return fail(TSLAM_EINVAL, "step_scale must be in (0, 1]");
    if (p.outputs < 1 || p.outputs > 15 || p.reserved != 0) return fail(TSLAM_EINVAL, "outputs must be a bit mask 1..15 and reserved 0");
    if (max_views < 1 || max_views > TSDF_MAX_FRAMES) return fail(TSLAM_EINVAL, "max_views must be 1..256");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    h->rnd_on = false;
    const size_t px = (size_t)p.width * p.height;
    std::vector<double> L(px);
    ray_length_table(p.width, p.height, p.fx, p.fy, p.cx, p.cy, L.data());
    int rc = dev_grow(h, (void**)&h->d_rnd_L, sizeof(double) * px);
    if (rc == TSLAM_OK && !h->d_rnd_poses) rc = dev_alloc(h, (void**)&h->d_rnd_poses, sizeof(double) * TSDF_MAX_FRAMES * TSDF_POSE);
    if (rc == TSLAM_OK && !h->d_rnd_wTc) rc = dev_alloc(h, (void**)&h->d_rnd_wTc, sizeof(double) * TSDF_MAX_FRAMES * 16);
    // an output that is not asked for keeps no buffer
    const size_t n = px * max_views;
    auto out = [&](void** buf, int bit, size_t bytes) {
        if (rc != TSLAM_OK) return;
        if (p.outputs & bit) rc = dev_grow(h, buf, bytes);
        else dev_release(h, buf);
    };
    out((void**)&h->d_rnd_depth_m, TSLAM_RENDER_DEPTH_M, sizeof(float) * n);
    out((void**)&h->d_rnd_depth_mm, TSLAM_RENDER_DEPTH_MM, sizeof(uint16_t) * n);
    out((void**)&h->d_rnd_normal, TSLAM_RENDER_NORMAL, sizeof(float) * 3 * n);
    out((void**)&h->d_rnd_color, TSLAM_RENDER_COLOR, 3 * n);
    if (rc != TSLAM_OK) return rc;
    HIPCHK(hipMemcpy(h->d_rnd_L, L.data(), sizeof(double) * px, hipMemcpyHostToDevice));
    h->rnd_prm = p;
    h->rnd_views = max_views;
    h->rnd_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_render(tslam_handle* h, int pair, const double* world_T_cam, int n_views, int64_t first_frame, void* stream) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    if (const int rc = dense_open(h, "tslam_tsdf_render", h->rnd_on, NO_RENDER); rc != TSLAM_OK) return rc;
    if (h->tsdf.nx < 2 || h->tsdf.ny < 2 || h->tsdf.nz < 2) return fail(TSLAM_EINVAL, "rendering needs volume dims >= 2");
    if (n_views < 0 || n_views > h->rnd_views) return fail(TSLAM_EINVAL, "n_views must be 0..max_views");
    int f0;
    if (const int rc = batch_frames(h, world_T_cam, first_frame, n_views, &f0); rc != TSLAM_OK) return rc;
    if (n_views == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const tslam_tsdf_render_params& p = h->rnd_prm;
    TsdfRenderArgs a{};
    volume_view(h, a);
    a.col = h->tsdf_color ? h->tsdf.col : nullptr;
    a.col_w = h->tsdf_color ? h->tsdf.col_w : nullptr;
    a.W = p.width;
    a.H = p.height;
    a.fx = p.fx;
    a.fy = p.fy;
    a.cx = p.cx;
    a.cy = p.cy;
    a.min_weight = p.min_weight;
    a.min_depth = p.min_depth;
    a.max_depth = p.max_depth;
    a.step_scale = p.step_scale;
    a.L = h->d_rnd_L;
    a.depth_m = h->d_rnd_depth_m;
    a.depth_mm = h->d_rnd_depth_mm;
    a.normal = h->d_rnd_normal;
    a.color = h->d_rnd_color;
    // host poses staged on the stream: the next call's copy is ordered behind this call's pose kernel.
    // From pageable memory the runtime reads the source before it returns (and may wait for the
    // stream to get there); no explicit synchronise is added, and device poses never wait
    const double* wtc;
    if (const int rc = stage_poses(world_T_cam, n_views, h->d_rnd_wTc, s, &wtc); rc != TSLAM_OK) return rc;
    launch_tsdf_render(make_ctx(h), pair, f0, wtc, a, n_views, h->d_rnd_poses, s);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_tsdf_render_buffers(tslam_handle* h, void** depth_m, void** depth_mm, void** normal, void** color,
                              int64_t* view_bytes) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->rnd_on) return fail(TSLAM_ESTATE, NO_RENDER);
    if (depth_m) *depth_m = h->d_rnd_depth_m;
    if (depth_mm) *depth_mm = h->d_rnd_depth_mm;
    if (normal) *normal = h->d_rnd_normal;
    if (color) *color = h->d_rnd_color;
    if (view_bytes) {
        const int64_t px = (int64_t)h->rnd_prm.width * h->rnd_prm.height;
        view_bytes[0] = 4 * px;
        view_bytes[1] = 2 * px;
        view_bytes[2] = 12 * px;
        view_bytes[3] = 3 * px;
    }
    return TSLAM_OK;
}

int tslam_tsdf_render_read(tslam_handle* h, int view, float* depth_m, uint16_t* depth_mm, float* normal, uint8_t* color) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->rnd_on) return fail(TSLAM_ESTATE, NO_RENDER);
    if (view < 0 || view >= h->rnd_views) return fail(TSLAM_EINVAL, "view out of range");
    if ((depth_m && !h->d_rnd_depth_m) || (depth_mm && !h->d_rnd_depth_mm) || (normal && !h->d_rnd_normal) ||
        (color && !h->d_rnd_color))
        return fail(TSLAM_EINVAL, "an output that tslam_tsdf_render_init was not asked for");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t px = (size_t)h->rnd_prm.width * h->rnd_prm.height;
    if (depth_m) HIPCHK(hipMemcpy(depth_m, h->d_rnd_depth_m + px * view, 4 * px, hipMemcpyDeviceToHost));
    if (depth_mm) HIPCHK(hipMemcpy(depth_mm, h->d_rnd_depth_mm + px * view, 2 * px, hipMemcpyDeviceToHost));
    if (normal) HIPCHK(hipMemcpy(normal, h->d_rnd_normal + 3 * px * view, 12 * px, hipMemcpyDeviceToHost));
    if (color) HIPCHK(hipMemcpy(color, h->d_rnd_color + 3 * px * view, 3 * px, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

// -- dense frame-to-model alignment (k_tsdf_align.hip; thor_slam_amd/dense_align.py) ---------------
int tslam_tsdf_align_init(tslam_handle* h, int pair, int rect, const tslam_tsdf_align_params* params, int max_frames) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_align_init"); rc != TSLAM_OK) return rc;
    if (!params) {   // off: the buffers go back
        if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
        align_off(h);
        return TSLAM_OK;
    }
    if (pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad pair");
    const tslam_tsdf_align_params p = *params;
    if (h->tsdf.nx < 2 || h->tsdf.ny < 2 || h->tsdf.nz < 2) return fail(TSLAM_EINVAL, "alignment needs volume dims >= 2");
    if (p.iterations < 1 || p.iterations > 64) return fail(TSLAM_EINVAL, "iterations must be 1..64");
    if (p.min_inliers < 6) return fail(TSLAM_EINVAL, "min_inliers must be >= 6");
    if (max_frames < 1 || max_frames > TSDF_MAX_FRAMES) return fail(TSLAM_EINVAL, "max_frames must be 1..256");
    for (const double v : {p.max_distance, p.min_weight, p.max_depth, p.step_scale, p.max_translation, p.max_rotation,
                           p.eps_translation, p.eps_rotation, p.min_pivot})
        if (!std::isfinite(v)) return fail(TSLAM_EINVAL, "align parameters must be finite");
    if (!(p.max_distance > 0.0 && p.max_depth > 0.0 && p.max_translation > 0.0))
        return fail(TSLAM_EINVAL, "max_distance, max_depth and max_translation must be > 0");
    if (!(p.min_weight >= 0.0)) return fail(TSLAM_EINVAL, "min_weight must be >= 0");
    if (!(p.step_scale > 0.0 && p.step_scale <= 1.0)) return fail(TSLAM_EINVAL, "step_scale must be in (0, 1]");
    if (!(p.max_rotation > 0.0 && p.max_rotation <= 3.141592653589793)) return fail(TSLAM_EINVAL, "max_rotation must be in (0, pi]");
    if (!(p.eps_translation >= 0.0 && p.eps_rotation >= 0.0)) return fail(TSLAM_EINVAL, "eps_translation and eps_rotation must be >= 0");
    if (!(p.min_pivot > 0.0 && p.min_pivot < 1.0)) return fail(TSLAM_EINVAL, "min_pivot must be in (0, 1)");
    for (const int32_t r : p.reserved)
        if (r != 0) return fail(TSLAM_EINVAL, "reserved must be 0");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    h->aln_on = false;
    // the pair's rectified camera, as tslam_tsdf_render_init takes its own
    const int W = h->W, H = h->H;
    const PairCamera k = pair_camera(h, pair, true);
    const size_t px = (size_t)W * H;
    std::vector<double> L(px);
    ray_length_table(W, H, k.fx, k.fy, k.cx, k.cy, L.data());
    const int blocks = ((W + 15) / 16) * ((H + 15) / 16);
    int pblocks = 256;
    while (pblocks < blocks) pblocks *= 2;
    const size_t n = (size_t)max_frames;
    int rc = dev_grow(h, (void**)&h->d_aln_L, sizeof(double) * px);
    if (rc == TSLAM_OK && !h->d_aln_poses) rc = dev_alloc(h, (void**)&h->d_aln_poses, sizeof(double) * TSDF_MAX_FRAMES * TSDF_POSE);
    if (rc == TSLAM_OK && !h->d_aln_wTc_in) rc = dev_alloc(h, (void**)&h->d_aln_wTc_in, sizeof(double) * TSDF_MAX_FRAMES * 16);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_depth_m, sizeof(float) * px * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_normal, sizeof(float) * 3 * px * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_state, sizeof(double) * ALIGN_STATE * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_part, sizeof(double) * ALIGN_PART * pblocks * n);   // zeroed: the padding stays zero
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_wTc, sizeof(double) * 16 * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_stats, sizeof(int32_t) * ALIGN_STATS * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_resid, sizeof(double) * 2 * n);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&h->d_aln_neq, sizeof(double) * 28 * n);
    if (rc != TSLAM_OK) {
        align_off(h);
        return rc;
    }
    HIPCHK(hipMemcpy(h->d_aln_L, L.data(), sizeof(double) * px, hipMemcpyHostToDevice));
    h->aln_prm = p;
    h->aln_pair = pair;
    h->aln_rect = rect != 0;
    h->aln_frames = max_frames;
    h->aln_pblocks = pblocks;
    h->aln_n = 0;
    h->aln_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_align(tslam_handle* h, const void* depth, int64_t stride_bytes, int n_frames, int64_t first_frame,
                     const double* world_T_cam, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_align", h->aln_on, NO_ALIGN); rc != TSLAM_OK) return rc;
    if (!depth || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (n_frames < 0 || n_frames > h->aln_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    const int pair = h->aln_pair;
    int f0;
    if (const int rc = batch_frames(h, world_T_cam, first_frame, n_frames, &f0); rc != TSLAM_OK) return rc;
    h->aln_n = n_frames;
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const tslam_tsdf_align_params& p = h->aln_prm;
    const PairCamera k = pair_camera(h, pair, h->aln_rect);
    TsdfRenderArgs r{};   // the ray caster as it stands, into this state's images (depth_m and normals only, no colour)
    volume_view(h, r);
    r.W = h->W;
    r.H = h->H;
    r.fx = k.fx;
    r.fy = k.fy;
    r.cx = k.cx;
    r.cy = k.cy;
    r.min_weight = p.min_weight;
    r.min_depth = 0.0;
    r.max_depth = p.max_depth;
    r.step_scale = p.step_scale;
    r.L = h->d_aln_L;
    r.depth_m = h->d_aln_depth_m;
    r.normal = h->d_aln_normal;
    TsdfAlignArgs a{};
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
    a.max_dist = h->tsdf.max_dist;
    a.depth_m = h->d_aln_depth_m;
    a.normal = h->d_aln_normal;
    a.max_distance2 = p.max_distance * p.max_distance;
    a.eps_t2 = p.eps_translation * p.eps_translation;
    a.eps_r2 = p.eps_rotation * p.eps_rotation;
    a.max_t2 = p.max_translation * p.max_translation;
    a.rot_lim = 1.0 + 2.0 * std::cos(p.max_rotation);
    a.min_pivot = p.min_pivot;
    a.min_inliers = p.min_inliers;
    a.iterations = p.iterations;
    a.pblocks = h->aln_pblocks;
    a.state = h->d_aln_state;
    a.partial = h->d_aln_part;
    a.wTc = h->d_aln_wTc;
    a.stats = h->d_aln_stats;
    a.resid = h->d_aln_resid;
    a.neq = h->d_aln_neq;
    const double* wtc;   // staged on the stream, as tslam_tsdf_render stages its host poses
    if (const int rc = stage_poses(world_T_cam, n_frames, h->d_aln_wTc_in, s, &wtc); rc != TSLAM_OK) return rc;
    launch_tsdf_align(make_ctx(h), pair, f0, wtc, r, a, h->d_aln_poses, s);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_tsdf_align_read(tslam_handle* h, int max_frames, double* world_T_cam, int32_t* stats, double* residuals,
                          double* normal_eq) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->aln_on) return fail(TSLAM_ESTATE, NO_ALIGN);
    if (max_frames < 0) return fail(TSLAM_EINVAL, "max_frames must be >= 0");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t n = (size_t)std::min(max_frames, h->aln_n);
    if (n == 0) return TSLAM_OK;
    if (world_T_cam) HIPCHK(hipMemcpy(world_T_cam, h->d_aln_wTc, sizeof(double) * 16 * n, hipMemcpyDeviceToHost));
    if (stats) HIPCHK(hipMemcpy(stats, h->d_aln_stats, sizeof(int32_t) * ALIGN_STATS * n, hipMemcpyDeviceToHost));
    if (residuals) HIPCHK(hipMemcpy(residuals, h->d_aln_resid, sizeof(double) * 2 * n, hipMemcpyDeviceToHost));
    if (normal_eq) HIPCHK(hipMemcpy(normal_eq, h->d_aln_neq, sizeof(double) * 28 * n, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_tsdf_align_buffers(tslam_handle* h, void** world_T_cam, void** stats) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->aln_on) return fail(TSLAM_ESTATE, NO_ALIGN);
    if (world_T_cam) *world_T_cam = h->d_aln_wTc;
    if (stats) *stats = h->d_aln_stats;
    return TSLAM_OK;
}

int tslam_tsdf_integrate_aligned(tslam_handle* h, const void* color, const void* depth, int64_t stride_bytes, int n_frames,
                                 void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_integrate_aligned", h->aln_on, NO_ALIGN); rc != TSLAM_OK) return rc;
    if (color && !h->tsdf_color) return fail(TSLAM_ESTATE, "no colour layer (tslam_tsdf_color before tslam_tsdf_init)");
    if (!depth || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (n_frames < 0 || n_frames > h->aln_n) return fail(TSLAM_EINVAL, "n_frames must be 0 .. the frames of the last tslam_tsdf_align");
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    TsdfArgs a = integrate_args(h, pair_camera(h, h->aln_pair, h->aln_rect), color != nullptr);
    a.stride = stride_bytes;
    a.n = n_frames;   // at most TSDF_MAX_FRAMES: one chunk
    a.depth = static_cast<const uint8_t*>(depth);
    a.color = static_cast<const uint8_t*>(color);
    const TsdfFollowCall fc = follow_call(h);
    launch_align_poses(h->d_aln_wTc, h->d_aln_stats, n_frames, h->d_tsdf_poses, s);
    launch_tsdf_posed(a, h->d_tsdf_poses, s, h->tsdf_follow_on ? &fc : nullptr);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

}  // extern "C"
