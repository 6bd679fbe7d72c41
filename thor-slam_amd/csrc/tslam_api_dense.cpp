// tslam_api_dense.cpp — the dense map on the host side: TSDF integration, dense stereo depth, and
// the outputs of the volume (marching-cubes mesh, ESDF, ESDF slice).
#include <algorithm>
#include <cmath>
#include <vector>

#include "tslam_handle.h"

static size_t tsdf_voxels(const tslam_handle* h) { return (size_t)h->tsdf.nx * h->tsdf.ny * h->tsdf.nz; }

// the synchronous reads and writes below: every stream's work on the map is done
static int dense_quiesce(tslam_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

// -- the rolling window (thor_slam_amd/dense_follow.py) -----------------------------------------
static size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

// the record and the move's scratch, on first use and after a larger tslam_tsdf_init
static int window_alloc(tslam_handle* h) {
    const size_t nv = tsdf_voxels(h);
    const size_t floats = 2 * align4(nv) + (h->tsdf.col ? align4(nv) + align4(3 * nv) : 0);
    int rc = dev_grow(h, (void**)&h->d_tsdf_scratch, sizeof(float) * floats, &h->tsdf_scratch_cap);
    if (rc == TSLAM_OK && !h->d_tsdf_win) {
        rc = dev_alloc(h, (void**)&h->d_tsdf_win, sizeof(TsdfWindow));
        if (rc != TSLAM_OK) return rc;
        HIPCHK(hipMemset(h->d_tsdf_win, 0, sizeof(TsdfWindow)));
    }
    return rc;
}

static TsdfLayers window_layers(const tslam_handle* h) {
    const TsdfArgs& t = h->tsdf;
    const size_t nv = tsdf_voxels(h);
    TsdfLayers l{};
    l.nx = t.nx;
    l.ny = t.ny;
    l.nz = t.nz;
    float* s = h->d_tsdf_scratch;
    auto add = [&](float* vol, int comp) {
        l.vol[l.n] = vol;
        l.scratch[l.n] = s;
        l.comp[l.n++] = comp;
        s += align4(nv * comp);
    };
    add(t.tsdf, 1);
    add(t.weight, 1);
    if (t.col) {
        add(t.col_w, 1);
        add(t.col, 3);
    }
    return l;
}

// the window as the device has it once `s` has drained: one small copy and a stream synchronise
// when the record exists, nothing otherwise
static int window_read(tslam_handle* h, hipStream_t s, int32_t shift[3], double origin[3]) {
    const TsdfArgs& t = h->tsdf;
    shift[0] = shift[1] = shift[2] = 0;
    if (h->d_tsdf_win) {
        HIPCHK(hipMemcpyAsync(shift, h->d_tsdf_win->shift, sizeof(int32_t) * 3, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    const double o0[3] = {t.ox, t.oy, t.oz};
    for (int a = 0; a < 3; ++a) origin[a] = h->d_tsdf_win ? o0[a] + t.s * (double)shift[a] : o0[a];
    return TSLAM_OK;
}

// tslam_reset: the volume belongs to the session (the stereo depth slots do not: they stay)
int dense_reset(tslam_handle* h) {
    if (h->tsdf_on) {
        if (h->d_tsdf_win) HIPCHK(hipMemset(h->d_tsdf_win, 0, sizeof(TsdfWindow)));
        const size_t nv = tsdf_voxels(h);
        HIPCHK(hipMemset(h->tsdf.tsdf, 0, sizeof(float) * nv));
        HIPCHK(hipMemset(h->tsdf.weight, 0, sizeof(float) * nv));
        if (h->tsdf.col) {
            HIPCHK(hipMemset(h->tsdf.col, 0, sizeof(float) * 3 * nv));
            HIPCHK(hipMemset(h->tsdf.col_w, 0, sizeof(float) * nv));
        }
    }
    if (h->rnd_on) {   // the render state stays, its images do not
        const size_t n = (size_t)h->rnd_prm.width * h->rnd_prm.height * h->rnd_views;
        if (h->d_rnd_depth_m) HIPCHK(hipMemset(h->d_rnd_depth_m, 0, sizeof(float) * n));
        if (h->d_rnd_depth_mm) HIPCHK(hipMemset(h->d_rnd_depth_mm, 0, sizeof(uint16_t) * n));
        if (h->d_rnd_normal) HIPCHK(hipMemset(h->d_rnd_normal, 0, sizeof(float) * 3 * n));
        if (h->d_rnd_color) HIPCHK(hipMemset(h->d_rnd_color, 0, 3 * n));
    }
    return TSLAM_OK;
}

// the align state's buffers go back to the device (tslam_tsdf_align_init with NULL; a new volume)
static void align_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_aln_L, (void**)&h->d_aln_poses, (void**)&h->d_aln_wTc_in, (void**)&h->d_aln_depth_m,
                     (void**)&h->d_aln_normal, (void**)&h->d_aln_state, (void**)&h->d_aln_part, (void**)&h->d_aln_wTc,
                     (void**)&h->d_aln_stats, (void**)&h->d_aln_resid, (void**)&h->d_aln_neq}) {
        if (!*p) continue;
        (void)hipFree(*p);
        h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), *p), h->allocs.end());
        *p = nullptr;
    }
    h->aln_on = false;
    h->aln_frames = h->aln_n = 0;
}

extern "C" {

// -- RGB-D dense mapping: TSDF integration -------------------------------------------------------
int tslam_tsdf_init(tslam_handle* h, const double* origin, const int32_t* dims, double voxel_size, double trunc_vox,
                    double max_dist, double max_weight) {
    if (!h || !origin || !dims) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || (int64_t)dims[0] * dims[1] * dims[2] > ((int64_t)1 << 31))
        return fail(TSLAM_EINVAL, "dims must be >= 1 with at most 2^31 voxels");
    if (!(voxel_size > 0.0) || !(trunc_vox > 0.0) || !(max_dist > 0.0) || !(max_weight >= 1.0))
        return fail(TSLAM_EINVAL, "voxel_size, trunc_vox, max_dist must be > 0 and max_weight >= 1");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = (size_t)dims[0] * dims[1] * dims[2];
    TsdfArgs& a = h->tsdf;
    int rc = dev_grow(h, (void**)&a.tsdf, sizeof(float) * nv);
    if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&a.weight, sizeof(float) * nv);
    if (rc == TSLAM_OK && h->tsdf_color) {
        rc = dev_grow(h, (void**)&a.col, sizeof(float) * 3 * nv);
        if (rc == TSLAM_OK) rc = dev_grow(h, (void**)&a.col_w, sizeof(float) * nv);
    }
    if (rc == TSLAM_OK && !h->d_tsdf_poses) rc = dev_alloc(h, (void**)&h->d_tsdf_poses, sizeof(double) * TSDF_MAX_FRAMES * TSDF_POSE);
    if (rc == TSLAM_OK && !h->d_tsdf_wTc) rc = dev_alloc(h, (void**)&h->d_tsdf_wTc, sizeof(double) * TSDF_MAX_FRAMES * 16);
    if (rc != TSLAM_OK) return rc;
    if (h->d_tsdf_win) HIPCHK(hipMemset(h->d_tsdf_win, 0, sizeof(TsdfWindow)));   // a new volume: shift 0, not following
    h->tsdf_follow_on = false;
    align_off(h);   // the align state belongs to the volume it was made for
    a.nx = dims[0];
    a.ny = dims[1];
    a.nz = dims[2];
    a.ox = origin[0];
    a.oy = origin[1];
    a.oz = origin[2];
    a.s = voxel_size;
    a.trunc = trunc_vox * voxel_size;
    a.max_dist = max_dist;
    a.max_weight = max_weight;
    h->tsdf_on = true;
    h->esdf_valid = false;   // outputs of the previous volume are gone
    h->mesh_n = 0;
    return TSLAM_OK;
}

static int tsdf_integrate(tslam_handle* h, int pair, const void* color, const void* depth, int64_t stride_bytes,
                          int n_frames, int64_t first_frame, const double* world_T_cam, void* stream, bool rect = false) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (!depth || n_frames < 0 || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_integrate inside a batch");
    int f0 = 0;
    if (!world_T_cam) {   // device poses: frames of the last batch
        f0 = (int)(first_frame - h->cur_g0);
        if (first_frame < h->cur_g0 || f0 + n_frames > h->cur_n)
            return fail(TSLAM_EINVAL, "device poses: frames must belong to the last batch");
    }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    const BatchCtx c = make_ctx(h);
    const int cam = c.cpp * pair;
    TsdfArgs a = h->tsdf;
    a.W = h->W;
    a.H = h->H;
    a.fx = h->calib[pair].fx;
    a.fy = h->calib[pair].fy;
    a.cx = h->calib[pair].cx;
    a.cy = h->calib[pair].cy;
    // rect: the depth lives in the pair's rectified camera already (tslam_stereo_depth)
    a.map = (!rect && ((h->map_mask >> cam) & 1u)) ? h->d_maps + (size_t)cam * h->W * h->H * 2 : nullptr;
    a.stride = stride_bytes;
    // following: the call's decision and move between chunk 0's poses and its integration
    a.win = h->d_tsdf_win;   // null unless the window was ever followed or shifted
    const TsdfFollowCall fc{h->tsdf_follow, h->tsdf_follow_on ? window_layers(h) : TsdfLayers{}, h->d_tsdf_win};
    if (!color) a.col = a.col_w = nullptr;   // the colour layer keeps its state without colour input
    for (int b0 = 0; b0 < n_frames; b0 += TSDF_MAX_FRAMES) {
        a.n = std::min(TSDF_MAX_FRAMES, n_frames - b0);
        a.depth = static_cast<const uint8_t*>(depth) + (size_t)b0 * stride_bytes;
        a.color = color ? static_cast<const uint8_t*>(color) + (size_t)b0 * stride_bytes : nullptr;
        const double* wtc = nullptr;
        if (world_T_cam) {
            HIPCHK(hipMemcpyAsync(h->d_tsdf_wTc, world_T_cam + (size_t)16 * b0, sizeof(double) * 16 * a.n,
                                  hipMemcpyHostToDevice, s));
            wtc = h->d_tsdf_wTc;
        }
        launch_tsdf(c, pair, f0 + b0, wtc, a, h->d_tsdf_poses, s, h->tsdf_follow_on && b0 == 0 ? &fc : nullptr);
        HIPCHK(hipGetLastError());
        if (world_T_cam) HIPCHK(hipStreamSynchronize(s));   // the staged host poses are reused
    }
    return TSLAM_OK;
}

int tslam_tsdf_follow(tslam_handle* h, const tslam_tsdf_follow_params* p) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_follow inside a batch");
    if (!p) {   // off: the window stays where it is
        h->tsdf_follow_on = false;
        return TSLAM_OK;
    }
    if (p->step < 1 || p->margin < p->step || p->margin >= TSDF_SHIFT_LIMIT) return fail(TSLAM_EINVAL, "need 1 <= step <= margin < 2^30");
    for (int a = 0; a < 3; ++a)
        if (p->anchor[a] <= -TSDF_SHIFT_LIMIT || p->anchor[a] >= TSDF_SHIFT_LIMIT) return fail(TSLAM_EINVAL, "|anchor| must be below 2^30");
    HIPCHK(hipSetDevice(h->device));
    if (const int rc = window_alloc(h); rc != TSLAM_OK) return rc;
    h->tsdf_follow = TsdfFollow{{p->anchor[0], p->anchor[1], p->anchor[2]}, p->margin, p->step};
    h->tsdf_follow_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_shift(tslam_handle* h, const int32_t* delta, void* stream) {
    if (!h || !delta) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_shift inside a batch");
    for (int a = 0; a < 3; ++a)
        if (delta[a] <= -TSDF_SHIFT_LIMIT || delta[a] >= TSDF_SHIFT_LIMIT) return fail(TSLAM_EINVAL, "|delta| must be below 2^30");
    HIPCHK(hipSetDevice(h->device));
    if (const int rc = window_alloc(h); rc != TSLAM_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    launch_tsdf_shift(h->d_tsdf_win, delta[0], delta[1], delta[2], s);
    launch_tsdf_move(window_layers(h), h->d_tsdf_win, s);
    HIPCHK(hipGetLastError());
    h->esdf_valid = false;
    return TSLAM_OK;
}

int tslam_tsdf_window(tslam_handle* h, int32_t* shift, double* origin) {
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    int32_t sh[3];
    double o[3];
    if (const int rc = window_read(h, h->last_stream, sh, o); rc != TSLAM_OK) return rc;
    for (int a = 0; a < 3; ++a) {
        if (shift) shift[a] = sh[a];
        if (origin) origin[a] = o[a];
    }
    return TSLAM_OK;
}

int tslam_tsdf_integrate(tslam_handle* h, int pair, const void* depth, int64_t stride_bytes, int n_frames,
                         int64_t first_frame, const double* world_T_cam, void* stream) {
    return tsdf_integrate(h, pair, nullptr, depth, stride_bytes, n_frames, first_frame, world_T_cam, stream);
}

int tslam_tsdf_integrate_rgbd(tslam_handle* h, int pair, const void* color, const void* depth, int64_t stride_bytes,
                              int n_frames, int64_t first_frame, const double* world_T_cam, void* stream) {
    if (!color) return fail(TSLAM_EINVAL, "null colour images");
    if (h && !h->tsdf_color) return fail(TSLAM_ESTATE, "no colour layer (tslam_tsdf_color before tslam_tsdf_init)");
    return tsdf_integrate(h, pair, color, depth, stride_bytes, n_frames, first_frame, world_T_cam, stream);
}

int tslam_tsdf_color(tslam_handle* h, int enable) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (h->tsdf_on && (enable != 0) != h->tsdf_color) return fail(TSLAM_ESTATE, "tslam_tsdf_color before tslam_tsdf_init");
    h->tsdf_color = enable != 0;
    return TSLAM_OK;
}

int tslam_tsdf_integrate_rect(tslam_handle* h, int pair, const void* depth, int64_t stride_bytes, int n_frames,
                              int64_t first_frame, const double* world_T_cam, void* stream) {
    return tsdf_integrate(h, pair, nullptr, depth, stride_bytes, n_frames, first_frame, world_T_cam, stream, true);
}

// Several cameras of a rig in one launch per chunk, on the body pose (k_tsdf.hip, launch_tsdf_rig).
int tslam_tsdf_integrate_rig(tslam_handle* h, const tslam_tsdf_rig_camera* cams, int n_cams, int n_frames,
                             int64_t first_frame, const double* world_T_base, void* stream) {
    if (!h || !cams) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->rig) return fail(TSLAM_ESTATE, "no rig set (tslam_set_rig)");
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_integrate_rig inside a batch");
    if (n_cams < 1 || n_cams > TS_RIG_MAXP) return fail(TSLAM_EINVAL, "n_cams must be 1..8");
    if (n_frames < 0) return fail(TSLAM_EINVAL, "n_frames must be >= 0");
    const bool color = cams[0].color != nullptr;
    for (int ci = 0; ci < n_cams; ++ci) {
        const tslam_tsdf_rig_camera& cm = cams[ci];
        if (cm.pair < 0 || cm.pair >= h->P || (ci > 0 && cm.pair <= cams[ci - 1].pair))
            return fail(TSLAM_EINVAL, "pairs must be strictly ascending and in range");
        if (!cm.depth || (n_frames > 1 && cm.stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
        if ((cm.color != nullptr) != color) return fail(TSLAM_EINVAL, "colour for all cameras or for none");
    }
    if (color && !h->tsdf_color) return fail(TSLAM_EINVAL, "colour without the colour layer (tslam_tsdf_color)");
    int f0 = 0;
    if (!world_T_base) {   // device poses: frames of the last batch
        f0 = (int)(first_frame - h->cur_g0);
        if (first_frame < h->cur_g0 || f0 + n_frames > h->cur_n)
            return fail(TSLAM_EINVAL, "device poses: frames must belong to the last batch");
    }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    const BatchCtx c = make_ctx(h);
    TsdfRigArgs a{};
    static_cast<TsdfArgs&>(a) = h->tsdf;
    a.W = h->W;
    a.H = h->H;
    a.n_cams = n_cams;
    a.win = h->d_tsdf_win;
    const TsdfFollowCall fc{h->tsdf_follow, h->tsdf_follow_on ? window_layers(h) : TsdfLayers{}, h->d_tsdf_win};
    if (!color) a.col = a.col_w = nullptr;   // the colour layer keeps its state without colour input
    uint64_t pairs = 0;
    for (int ci = 0; ci < n_cams; ++ci) {
        const int pair = cams[ci].pair, cam = c.cpp * pair;
        pairs |= (uint64_t)pair << (8 * ci);
        TsdfRigCam& r = a.cams[ci];
        r.fx = h->calib[pair].fx;
        r.fy = h->calib[pair].fy;
        r.cx = h->calib[pair].cx;
        r.cy = h->calib[pair].cy;
        r.map = (!cams[ci].rect && ((h->map_mask >> cam) & 1u)) ? h->d_maps + (size_t)cam * h->W * h->H * 2 : nullptr;
        r.stride = cams[ci].stride_bytes;
    }
    // chunks of whole frames, so that every chunk's views fit the pose table and stay frame-major
    const int chunk = TSDF_MAX_FRAMES / n_cams;
    for (int b0 = 0; b0 < n_frames; b0 += chunk) {
        const int nf = std::min(chunk, n_frames - b0);
        a.n = nf * n_cams;
        for (int ci = 0; ci < n_cams; ++ci) {
            const size_t o = (size_t)b0 * cams[ci].stride_bytes;
            a.cams[ci].depth = static_cast<const uint8_t*>(cams[ci].depth) + o;
            a.cams[ci].color = color ? static_cast<const uint8_t*>(cams[ci].color) + o : nullptr;
        }
        const double* wtb = nullptr;
        if (world_T_base) {
            HIPCHK(hipMemcpyAsync(h->d_tsdf_wTc, world_T_base + (size_t)16 * b0, sizeof(double) * 16 * nf,
                                  hipMemcpyHostToDevice, s));
            wtb = h->d_tsdf_wTc;
        }
        launch_tsdf_rig(c, pairs, f0 + b0, wtb, a, h->d_tsdf_poses, s, h->tsdf_follow_on && b0 == 0 ? &fc : nullptr);
        HIPCHK(hipGetLastError());
        if (world_T_base) HIPCHK(hipStreamSynchronize(s));   // the staged host poses are reused
    }
    return TSLAM_OK;
}

// -- the volume seen from a pose (k_tsdf_render.hip; thor_slam_amd/dense_render.py) ----------------
static const int RENDER_MAX_IMAGE = 16384;

int tslam_tsdf_render_init(tslam_handle* h, const tslam_tsdf_render_params* params, int max_views) {
    if (!h || !params) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_render_init inside a batch");
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
    // rule 1's L, on the host: the device takes no square root on the marching path
    const size_t px = (size_t)p.width * p.height;
    std::vector<double> L(px);
    for (int y = 0; y < p.height; ++y) {
        const double dc1 = ((double)y - p.cy) / p.fy;
        for (int x = 0; x < p.width; ++x) {
            const double dc0 = ((double)x - p.cx) / p.fx;
            L[(size_t)y * p.width + x] = std::sqrt((dc0 * dc0 + dc1 * dc1) + 1.0);
        }
    }
    int rc = dev_grow(h, (void**)&h->d_rnd_L, sizeof(double) * px);
    if (rc == TSLAM_OK && !h->d_rnd_poses) rc = dev_alloc(h, (void**)&h->d_rnd_poses, sizeof(double) * TSDF_MAX_FRAMES * TSDF_POSE);
    if (rc == TSLAM_OK && !h->d_rnd_wTc) rc = dev_alloc(h, (void**)&h->d_rnd_wTc, sizeof(double) * TSDF_MAX_FRAMES * 16);
    // an output that is not asked for keeps no buffer
    const size_t n = px * max_views;
    auto out = [&](void** buf, int bit, size_t bytes) {
        if (rc != TSLAM_OK) return;
        if (p.outputs & bit) {
            rc = dev_grow(h, buf, bytes);
        } else if (*buf) {
            (void)hipFree(*buf);
            h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), *buf), h->allocs.end());
            *buf = nullptr;
        }
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
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (!h->rnd_on) return fail(TSLAM_ESTATE, "no render state (tslam_tsdf_render_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_render inside a batch");
    if (h->tsdf.nx < 2 || h->tsdf.ny < 2 || h->tsdf.nz < 2) return fail(TSLAM_EINVAL, "rendering needs volume dims >= 2");
    if (n_views < 0 || n_views > h->rnd_views) return fail(TSLAM_EINVAL, "n_views must be 0..max_views");
    int f0 = 0;
    if (!world_T_cam) {   // device poses: frames of the last batch
        f0 = (int)(first_frame - h->cur_g0);
        if (first_frame < h->cur_g0 || f0 + n_views > h->cur_n)
            return fail(TSLAM_EINVAL, "device poses: frames must belong to the last batch");
    }
    if (n_views == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    const TsdfArgs& t = h->tsdf;
    const tslam_tsdf_render_params& p = h->rnd_prm;
    TsdfRenderArgs a{};
    a.tsdf = t.tsdf;
    a.weight = t.weight;
    a.col = h->tsdf_color ? t.col : nullptr;
    a.col_w = h->tsdf_color ? t.col_w : nullptr;
    a.nx = t.nx;
    a.ny = t.ny;
    a.nz = t.nz;
    a.ox = t.ox;
    a.oy = t.oy;
    a.oz = t.oz;
    a.s = t.s;
    a.win = h->d_tsdf_win;
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
    const double* wtc = nullptr;
    if (world_T_cam) {   // staged on the stream: the next call's copy is ordered behind this call's pose kernel.
                         // From pageable memory the runtime reads the source before it returns (and may wait for
                         // the stream to get there); no explicit synchronise is added, and device poses never wait
        HIPCHK(hipMemcpyAsync(h->d_rnd_wTc, world_T_cam, sizeof(double) * 16 * n_views, hipMemcpyHostToDevice, s));
        wtc = h->d_rnd_wTc;
    }
    launch_tsdf_render(make_ctx(h), pair, f0, wtc, a, n_views, h->d_rnd_poses, s);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_tsdf_render_buffers(tslam_handle* h, void** depth_m, void** depth_mm, void** normal, void** color,
                              int64_t* view_bytes) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->rnd_on) return fail(TSLAM_ESTATE, "no render state (tslam_tsdf_render_init)");
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
    if (!h->rnd_on) return fail(TSLAM_ESTATE, "no render state (tslam_tsdf_render_init)");
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
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_align_init inside a batch");
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
    // the pair's rectified camera: rule 1's L on the host, as tslam_tsdf_render_init builds it
    const int W = h->W, H = h->H;
    const PairCalib& k = h->calib[pair];
    const size_t px = (size_t)W * H;
    std::vector<double> L(px);
    for (int y = 0; y < H; ++y) {
        const double dc1 = ((double)y - k.cy) / k.fy;
        for (int x = 0; x < W; ++x) {
            const double dc0 = ((double)x - k.cx) / k.fx;
            L[(size_t)y * W + x] = std::sqrt((dc0 * dc0 + dc1 * dc1) + 1.0);
        }
    }
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
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (!h->aln_on) return fail(TSLAM_ESTATE, "no align state (tslam_tsdf_align_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_align inside a batch");
    if (!depth || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (n_frames < 0 || n_frames > h->aln_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    const int pair = h->aln_pair;
    int f0 = 0;
    if (!world_T_cam) {   // device poses: frames of the last batch
        f0 = (int)(first_frame - h->cur_g0);
        if (first_frame < h->cur_g0 || f0 + n_frames > h->cur_n)
            return fail(TSLAM_EINVAL, "device poses: frames must belong to the last batch");
    }
    h->aln_n = n_frames;
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    const BatchCtx c = make_ctx(h);
    const TsdfArgs& t = h->tsdf;
    const tslam_tsdf_align_params& p = h->aln_prm;
    const PairCalib& k = h->calib[pair];
    TsdfRenderArgs r{};   // the ray caster as it stands, into this state's images (depth_m and normals only)
    r.tsdf = t.tsdf;
    r.weight = t.weight;
    r.nx = t.nx;
    r.ny = t.ny;
    r.nz = t.nz;
    r.ox = t.ox;
    r.oy = t.oy;
    r.oz = t.oz;
    r.s = t.s;
    r.win = h->d_tsdf_win;
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
    const int cam = c.cpp * pair;
    a.map = (!h->aln_rect && ((h->map_mask >> cam) & 1u)) ? h->d_maps + (size_t)cam * h->W * h->H * 2 : nullptr;
    a.max_dist = t.max_dist;
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
    const double* wtc = nullptr;
    if (world_T_cam) {   // staged on the stream, as tslam_tsdf_render stages its host poses
        HIPCHK(hipMemcpyAsync(h->d_aln_wTc_in, world_T_cam, sizeof(double) * 16 * n_frames, hipMemcpyHostToDevice, s));
        wtc = h->d_aln_wTc_in;
    }
    launch_tsdf_align(c, pair, f0, wtc, r, a, h->d_aln_poses, s);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_tsdf_align_read(tslam_handle* h, int max_frames, double* world_T_cam, int32_t* stats, double* residuals,
                          double* normal_eq) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->aln_on) return fail(TSLAM_ESTATE, "no align state (tslam_tsdf_align_init)");
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
    if (!h->aln_on) return fail(TSLAM_ESTATE, "no align state (tslam_tsdf_align_init)");
    if (world_T_cam) *world_T_cam = h->d_aln_wTc;
    if (stats) *stats = h->d_aln_stats;
    return TSLAM_OK;
}

int tslam_tsdf_integrate_aligned(tslam_handle* h, const void* color, const void* depth, int64_t stride_bytes, int n_frames,
                                 void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (!h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    if (!h->aln_on) return fail(TSLAM_ESTATE, "no align state (tslam_tsdf_align_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_integrate_aligned inside a batch");
    if (color && !h->tsdf_color) return fail(TSLAM_ESTATE, "no colour layer (tslam_tsdf_color before tslam_tsdf_init)");
    if (!depth || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (n_frames < 0 || n_frames > h->aln_n) return fail(TSLAM_EINVAL, "n_frames must be 0 .. the frames of the last tslam_tsdf_align");
    if (n_frames == 0) return TSLAM_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    const int pair = h->aln_pair, cam = make_ctx(h).cpp * pair;
    TsdfArgs a = h->tsdf;
    a.W = h->W;
    a.H = h->H;
    a.fx = h->calib[pair].fx;
    a.fy = h->calib[pair].fy;
    a.cx = h->calib[pair].cx;
    a.cy = h->calib[pair].cy;
    a.map = (!h->aln_rect && ((h->map_mask >> cam) & 1u)) ? h->d_maps + (size_t)cam * h->W * h->H * 2 : nullptr;
    a.stride = stride_bytes;
    a.win = h->d_tsdf_win;
    const TsdfFollowCall fc{h->tsdf_follow, h->tsdf_follow_on ? window_layers(h) : TsdfLayers{}, h->d_tsdf_win};
    if (!color) a.col = a.col_w = nullptr;   // the colour layer keeps its state without colour input
    a.n = n_frames;   // at most TSDF_MAX_FRAMES: one chunk
    a.depth = static_cast<const uint8_t*>(depth);
    a.color = static_cast<const uint8_t*>(color);
    launch_align_poses(h->d_aln_wTc, h->d_aln_stats, n_frames, h->d_tsdf_poses, s);
    launch_tsdf_posed(a, h->d_tsdf_poses, s, h->tsdf_follow_on ? &fc : nullptr);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

// -- dense stereo depth ------------------------------------------------------------------------------
// the semi-global matcher's scratch (A and S) goes back to the device; the box matcher runs again
static void sgm_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_sd_vol, (void**)&h->d_sd_sum}) {
        if (!*p) continue;
        (void)hipFree(*p);
        h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), *p), h->allocs.end());
        *p = nullptr;
    }
    h->sd_sgm_on = false;
    h->sd_sgm_chunk = 0;
}

// the speckle filter's label and count planes go back to the device; the matcher's output is final again
static void filter_off(tslam_handle* h) {
    for (void** p : {(void**)&h->d_sd_label, (void**)&h->d_sd_count}) {
        if (!*p) continue;
        (void)hipFree(*p);
        h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), *p), h->allocs.end());
        *p = nullptr;
    }
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
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
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
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_stereo_depth_sgm inside a batch");
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
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_stereo_depth_filter inside a batch");
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
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_stereo_depth_filter_apply inside a batch");
    if (!h->sd_flt_on) return fail(TSLAM_ESTATE, "the filters are off (tslam_stereo_depth_filter)");
    if (n_frames < 0 || n_frames > h->sd_frames) return fail(TSLAM_EINVAL, "n_frames must be 0..max_frames");
    if (width < 16 || height < 16 || width > h->W || height > h->H)
        return fail(TSLAM_EINVAL, "width / height must be 16 .. the handle's size");
    if (!(fxb > 0.0)) return fail(TSLAM_EINVAL, "fxb must be > 0");
    BA_FLUSH(h);
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
    HIPCHK(launch_sd_filter_load(disp32, h->d_sd_disp, (size_t)n_frames * width * height, s));
    if (const int rc = stereo_filter_run(h, width, height, n_frames, fxb, s); rc != TSLAM_OK) return rc;
    h->sd_w = width;
    h->sd_h = height;
    return TSLAM_OK;
}

int tslam_stereo_depth_slots(tslam_handle* h, int pair, int64_t first_frame, int n_frames, int first_slot, void* stream) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_stereo_depth inside a batch");
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
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_stereo_depth_images inside a batch");
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
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (depth) *depth = h->d_sd_depth;
    if (disp32) *disp32 = h->d_sd_disp;
    if (frame_bytes) *frame_bytes = 2LL * h->W * h->H;
    return TSLAM_OK;
}

int tslam_stereo_depth_read(tslam_handle* h, int slot, uint16_t* depth, uint16_t* disp32) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->sd_on) return fail(TSLAM_ESTATE, "no stereo depth buffers (tslam_stereo_depth_init)");
    if (slot < 0 || slot >= h->sd_frames) return fail(TSLAM_EINVAL, "slot out of range");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t px = (size_t)h->sd_w * h->sd_h;
    if (depth) HIPCHK(hipMemcpy(depth, h->d_sd_depth + px * slot, 2 * px, hipMemcpyDeviceToHost));
    if (disp32) HIPCHK(hipMemcpy(disp32, h->d_sd_disp + px * slot, 2 * px, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_tsdf_read(tslam_handle* h, float* tsdf, float* weight) {
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    BA_FLUSH(h);
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = tsdf_voxels(h);
    if (tsdf) HIPCHK(hipMemcpy(tsdf, h->tsdf.tsdf, sizeof(float) * nv, hipMemcpyDeviceToHost));
    if (weight) HIPCHK(hipMemcpy(weight, h->tsdf.weight, sizeof(float) * nv, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_tsdf_read_color(tslam_handle* h, float* rgb, float* weight) {
    if (!h || !h->tsdf_on || !h->tsdf_color) return fail(TSLAM_ESTATE, "no colour layer");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = tsdf_voxels(h);
    if (rgb) HIPCHK(hipMemcpy(rgb, h->tsdf.col, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost));
    if (weight) HIPCHK(hipMemcpy(weight, h->tsdf.col_w, sizeof(float) * nv, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_tsdf_write_color(tslam_handle* h, const float* rgb, const float* weight) {
    if (!h || !h->tsdf_on || !h->tsdf_color) return fail(TSLAM_ESTATE, "no colour layer");
    if (!rgb || !weight) return fail(TSLAM_EINVAL, "null colour volume");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = tsdf_voxels(h);
    HIPCHK(hipMemcpy(h->tsdf.col, rgb, sizeof(float) * 3 * nv, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tsdf.col_w, weight, sizeof(float) * nv, hipMemcpyHostToDevice));
    return TSLAM_OK;
}

int tslam_tsdf_write(tslam_handle* h, const float* tsdf, const float* weight) {
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    BA_FLUSH(h);
    if (!tsdf || !weight) return fail(TSLAM_EINVAL, "null volume");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = tsdf_voxels(h);
    HIPCHK(hipMemcpy(h->tsdf.tsdf, tsdf, sizeof(float) * nv, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tsdf.weight, weight, sizeof(float) * nv, hipMemcpyHostToDevice));
    h->esdf_valid = false;
    return TSLAM_OK;
}

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
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
    BA_FLUSH(h);
    if (!(min_weight >= 0.0)) return fail(TSLAM_EINVAL, "min_weight must be >= 0");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
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
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
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
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
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
    hipStream_t s = stream ? (hipStream_t)stream : h->last_stream;
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
    if (!h || !h->tsdf_on) return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)");
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
