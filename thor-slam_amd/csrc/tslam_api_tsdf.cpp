// tslam_api_tsdf.cpp — the dense map's volume on the host side: the TSDF volume and its colour layer,
// the rolling window, every integrate entry point, and what the other dense files (render, stereo,
// outputs) share to work on the volume.
#include <algorithm>

#include "tslam_handle.h"

size_t tsdf_voxels(const tslam_handle* h) { return (size_t)h->tsdf.nx * h->tsdf.ny * h->tsdf.nz; }

// the synchronous reads and writes: every stream's work on the map is done
int dense_quiesce(tslam_handle* h) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

int no_volume() { return fail(TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)"); }

int dense_open(tslam_handle* h, const char* name, bool ready, const char* need) {
    BA_FLUSH(h);
    if (!h->tsdf_on) return no_volume();
    if (!ready) return fail(TSLAM_ESTATE, need);
    if (h->in_batch) return fail(TSLAM_ESTATE, std::string(name) + " inside a batch");
    return TSLAM_OK;
}

int batch_frames(const tslam_handle* h, const double* host_poses, int64_t first_frame, int n, int* f0) {
    *f0 = 0;
    if (host_poses) return TSLAM_OK;
    *f0 = (int)(first_frame - h->cur_g0);
    if (first_frame < h->cur_g0 || *f0 + n > h->cur_n)
        return fail(TSLAM_EINVAL, "device poses: frames must belong to the last batch");
    return TSLAM_OK;
}

PairCamera pair_camera(tslam_handle* h, int pair, bool rect) {
    const PairCalib& k = h->calib[pair];
    const int cam = make_ctx(h).cpp * pair;
    // rect: the depth lives in the pair's rectified camera already (tslam_stereo_depth)
    const bool table = !rect && ((h->map_mask >> cam) & 1u);
    return {k.fx, k.fy, k.cx, k.cy, table ? h->d_maps + (size_t)cam * h->W * h->H * 2 : nullptr};
}

void volume_view(const tslam_handle* h, TsdfRenderArgs& a) {
    const TsdfArgs& t = h->tsdf;
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
}

// -- the rolling window (thor_slam_amd/dense_follow.py) -----------------------------------------
static size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

// the record and the move's scratch, on first use, after a larger tslam_tsdf_init and when the
// free-space layer is added
int window_alloc(tslam_handle* h) {
    const size_t nv = tsdf_voxels(h);
    const size_t floats = 2 * align4(nv) + (h->tsdf.col ? align4(nv) + align4(3 * nv) : 0) + (h->d_fs_words ? align4(nv) : 0);
    int rc = dev_grow(h, (void**)&h->d_tsdf_scratch, sizeof(float) * floats, &h->tsdf_scratch_cap);
    if (rc == TSLAM_OK && !h->d_tsdf_win) {
        rc = dev_alloc(h, (void**)&h->d_tsdf_win, sizeof(TsdfWindow));
        if (rc != TSLAM_OK) return rc;
        HIPCHK(hipMemset(h->d_tsdf_win, 0, sizeof(TsdfWindow)));
    }
    return rc;
}

TsdfLayers window_layers(const tslam_handle* h) {
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
    // the free-space words: one more 1-component 4-byte layer, moved as bits (entering voxels: 0)
    if (h->d_fs_words) add(reinterpret_cast<float*>(h->d_fs_words), 1);
    return l;
}

// the window as the device has it once `s` has drained: one small copy and a stream synchronise
// when the record exists, nothing otherwise
int window_read(tslam_handle* h, hipStream_t s, int32_t shift[3], double origin[3]) {
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

TsdfArgs integrate_args(const tslam_handle* h, const PairCamera& k, bool color_given) {
    TsdfArgs a = h->tsdf;
    a.W = h->W;
    a.H = h->H;
    a.fx = k.fx;
    a.fy = k.fy;
    a.cx = k.cx;
    a.cy = k.cy;
    a.map = k.map;
    a.win = h->d_tsdf_win;   // null unless the window was ever followed or shifted
    if (!color_given) a.col = a.col_w = nullptr;   // the colour layer keeps its state without colour input
    return a;
}

// following: the call's decision and move between chunk 0's poses and its integration
TsdfFollowCall follow_call(const tslam_handle* h) {
    return {h->tsdf_follow, h->tsdf_follow_on ? window_layers(h) : TsdfLayers{}, h->d_tsdf_win, store_of(h)};
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
        if (const int rc = archive_reset(h); rc != TSLAM_OK) return rc;
        if (const int rc = freespace_reset(h); rc != TSLAM_OK) return rc;
        if (const int rc = store_clear(h); rc != TSLAM_OK) return rc;   // the brick store is empty too
    }
    if (h->rnd_on) {   // the render state stays, its images do not
        const size_t n = (size_t)h->rnd_prm.width * h->rnd_prm.height * h->rnd_views;
        if (h->d_rnd_depth_m) HIPCHK(hipMemset(h->d_rnd_depth_m, 0, sizeof(float) * n));
        if (h->d_rnd_depth_mm) HIPCHK(hipMemset(h->d_rnd_depth_mm, 0, sizeof(uint16_t) * n));
        if (h->d_rnd_normal) HIPCHK(hipMemset(h->d_rnd_normal, 0, sizeof(float) * 3 * n));
        if (h->d_rnd_color) HIPCHK(hipMemset(h->d_rnd_color, 0, 3 * n));
    }
    return dynamic_reset(h);   // and so does the free-space mask's
}

int stage_poses(const double* host, int n, double* staging, hipStream_t s, const double** staged) {
    *staged = nullptr;
    if (!host) return TSLAM_OK;
    HIPCHK(hipMemcpyAsync(staging, host, sizeof(double) * 16 * n, hipMemcpyHostToDevice, s));
    *staged = staging;
    return TSLAM_OK;
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
    dynamic_off(h);   // and the free-space mask's state
    freespace_off(h);   // and the free-space layer
    archive_off(h);   // and so does the depth archive
    a.nx = dims[0];
    a.ny = dims[1];
    a.nz = dims[2];
    a.ox = origin[0];
    a.oy = origin[1];
    a.oz = origin[2];
    a.s = voxel_size;
    a.trunc = trunc_vox * voxel_size;
    h->tsdf_trunc_vox = trunc_vox;
    a.max_dist = max_dist;
    a.max_weight = max_weight;
    h->tsdf_on = true;
    h->esdf_valid = false;   // outputs of the previous volume are gone
    h->mesh_n = 0;
    return store_clear(h);   // a new volume: an empty brick store (it stays on)
}

// its own order of refusals: the depth and the stride before the batch.  color_stride 0: the colour
// lies in the depth's records (stride_bytes apart); mask: TsdfArgs::mask, or null
static int tsdf_integrate(tslam_handle* h, int pair, const void* color, const void* depth, int64_t stride_bytes,
                          int n_frames, int64_t first_frame, const double* world_T_cam, void* stream, bool rect = false,
                          int64_t color_stride = 0, const void* mask = nullptr, int64_t mask_stride = 0) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    BA_FLUSH(h);
    if (!h->tsdf_on) return no_volume();
    if (!depth || n_frames < 0 || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_integrate inside a batch");
    int f0;
    if (const int rc = batch_frames(h, world_T_cam, first_frame, n_frames, &f0); rc != TSLAM_OK) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const BatchCtx c = make_ctx(h);
    TsdfArgs a = integrate_args(h, pair_camera(h, pair, rect), color != nullptr);
    a.stride = stride_bytes;
    a.color_stride = color_stride ? color_stride : stride_bytes;
    a.mask_stride = mask_stride;
    const TsdfFollowCall fc = follow_call(h);
    for (int b0 = 0; b0 < n_frames; b0 += TSDF_MAX_FRAMES) {
        a.n = std::min(TSDF_MAX_FRAMES, n_frames - b0);
        a.depth = static_cast<const uint8_t*>(depth) + (size_t)b0 * stride_bytes;
        a.color = color ? static_cast<const uint8_t*>(color) + (size_t)b0 * a.color_stride : nullptr;
        a.mask = mask ? static_cast<const uint8_t*>(mask) + (size_t)b0 * mask_stride : nullptr;
        const double* wtc;
        if (const int rc = stage_poses(world_T_cam ? world_T_cam + (size_t)16 * b0 : nullptr, a.n, h->d_tsdf_wTc, s, &wtc); rc != TSLAM_OK) return rc;
        launch_tsdf(c, pair, f0 + b0, wtc, a, h->d_tsdf_poses, s, h->tsdf_follow_on && b0 == 0 ? &fc : nullptr);
        HIPCHK(hipGetLastError());
        if (world_T_cam) HIPCHK(hipStreamSynchronize(s));   // the staged host poses are reused
    }
    return TSLAM_OK;
}

int tslam_tsdf_follow(tslam_handle* h, const tslam_tsdf_follow_params* p) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (const int rc = dense_open(h, "tslam_tsdf_follow"); rc != TSLAM_OK) return rc;
    if (!p) {   // off: the window stays where it is
        h->tsdf_follow_on = false;
        return TSLAM_OK;
    }
    if (h->arc_on) return fail(TSLAM_ESTATE, "the depth archive does not follow the window (tslam_tsdf_archive_init)");
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
    if (const int rc = dense_open(h, "tslam_tsdf_shift"); rc != TSLAM_OK) return rc;
    for (int a = 0; a < 3; ++a)
        if (delta[a] <= -TSDF_SHIFT_LIMIT || delta[a] >= TSDF_SHIFT_LIMIT) return fail(TSLAM_EINVAL, "|delta| must be below 2^30");
    HIPCHK(hipSetDevice(h->device));
    if (const int rc = window_alloc(h); rc != TSLAM_OK) return rc;
    hipStream_t s = call_stream(h, stream);
    launch_tsdf_shift(h->d_tsdf_win, delta[0], delta[1], delta[2], s);
    launch_tsdf_move(window_layers(h), h->d_tsdf_win, s, store_of(h));
    HIPCHK(hipGetLastError());
    h->esdf_valid = false;
    return TSLAM_OK;
}

int tslam_tsdf_window(tslam_handle* h, int32_t* shift, double* origin) {
    if (!h || !h->tsdf_on) return no_volume();
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

int tslam_tsdf_integrate_rect_color(tslam_handle* h, int pair, const void* color, int64_t color_stride, const void* mask,
                                    int64_t mask_stride, const void* depth, int64_t stride_bytes, int n_frames,
                                    int64_t first_frame, const double* world_T_cam, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "bad handle or pair");
    if (!color) return fail(TSLAM_EINVAL, "null colour images");
    if (!h->tsdf_color) return fail(TSLAM_ESTATE, "no colour layer (tslam_tsdf_color before tslam_tsdf_init)");
    // strides of their own, so at least one image each, whatever n_frames is
    if (color_stride < 3LL * h->W * h->H || (mask && mask_stride < (int64_t)h->W * h->H))
        return fail(TSLAM_EINVAL, "bad colour / mask stride");
    return tsdf_integrate(h, pair, color, depth, stride_bytes, n_frames, first_frame, world_T_cam, stream, true,
                          color_stride, mask, mask_stride);
}

// Several cameras of a rig in one launch per chunk, on the body pose (k_tsdf.hip, launch_tsdf_rig).
// Its own order of refusals: the rig before the volume.  colors null: the colour of camera ci is
// cams[ci].color, in its depth's records; else colors[ci], with strides of its own and a mask.
static int tsdf_integrate_rig(tslam_handle* h, const tslam_tsdf_rig_camera* cams, const tslam_tsdf_rig_color* colors,
                              int n_cams, int n_frames, int64_t first_frame, const double* world_T_base, void* stream) {
    if (!h || !cams) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->rig) return fail(TSLAM_ESTATE, "no rig set (tslam_set_rig)");
    if (!h->tsdf_on) return no_volume();
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_integrate_rig inside a batch");
    if (n_cams < 1 || n_cams > TS_RIG_MAXP) return fail(TSLAM_EINVAL, "n_cams must be 1..8");
    if (n_frames < 0) return fail(TSLAM_EINVAL, "n_frames must be >= 0");
    const bool color = colors ? colors[0].color != nullptr : cams[0].color != nullptr;
    for (int ci = 0; ci < n_cams; ++ci) {
        const tslam_tsdf_rig_camera& cm = cams[ci];
        if (colors) {
            const tslam_tsdf_rig_color& cc = colors[ci];
            if (cm.color) return fail(TSLAM_EINVAL, "colour comes from the colour descriptors: cams[].color must be NULL");
            if ((cc.color != nullptr) != color) return fail(TSLAM_EINVAL, "colour for all cameras or for none");
            if (cc.color && (cc.color_stride < 3LL * h->W * h->H || (cc.mask && cc.mask_stride < (int64_t)h->W * h->H)))
                return fail(TSLAM_EINVAL, "bad colour / mask stride");
        }
        if (cm.pair < 0 || cm.pair >= h->P || (ci > 0 && cm.pair <= cams[ci - 1].pair))
            return fail(TSLAM_EINVAL, "pairs must be strictly ascending and in range");
        if (!cm.depth || (n_frames > 1 && cm.stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
        if (!colors && (cm.color != nullptr) != color) return fail(TSLAM_EINVAL, "colour for all cameras or for none");
    }
    if (color && !h->tsdf_color) return fail(TSLAM_EINVAL, "colour without the colour layer (tslam_tsdf_color)");
    int f0;
    if (const int rc = batch_frames(h, world_T_base, first_frame, n_frames, &f0); rc != TSLAM_OK) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const BatchCtx c = make_ctx(h);
    TsdfRigArgs a{};
    static_cast<TsdfArgs&>(a) = integrate_args(h, PairCamera{}, color);   // the cameras go into their records
    a.n_cams = n_cams;
    const TsdfFollowCall fc = follow_call(h);
    uint64_t pairs = 0;
    for (int ci = 0; ci < n_cams; ++ci) {
        const PairCamera k = pair_camera(h, cams[ci].pair, cams[ci].rect != 0);
        pairs |= (uint64_t)cams[ci].pair << (8 * ci);
        TsdfRigCam& r = a.cams[ci];
        r.fx = k.fx;
        r.fy = k.fy;
        r.cx = k.cx;
        r.cy = k.cy;
        r.map = k.map;
        r.stride = cams[ci].stride_bytes;
        r.color_stride = colors ? colors[ci].color_stride : r.stride;
        r.mask_stride = colors ? colors[ci].mask_stride : 0;
    }
    // chunks of whole frames, so that every chunk's views fit the pose table and stay frame-major
    const int chunk = TSDF_MAX_FRAMES / n_cams;
    for (int b0 = 0; b0 < n_frames; b0 += chunk) {
        const int nf = std::min(chunk, n_frames - b0);
        a.n = nf * n_cams;
        for (int ci = 0; ci < n_cams; ++ci) {
            const size_t o = (size_t)b0 * cams[ci].stride_bytes;
            a.cams[ci].depth = static_cast<const uint8_t*>(cams[ci].depth) + o;
            const void* col = colors ? colors[ci].color : cams[ci].color;
            const void* msk = colors ? colors[ci].mask : nullptr;
            a.cams[ci].color = color ? static_cast<const uint8_t*>(col) + (size_t)b0 * a.cams[ci].color_stride : nullptr;
            a.cams[ci].mask = color && msk ? static_cast<const uint8_t*>(msk) + (size_t)b0 * a.cams[ci].mask_stride : nullptr;
        }
        const double* wtb;
        if (const int rc = stage_poses(world_T_base ? world_T_base + (size_t)16 * b0 : nullptr, nf, h->d_tsdf_wTc, s, &wtb); rc != TSLAM_OK) return rc;
        launch_tsdf_rig(c, pairs, f0 + b0, wtb, a, h->d_tsdf_poses, s, h->tsdf_follow_on && b0 == 0 ? &fc : nullptr);
        HIPCHK(hipGetLastError());
        if (world_T_base) HIPCHK(hipStreamSynchronize(s));   // the staged host poses are reused
    }
    return TSLAM_OK;
}

int tslam_tsdf_integrate_rig(tslam_handle* h, const tslam_tsdf_rig_camera* cams, int n_cams, int n_frames,
                             int64_t first_frame, const double* world_T_base, void* stream) {
    return tsdf_integrate_rig(h, cams, nullptr, n_cams, n_frames, first_frame, world_T_base, stream);
}

int tslam_tsdf_integrate_rig_color(tslam_handle* h, const tslam_tsdf_rig_camera* cams, const tslam_tsdf_rig_color* colors,
                                   int n_cams, int n_frames, int64_t first_frame, const double* world_T_base, void* stream) {
    if (!colors) return fail(TSLAM_EINVAL, "bad argument");
    return tsdf_integrate_rig(h, cams, colors, n_cams, n_frames, first_frame, world_T_base, stream);
}

// -- the volume read and written on the host ------------------------------------------------------
int tslam_tsdf_read(tslam_handle* h, float* tsdf, float* weight) {
    if (!h || !h->tsdf_on) return no_volume();
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
    if (!h || !h->tsdf_on) return no_volume();
    BA_FLUSH(h);
    if (!tsdf || !weight) return fail(TSLAM_EINVAL, "null volume");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    const size_t nv = tsdf_voxels(h);
    HIPCHK(hipMemcpy(h->tsdf.tsdf, tsdf, sizeof(float) * nv, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->tsdf.weight, weight, sizeof(float) * nv, hipMemcpyHostToDevice));
    h->esdf_valid = false;
    archive_off(h);   // the archived frames are not what this volume holds
    return TSLAM_OK;
}

}  // extern "C"
