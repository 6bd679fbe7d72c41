// tslam_api_archive.cpp — the dense map's depth archive on the host side: the ring of the depth
// frames the volume was built from, the integrate call that fills it, and the move that takes the
// frames whose poses changed out of the volume and puts them back (k_tsdf_move_frames.hip;
// thor_slam_amd/dense_loop.py).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "tslam_handle.h"

static int no_archive() { return fail(TSLAM_ESTATE, "no depth archive (tslam_tsdf_archive_init)"); }

static int64_t slot_stride(const tslam_handle* h) { return (2LL * h->W * h->H + 15) & ~15LL; }

// the ring is empty: no frame, nothing moved
static int ring_clear(tslam_handle* h) {
    HIPCHK(hipMemset(h->arc.rec, 0, sizeof(TsdfArchiveRec)));
    HIPCHK(hipMemset(h->arc.frame, 0xFF, sizeof(int64_t) * h->arc.cap));
    return TSLAM_OK;
}

int archive_reset(tslam_handle* h) { return h->arc_on ? ring_clear(h) : TSLAM_OK; }

void archive_off(tslam_handle* h) { h->arc_on = false; }

void archive_destroy(tslam_handle* h) {
    if (h->arc_ev) (void)hipEventDestroy(h->arc_ev);
    h->arc_ev = nullptr;
}

// a move's requests: n frame ids, then n poses, at 8-byte granules
static size_t req_bytes(int n) { return sizeof(int64_t) * (size_t)n + sizeof(double) * 16 * (size_t)n; }

extern "C" {

int tslam_tsdf_archive_init(tslam_handle* h, int pair, int rect, int capacity, int interval) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    if (const int rc = dense_open(h, "tslam_tsdf_archive_init"); rc != TSLAM_OK) return rc;
    if (h->tsdf_color) return fail(TSLAM_ESTATE, "the depth archive does not move the colour layer (tslam_tsdf_color)");
    if (h->tsdf_follow_on) return fail(TSLAM_ESTATE, "the depth archive does not follow the window (tslam_tsdf_follow)");
    if (h->store_on) return fail(TSLAM_ESTATE, "the depth archive does not run with the brick store (tslam_tsdf_store_init)");
    if (capacity < 1 || interval < 1) return fail(TSLAM_EINVAL, "capacity and interval must be >= 1");
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    h->arc_on = false;
    TsdfArchive& ar = h->arc;
    const size_t cap = (size_t)capacity;
    ar.slot_stride = slot_stride(h);
    int rc = dev_grow(h, (void**)&ar.depth, cap * (size_t)ar.slot_stride);
    auto grow = [&](void** p, size_t bytes) {
        if (rc == TSLAM_OK) rc = dev_grow(h, p, bytes);
    };
    grow((void**)&ar.pose, sizeof(double) * TSDF_POSE * cap);
    grow((void**)&ar.wTc, sizeof(double) * 16 * cap);
    grow((void**)&ar.frame, sizeof(int64_t) * cap);
    grow((void**)&ar.sel_slot, sizeof(int32_t) * cap);
    grow((void**)&ar.sel_old, sizeof(double) * TSDF_POSE * cap);
    grow((void**)&ar.sel_new, sizeof(double) * TSDF_POSE * cap);
    grow((void**)&ar.sel_wTc, sizeof(double) * 16 * cap);
    if (rc == TSLAM_OK && !ar.rec) rc = dev_alloc(h, (void**)&ar.rec, sizeof(TsdfArchiveRec));
    if (rc == TSLAM_OK && !h->d_arc_wTc) rc = dev_alloc(h, (void**)&h->d_arc_wTc, sizeof(double) * TSDF_MAX_FRAMES * 16);
    if (rc == TSLAM_OK && !h->d_arc_slot_of) rc = dev_alloc(h, (void**)&h->d_arc_slot_of, sizeof(int32_t) * TSDF_MAX_FRAMES);
    if (rc != TSLAM_OK) return rc;
    if (!h->arc_ev) HIPCHK(hipEventCreateWithFlags(&h->arc_ev, hipEventDisableTiming));
    ar.cap = capacity;
    if (const int rc2 = ring_clear(h); rc2 != TSLAM_OK) return rc2;
    HIPCHK(hipDeviceSynchronize());   // the null stream's memsets before any stream of the handle's
    h->arc_pair = pair;
    h->arc_rect = rect != 0;
    h->arc_interval = interval;
    h->arc_on = true;
    return TSLAM_OK;
}

int tslam_tsdf_archive_integrate(tslam_handle* h, const void* depth, int64_t stride_bytes, int n_frames, int64_t first_frame,
                                 const double* world_T_corr, const double* world_T_cam, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (!h->tsdf_on) return no_volume();
    if (!h->arc_on) return no_archive();
    if (!depth || n_frames < 0 || (n_frames > 1 && stride_bytes < 2LL * h->W * h->H)) return fail(TSLAM_EINVAL, "bad depth / stride");
    if (first_frame < 0) return fail(TSLAM_EINVAL, "first_frame must be >= 0");
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_tsdf_archive_integrate inside a batch");
    int f0;
    if (const int rc = batch_frames(h, world_T_cam, first_frame, n_frames, &f0); rc != TSLAM_OK) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const BatchCtx c = make_ctx(h);
    TsdfArgs a = integrate_args(h, pair_camera(h, h->arc_pair, h->arc_rect != 0), false);
    a.stride = stride_bytes;
    a.color_stride = stride_bytes;
    Mat4 corr{};
    if (world_T_corr) std::memcpy(corr.m, world_T_corr, sizeof(corr.m));
    for (int b0 = 0; b0 < n_frames; b0 += TSDF_MAX_FRAMES) {
        a.n = std::min(TSDF_MAX_FRAMES, n_frames - b0);
        a.depth = static_cast<const uint8_t*>(depth) + (size_t)b0 * stride_bytes;
        const double* wtc;
        if (const int rc = stage_poses(world_T_cam ? world_T_cam + (size_t)16 * b0 : nullptr, a.n, h->d_tsdf_wTc, s, &wtc); rc != TSLAM_OK) return rc;
        launch_tsdf_archive_poses(c, h->arc_pair, f0 + b0, wtc, a.n, first_frame + b0, h->arc_interval, world_T_corr != nullptr,
                                  corr, h->d_tsdf_poses, h->d_arc_wTc, s);
        launch_tsdf_posed(a, h->d_tsdf_poses, s);
        launch_tsdf_archive_put(h->arc, h->d_tsdf_poses, h->d_arc_wTc, a.n, first_frame + b0, a.depth, stride_bytes, h->W * h->H,
                                h->d_arc_slot_of, s);
        HIPCHK(hipGetLastError());
        if (world_T_cam) HIPCHK(hipStreamSynchronize(s));   // the staged host poses are reused
    }
    return TSLAM_OK;
}

int tslam_tsdf_archive_move(tslam_handle* h, int n, const int64_t* frames, const double* world_T_cam_new, double min_translation,
                            double min_rotation, void* stream) {
    if (!h || n < 0 || (n > 0 && (!frames || !world_T_cam_new))) return fail(TSLAM_EINVAL, "bad argument");
    if (const int rc = dense_open(h, "tslam_tsdf_archive_move", h->arc_on, "no depth archive (tslam_tsdf_archive_init)"); rc != TSLAM_OK) return rc;
    if (!(min_translation >= 0.0) || !std::isfinite(min_translation) || !(min_rotation >= 0.0) || !(min_rotation <= M_PI))
        return fail(TSLAM_EINVAL, "need min_translation >= 0 (finite) and 0 <= min_rotation <= pi");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = call_stream(h, stream);
    const size_t bytes = req_bytes(n);
    if (h->arc_ev_armed) {   // the copy out of the pinned requests of the move before
        HIPCHK(hipEventSynchronize(h->arc_ev));
        h->arc_ev_armed = false;
    }
    if (const int rc = pinned_reserve(h, &h->arc_pin, &h->arc_pin_cap, bytes); rc != TSLAM_OK) return rc;
    if (bytes > h->arc_req_cap) {   // grows geometrically: every growth synchronises the device
        if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
        if (const int rc = dev_grow(h, &h->d_arc_req, std::max(bytes, 2 * h->arc_req_cap), &h->arc_req_cap); rc != TSLAM_OK) return rc;
    }
    const int64_t* req_frame = static_cast<const int64_t*>(h->d_arc_req);
    const double* req_wTc = reinterpret_cast<const double*>(req_frame + n);
    if (n > 0) {
        std::memcpy(h->arc_pin, frames, sizeof(int64_t) * (size_t)n);
        std::memcpy(static_cast<int64_t*>(h->arc_pin) + n, world_T_cam_new, sizeof(double) * 16 * (size_t)n);
        HIPCHK(hipMemcpyAsync(h->d_arc_req, h->arc_pin, bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipEventRecord(h->arc_ev, s));
        h->arc_ev_armed = true;
    }
    const TsdfArgs a = integrate_args(h, pair_camera(h, h->arc_pair, h->arc_rect != 0), false);
    launch_tsdf_archive_move(h->arc, a, req_frame, req_wTc, n, min_translation * min_translation, 1.0 + 2.0 * std::cos(min_rotation), s);
    HIPCHK(hipGetLastError());
    h->esdf_valid = false;
    return TSLAM_OK;
}

// archive order: the oldest frame in the ring first
int tslam_tsdf_archive_read(tslam_handle* h, int max_frames, int64_t* frames, double* world_T_cam, int* count, int* moved_last,
                            int64_t* moved_total) {
    if (!h || max_frames < 0) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (count) *count = 0;
    if (moved_last) *moved_last = 0;
    if (moved_total) *moved_total = 0;
    if (!h->arc_on) return TSLAM_OK;   // no archive, or one whose volume was replaced: nothing archived
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    TsdfArchiveRec rec;
    HIPCHK(hipMemcpy(&rec, h->arc.rec, sizeof(rec), hipMemcpyDeviceToHost));
    const int cap = h->arc.cap, m = (int)std::min<int64_t>(rec.count, cap);
    if (count) *count = m;
    if (moved_last) *moved_last = rec.moved_last;
    if (moved_total) *moved_total = rec.moved_total;
    const int n = std::min(m, max_frames);
    if (n < 1 || (!frames && !world_T_cam)) return TSLAM_OK;
    // the ring in two copies, then put into archive order
    std::vector<int64_t> ring_frame(frames ? (size_t)cap : 0);
    std::vector<double> ring_wTc(world_T_cam ? (size_t)cap * 16 : 0);
    if (frames) HIPCHK(hipMemcpy(ring_frame.data(), h->arc.frame, sizeof(int64_t) * cap, hipMemcpyDeviceToHost));
    if (world_T_cam) HIPCHK(hipMemcpy(ring_wTc.data(), h->arc.wTc, sizeof(double) * 16 * cap, hipMemcpyDeviceToHost));
    for (int a = 0; a < n; ++a) {
        const size_t slot = (size_t)((rec.count - m + a) % cap);
        if (frames) frames[a] = ring_frame[slot];
        if (world_T_cam) std::memcpy(world_T_cam + (size_t)16 * a, ring_wTc.data() + 16 * slot, sizeof(double) * 16);
    }
    return TSLAM_OK;
}

int tslam_tsdf_archive_read_depth(tslam_handle* h, int index, uint16_t* depth) {
    if (!h || !depth) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->arc_on) return no_archive();
    if (const int rc = dense_quiesce(h); rc != TSLAM_OK) return rc;
    TsdfArchiveRec rec;
    HIPCHK(hipMemcpy(&rec, h->arc.rec, sizeof(rec), hipMemcpyDeviceToHost));
    const int cap = h->arc.cap, m = (int)std::min<int64_t>(rec.count, cap);
    if (index < 0 || index >= m) return fail(TSLAM_EINVAL, "index must be 0 .. the archive's count - 1");
    const size_t slot = (size_t)((rec.count - m + index) % cap);
    HIPCHK(hipMemcpy(depth, h->arc.depth + slot * (size_t)h->arc.slot_stride, 2 * (size_t)h->W * h->H, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

}  // extern "C"
