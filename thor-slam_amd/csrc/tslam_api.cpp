// tslam_api.cpp — the core of the C-ABI of libtslam_hip.so (declared in include/tslam.h): the
// handle's workspace and lifecycle, the frame pipeline and its stage table, reads, the rig, the
// motion prior and the asynchronous host boundary.  Local BA, the shard exchange, relocalisation /
// loop closure and the dense map live in tslam_api_{ba,exchange,loop,tsdf,render,stereo,dense}.cpp.
//
// Owns the device workspace of one handle and sequences the stage kernels of a batch on the
// caller's stream.  The launch functions never allocate, copy synchronously or synchronise, so
// a batch can be captured into a hipGraph by the caller.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "tslam_describe.h"
#include "tslam_handle.h"
#include "tslam_tables.h"

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int tslam_internal_fail(int code, const char* msg) { return fail(code, msg); }

int dev_alloc(tslam_handle* h, void** p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(TSLAM_ENOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
    h->allocs.push_back(*p);
    HIPCHK(hipMemset(*p, 0, bytes));
    // hipMemset is ordered on the null stream only: the handle's non-blocking streams (and the
    // caller's) could otherwise write the buffer before the zeroing lands on it
    HIPCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

// A buffer back to the device: freed, forgotten by the handle, its pointer null (null: nothing to do)
void dev_release(tslam_handle* h, void** p) {
    if (!*p) return;
    (void)hipFree(*p);
    h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), *p), h->allocs.end());
    *p = nullptr;
}

// The device grow helper: a buffer below `need` bytes (*cap; without `cap`, any buffer) is released
// and allocated afresh, zeroed, at exactly `need`
int dev_grow(tslam_handle* h, void** p, size_t need, size_t* cap) {
    if (cap && *cap >= need && *p) return TSLAM_OK;
    dev_release(h, p);
    const int rc = dev_alloc(h, p, need);
    if (cap) *cap = rc == TSLAM_OK ? need : 0;
    return rc;
}

// Grows geometrically (and to at least 4 KiB): a job slot's buffer is reallocated O(log) times as
// the vote window or the pose-graph span grows, not on every job (a pinned allocation and free
// cost ~0.2 ms of the submitting thread).
int pinned_reserve(tslam_handle* h, void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return TSLAM_OK;
    bytes = std::max({bytes, 2 * *cap, (size_t)4096});
    if (*p) {
        (void)hipHostFree(*p);
        h->host_allocs.erase(std::remove(h->host_allocs.begin(), h->host_allocs.end(), *p), h->host_allocs.end());
        *p = nullptr;
        *cap = 0;
    }
    HIPCHK(hipHostMalloc(p, bytes, hipHostMallocDefault));
    h->host_allocs.push_back(*p);
    *cap = bytes;
    return TSLAM_OK;
}

static void free_all(tslam_handle* h) {
    if (h->drv && h->drv_owned) tslam_internal_driver_destroy(h->drv);
    h->drv = nullptr;
    for (void* p : h->allocs) (void)hipFree(p);
    h->allocs.clear();
    for (void* p : h->host_allocs) (void)hipHostFree(p);
    h->host_allocs.clear();
}

static void build_geometry(tslam_handle* h) {
    LevelGeom& g = h->g;
    const tslam_params& p = h->prm;
    g.n_levels = p.n_levels;
    g.K = p.n_features;
    int w = h->W, hh = h->H, off = 0;
    double tot = 0.0;
    for (int l = 0; l < p.n_levels; ++l) tot += std::pow(0.25, l);
    int sumq = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        g.W[l] = w;
        g.H[l] = hh;
        g.pyr_off[l] = off;
        off += w * hh;
        w >>= 1;
        hh >>= 1;
        g.Kq[l] = (int)((double)p.n_features * std::pow(0.25, l) / tot);
        if (l > 0) sumq += g.Kq[l];
    }
    g.Kq[0] = p.n_features - sumq;
    g.pyr_bytes = (off + 15) & ~15;
    int ko = 0, bs = 0, co = 0, qs = 0;
    // detect band height at level 0: the tallest of 32 / 24 / 16 rows whose band (2 * rows + 10
    // rows of W bytes of LDS) keeps 3 (W <= 640) or 2 (W <= 1280) blocks per CU; measured 778 ->
    // 690 us at 640x400 (32 rows) and 611 -> 575 us at 1280x800 (24 rows) against 16.  Coarser
    // levels take taller bands in the same LDS budget (fewer blocks and halo rows, similar pixels
    // per block), equalised over the level's rows: 640x400 -> 32 / 68 / 100 / 50 rows, 26 -> 18
    // blocks per image, 662 -> 625 us per 256-frame batch
    const int br0 = (2 * TS_BAND_ROWS_MAX + 10) * g.W[0] <= 48 * 1024 ? TS_BAND_ROWS_MAX
                  : (2 * 24 + 10) * g.W[0] <= 78 * 1024 ? 24 : 16;
    const int det_budget = (2 * br0 + 10) * g.W[0];
    g.det_lds = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        // <= 124 rows: detect's phase-B queue entries hold the score row (< 128) in 7 bits and the
        // quad (< 512, so W <= 2044) in 9
        const int maxr = l == 0 ? br0 : std::max(br0, std::min(124, (det_budget / g.W[l] - 10) / 2));
        const int nb = (g.H[l] + maxr - 1) / maxr;
        g.band_rows[l] = l == 0 ? br0 : ((g.H[l] + nb - 1) / nb + 1) & ~1;
        g.smooth_groups[l] = std::max(2, g.band_rows[l] / 16);
        g.det_lds = std::max(g.det_lds, (2 * g.band_rows[l] + 10) * g.W[l]);
    }
    g.dt_total = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        g.koff[l] = ko;
        ko += g.Kq[l];
        g.nbands[l] = (g.H[l] + g.band_rows[l] - 1) / g.band_rows[l];
        g.band_start[l] = bs;
        bs += g.nbands[l];
        g.cand_cap[l] = ((g.band_rows[l] + 1) / 2) * (g.W[l] / 2 + 1);
        g.cand_off[l] = co;
        co += g.nbands[l] * g.cand_cap[l];
        // describe tiles (origins at multiples of the tile size): the tile columns and rows up to
        // the last that meets the keypoint band [margin, W - margin) x [margin, H - margin).
        // 640x400: level 0's rows 384..399 and level 1's 192..199 hold no keypoint, 52 -> 44
        // blocks per image
        g.dt_nx[l] = (g.W[l] - p.edge_margin + TS_DT_W - 1) / TS_DT_W;
        g.dt_start[l] = g.dt_total;
        g.dt_total += g.dt_nx[l] * ((g.H[l] - p.edge_margin + TS_DT_H - 1) / TS_DT_H);
        g.qtiles[l] = (g.Kq[l] + 127) / 128;   // k_match: TS_MQ queries per block
        g.qtile_start[l] = qs;
        qs += g.qtiles[l];
    }
    g.total_bands = bs;
    g.cand_total = co;
    g.total_qtiles = qs;
    int ro = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        g.rs_off[l] = ro;
        ro += g.H[l] + 1;
    }
    g.rs_total = (ro + 7) & ~7;
}

BatchCtx make_ctx(tslam_handle* h) {
    BatchCtx c{};
    c.g = h->g;
    c.C = h->C;
    c.P = h->P;
    c.B = h->B;
    c.R = h->R;
    c.n = h->cur_n;
    ctx_set_first_frame(c, h->cur_g0);
    c.W = h->W;
    c.H = h->H;
    c.cpp = h->prm.rgbd ? 1 : 2;
    c.rgbd = h->prm.rgbd;
    c.images = h->prm.rgbd ? h->d_gray : h->cur_images;
    c.rgbd_in = h->prm.rgbd ? h->cur_images : nullptr;
    c.maps = h->d_maps;
    c.map_mask = h->map_mask;
    c.pyr = (uint8_t*)h->buf[TSLAM_BUF_PYRAMID].ptr;
    c.smo = (uint8_t*)h->buf[TSLAM_BUF_SMOOTH].ptr;
    c.cand = h->d_cand;
    c.ccount = h->d_ccount;
    c.hist = h->d_hist;
    c.kps = (uint32_t*)h->buf[TSLAM_BUF_KEYPOINTS].ptr;
    c.kcount = (int32_t*)h->buf[TSLAM_BUF_KCOUNT].ptr;
    c.desc = (uint32_t*)h->buf[TSLAM_BUF_DESC].ptr;
    c.ys = (uint4*)h->buf[TSLAM_BUF_YSORTED].ptr;
    c.desc_ys = (uint32_t*)h->buf[TSLAM_BUF_DESC_YS].ptr;
    c.rowstart = (uint16_t*)h->buf[TSLAM_BUF_ROWSTART].ptr;
    c.qbest = (uint32_t*)h->buf[TSLAM_BUF_QBEST].ptr;
    c.qsecond = (uint32_t*)h->buf[TSLAM_BUF_QSECOND].ptr;
    c.tbest = (uint32_t*)h->buf[TSLAM_BUF_TBEST].ptr;
    c.ypos = (uint16_t*)h->buf[TSLAM_BUF_YPOS].ptr;
    c.qtpos = (uint16_t*)h->buf[TSLAM_BUF_QTPOS].ptr;
    c.stereo = (int32_t*)h->buf[TSLAM_BUF_STEREO].ptr;
    c.disp = (double*)h->buf[TSLAM_BUF_DISP].ptr;
    c.temporal = (int32_t*)h->buf[TSLAM_BUF_TEMPORAL].ptr;
    c.tuv = (double*)h->buf[TSLAM_BUF_TEMPORAL_UV].ptr;
    c.corr = (double*)h->buf[TSLAM_BUF_CORR].ptr;
    c.pose = (double*)h->buf[TSLAM_BUF_POSE].ptr;
    c.stats = (int32_t*)h->buf[TSLAM_BUF_STATS].ptr;
    c.state = h->d_state;
    c.prior = h->prior_armed ? h->d_prior + (size_t)(h->batch_idx & 1) * TS_PRIOR_DOUBLES * h->P * h->B : nullptr;
    c.rig_E = h->d_rig_E;
    c.rig_Einv = h->d_rig_E ? h->d_rig_E + 16 * h->rig_q : nullptr;
    c.rig_pose = h->d_rig_pose;
    c.rig_stats = h->d_rig_stats;
    c.rig_state = h->d_rig_state;
    c.rig_prior = (h->prior_armed && h->d_rig_prior) ? h->d_rig_prior + (size_t)(h->batch_idx & 1) * TS_PRIOR_DOUBLES * h->B
                                                     : nullptr;
    c.ransac = h->d_ransac;
    c.hyp = h->d_hyp;
    c.det_thr = (const uint32_t*)h->buf[TSLAM_BUF_DET_THR].ptr;
    c.det_thr_acc = h->d_det_thr_acc;
    c.det_fail = (uint32_t*)h->buf[TSLAM_BUF_DET_FAIL].ptr;
    c.brief_table = h->d_brief;
    c.wedges = h->d_wedges;
    c.dt_tile = h->d_dt_tile;
    for (int p = 0; p < h->P; ++p) c.calib[p] = h->calib[p];
    c.mp.max_hamming = h->prm.max_hamming;
    c.mp.ratio_pct = h->prm.ratio_pct;
    c.mp.row_tol = h->prm.stereo_row_tol;
    c.mp.max_disp = h->prm.max_disparity;
    c.mp.window = h->prm.temporal_window;
    c.mp.refine_split = h->prm.match_refine;
    c.mp.merge_cap = h->match_mode == 1 ? 0 : h->match_cap > 0 ? std::min(h->match_cap, TS_MTB) : TS_MTB;
    c.mp.split = h->match_split;
    c.match_cnt = h->d_match_cnt;
    c.det_cnt = h->d_det_cnt;
    c.pp.n_hyp = h->prm.ransac_hypotheses;
    c.pp.iters = h->prm.refine_iters;
    c.pp.min_inliers = h->prm.min_inliers;
    c.pp.splits = h->prm.ransac_splits;
    c.pp.mode = h->prm.ransac_mode;
    c.pp.refine_block = h->prm.refine_block;
    c.pp.thr2 = h->prm.ransac_thr_px * h->prm.ransac_thr_px;
    c.pp.seed = h->prm.ransac_seed;
    c.fast_threshold = h->prm.fast_threshold;
    c.margin = h->prm.edge_margin;
    c.dt_list_cap = h->dt_list_cap > 0 ? std::min(h->dt_list_cap, TS_DT_LIST) : TS_DT_LIST;
    ctx_set_views(c, h->sh_cam_lo, h->sh_cam_hi - h->sh_cam_lo, 0, h->P);
    c.match_modes = 3;
    c.reloc = 0;
    c.peer_S = c.peer_me = c.peer_nbuf = c.peer_skip = 0;
    return c;
}

// -- the stage table: the pipeline order, written once ----------------------------------------------
// The front stages are the same on every path (a sharded stereo handle never has prm.rgbd set).
int run_front_stage(tslam_handle* h, const BatchCtx& c, int stage, hipStream_t s) {
    switch (stage) {
        case TSLAM_STAGE_RECTIFY:
        case TSLAM_KERNEL_RECTIFY_PYRAMID:
            if (h->prm.rgbd) launch_rgbd_gray(c, h->d_gray, s);   // the colour images become the gray input of rectify
            launch_rectify_pyramid(c, s);
            return 1;
        case TSLAM_STAGE_DETECT: launch_detect(c, s); launch_select(c, s, h->sel_mode, h->sel_rcap); return 1;
        case TSLAM_KERNEL_DETECT: launch_detect(c, s); return 1;
        case TSLAM_KERNEL_SELECT: launch_select(c, s, h->sel_mode, h->sel_rcap); return 1;
        case TSLAM_STAGE_DESCRIBE:
        case TSLAM_KERNEL_DESCRIBE: launch_describe(c, s); return 1;
        default: return 0;
    }
}

// The back stages on the contexts of `v` (BackView); the chains always cover the whole batch `c`.
int run_back_stage(tslam_handle* h, const BatchCtx& c, const BackView& v, int stage, hipStream_t s) {
    switch (stage) {
        case TSLAM_STAGE_MATCH:
            if (v.pre) launch_match_stereo(*v.pre, s);
            if (v.b) {
                launch_match(*v.b, s);
                launch_match_refine(*v.b, s);
            }
            return 1;
        case TSLAM_KERNEL_MATCH:
            if (v.pre) launch_match_stereo(*v.pre, s);
            if (v.b) launch_match(*v.b, s);
            return 1;
        case TSLAM_KERNEL_MATCH_REFINE:
            if (v.b) launch_match_refine(*v.b, s);
            return 1;
        case TSLAM_STAGE_POSE:
            if (v.b) launch_pose(*v.b, s);
            if (v.pose_rig && h->rig && v.rig) launch_rig_pose(*v.rig, s);
            if (v.pose_chain) {
                launch_chains(c, h->rig, s);
                loop_auto_store(h, c, s);
            }
            return 1;
        case TSLAM_KERNEL_POSE:
            if (v.b) launch_pose(*v.b, s);
            return 1;
        case TSLAM_KERNEL_RIG:
            if (!h->rig) return fail(TSLAM_ESTATE, "no rig set (tslam_set_rig)");
            if (v.rig) launch_rig_pose(*v.rig, s);
            return 1;
        case TSLAM_KERNEL_CHAIN: launch_chains(c, h->rig, s); return 1;
        default: return 0;
    }
}

extern "C" {

const char* tslam_last_error(void) { return g_err.c_str(); }

int tslam_abi_version(void) { return TSLAM_ABI_VERSION; }

int tslam_create(const tslam_stereo_desc* pairs, const tslam_params* params, int device, tslam_handle** out) {
    if (!pairs || !params || !out) return fail(TSLAM_EINVAL, "null argument");
    const tslam_params& p = *params;
    if (p.n_pairs < 1 || p.n_pairs > 8) return fail(TSLAM_EINVAL, "n_pairs must be in [1, 8]");
    if (p.n_levels < 1 || p.n_levels > TS_MAX_LEVELS) return fail(TSLAM_EINVAL, "n_levels must be in [1, 6]");
    if (p.n_features < 1 || p.n_features > 8192) return fail(TSLAM_EINVAL, "n_features must be in [1, 8192]");
    if (p.ransac_hypotheses < 1 || p.ransac_hypotheses > 256) return fail(TSLAM_EINVAL, "ransac_hypotheses must be in [1, 256]");
    if (p.edge_margin < 19) return fail(TSLAM_EINVAL, "edge_margin must be >= 19");
    if (p.fast_threshold < 0 || p.fast_threshold > 254) return fail(TSLAM_EINVAL, "fast_threshold must be in [0, 254]");
    if (p.max_batch < 1) return fail(TSLAM_EINVAL, "max_batch must be >= 1");
    if (p.max_hamming < 0 || p.max_hamming > 253) return fail(TSLAM_EINVAL, "max_hamming must be in [0, 253]");
    // k_match packs the gate offsets into 16-bit halves (query xy + window < 2^15)
    if (p.stereo_row_tol < 0 || p.stereo_row_tol > 2047 || p.max_disparity < 0 || p.max_disparity > 2047 ||
        p.temporal_window < 0 || p.temporal_window > 2047)
        return fail(TSLAM_EINVAL, "stereo_row_tol, max_disparity, temporal_window must be in [0, 2047]");
    if (!(p.ba_window == 0 || (p.ba_window >= 2 && p.ba_window <= TS_BA_MAXW)))
        return fail(TSLAM_EINVAL, "ba_window must be 0 (off) or in [2, 10]");
    if (p.ba_window && (p.ba_kf_interval < 1 || p.ba_iters < 1 || !(p.ba_lambda >= 0.0) || !(p.ba_outlier_px > 0.0)))
        return fail(TSLAM_EINVAL, "ba_kf_interval, ba_iters >= 1, ba_lambda >= 0, ba_outlier_px > 0");
    if (p.refine_iters < 1) return fail(TSLAM_EINVAL, "refine_iters must be >= 1");
    if (p.ransac_splits < 0 || p.ransac_splits > TS_MAX_SPLITS) return fail(TSLAM_EINVAL, "ransac_splits must be in [0, 32]");
    if (p.ransac_mode < 0 || p.ransac_mode > 2) return fail(TSLAM_EINVAL, "ransac_mode must be 0, 1 or 2");
    if (p.refine_block != 0 && p.refine_block != 128 && p.refine_block != 256)
        return fail(TSLAM_EINVAL, "refine_block must be 0, 128 or 256");
    if (p.match_refine != 0 && p.match_refine != 1) return fail(TSLAM_EINVAL, "match_refine must be 0 or 1");
    const int W = pairs[0].width, H = pairs[0].height;
    if (W < 64 || H < 64 || W > 2047 || H > 2047) return fail(TSLAM_EINVAL, "image size must be within [64, 2047]");
    for (int i = 1; i < p.n_pairs; ++i)
        if (pairs[i].width != W || pairs[i].height != H) return fail(TSLAM_EINVAL, "all pairs must share the image size");
    if ((H >> (p.n_levels - 1)) < 2 * p.edge_margin + 3 || (W >> (p.n_levels - 1)) < 2 * p.edge_margin + 3)
        return fail(TSLAM_EINVAL, "coarsest pyramid level smaller than 2*edge_margin+3");
    for (int i = 0; i < p.n_pairs; ++i)
        if (!(p.rgbd || pairs[i].baseline > 0.0) || !(pairs[i].fx > 0.0) || !(pairs[i].fy > 0.0))
            return fail(TSLAM_EINVAL, "pair calibration needs fx, fy, baseline > 0");
    if (p.rgbd != 0 && p.rgbd != 1) return fail(TSLAM_EINVAL, "rgbd must be 0 or 1");
    if (p.rgbd && ((W * H) & 1)) return fail(TSLAM_EINVAL, "RGB-D needs an even pixel count (u16 depth alignment)");

    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail(TSLAM_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

    tslam_handle* h = new tslam_handle();
    h->device = device;
    h->prm = p;
    h->W = W;
    h->H = H;
    h->P = p.n_pairs;
    h->C = (p.rgbd ? 1 : 2) * p.n_pairs;
    h->B = p.max_batch;
    h->sh_cam_hi = h->C;
    // the ring keeps frame t-1 of a batch's first frame while the front stages of the next batch
    // run (front / back on two streams): R = 2B + 1
    h->R = 2 * p.max_batch + 1;
    // with BA the ring also keeps the frames a keyframe's temporal match chain walks back over,
    // even while the next batch runs (BA may run on its own stream): R = 2B + interval + 1
    if (p.ba_window) h->R = 2 * p.max_batch + p.ba_kf_interval + 1;
    build_geometry(h);
    for (int i = 0; i < h->P; ++i) {
        h->calib[i].fx = pairs[i].fx;
        h->calib[i].fy = pairs[i].fy;
        h->calib[i].cx = pairs[i].cx;
        h->calib[i].cy = pairs[i].cy;
        h->calib[i].fxb = pairs[i].fx * (p.rgbd ? 1.0 : pairs[i].baseline);   // RGB-D: virtual 1 m baseline
    }

    const int64_t K = p.n_features, C = h->C, P = h->P, B = h->B, R = h->R, L = p.n_levels;
    struct Spec {
        int which;
        int64_t frames;
        int64_t per_frame;
    } specs[] = {
        {TSLAM_BUF_PYRAMID, R, C * h->g.pyr_bytes},
        {TSLAM_BUF_SMOOTH, B, C * h->g.pyr_bytes},
        {TSLAM_BUF_KEYPOINTS, R, C * K * 2 * 4},
        {TSLAM_BUF_KCOUNT, R, C * L * 4},
        {TSLAM_BUF_DESC, R, C * K * 8 * 4},
        {TSLAM_BUF_STEREO, R, P * K * 4},
        {TSLAM_BUF_DISP, R, P * K * 8},
        {TSLAM_BUF_TEMPORAL, R, P * K * 4},
        {TSLAM_BUF_TEMPORAL_UV, B, P * K * 2 * 8},
        {TSLAM_BUF_CORR, B, P * K * TS_CORR_DOUBLES * 8},
        {TSLAM_BUF_POSE, B, P * TS_POSE_DOUBLES * 8},
        {TSLAM_BUF_STATS, B, P * TS_STATS_INTS * 4},
        {TSLAM_BUF_QBEST, B, P * 2 * K * 4},
        {TSLAM_BUF_QSECOND, B, P * 2 * K * 4},
        {TSLAM_BUF_TBEST, B, P * 2 * K * 4},
        {TSLAM_BUF_YSORTED, R, C * K * 16},
        {TSLAM_BUF_DESC_YS, R, C * K * 8 * 4},
        {TSLAM_BUF_ROWSTART, R, C * (int64_t)h->g.rs_total * 2},
        {TSLAM_BUF_DET_THR, 1, C * L * 4},
        {TSLAM_BUF_DET_FAIL, B, C * L * 4},
        {TSLAM_BUF_YPOS, R, C * K * 2},
        {TSLAM_BUF_QTPOS, B, P * 2 * K * 2},
        {TSLAM_BUF_HYP, B, P * 4 * (int64_t)p.ransac_hypotheses * TS_HYP_DOUBLES * 8},
    };
    int rc = TSLAM_OK;
    for (const Spec& s : specs) {
        Buffer& b = h->buf[s.which];
        b.per_frame = s.per_frame;
        b.bytes = s.per_frame * s.frames;
        if ((rc = dev_alloc(h, &b.ptr, (size_t)b.bytes)) != TSLAM_OK) break;
    }
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_cand, sizeof(uint32_t) * (size_t)B * C * h->g.cand_total);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_ccount, sizeof(uint32_t) * (size_t)B * C * h->g.total_bands);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_hist, sizeof(uint32_t) * (size_t)B * C * L * 256);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_det_thr_acc, sizeof(uint32_t) * (size_t)C * L);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_state, sizeof(double) * 32 * (size_t)P);   // chain (A, Q) per pair
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_ransac, sizeof(uint32_t) * TS_RANSAC_WORDS * TS_MAX_SPLITS * (size_t)B * P);
    if (rc == TSLAM_OK) h->d_hyp = (double*)h->buf[TSLAM_BUF_HYP].ptr;
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_brief, sizeof(TSLAM_BRIEF_TABLE));
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_wedges, sizeof(TSLAM_WEDGES));
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_dt_tile, sizeof(uint32_t) * (size_t)h->g.dt_total);
    if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_maps, sizeof(int32_t) * (size_t)C * W * H * 2);
    if (rc == TSLAM_OK && p.ba_window) rc = alloc_ba(h);
    if (rc == TSLAM_OK && p.rgbd) rc = dev_alloc(h, (void**)&h->d_gray, (size_t)B * P * W * H);
    if (rc != TSLAM_OK) {
        free_all(h);
        delete h;
        return rc;
    }
    // the describe kernel reads the rotated pattern as byte offsets from the patch origin
    // (x - 18, y - 18) in its LDS tile: (py + 18) * TS_DT_P + px + 18 for both points, packed
    // low | high << 16
    std::vector<uint32_t> brief_off(30 * 256);
    for (int i = 0; i < 30 * 256; ++i) {
        const uint32_t t = TSLAM_BRIEF_TABLE[i];
        const int px = (int8_t)(t & 0xFF), py = (int8_t)((t >> 8) & 0xFF);
        const int qx = (int8_t)((t >> 16) & 0xFF), qy = (int8_t)(t >> 24);
        brief_off[i] = (uint32_t)((py + 18) * TS_DT_P + px + 18) | ((uint32_t)((qy + 18) * TS_DT_P + qx + 18) << 16);
    }
    bool ok = hipMemcpy(h->d_brief, brief_off.data(), sizeof(uint32_t) * brief_off.size(), hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(h->d_wedges, TSLAM_WEDGES, sizeof(TSLAM_WEDGES), hipMemcpyHostToDevice) == hipSuccess;
    std::vector<uint32_t> dt_tile(h->g.dt_total);
    describe_tile_table(h->g, dt_tile.data());
    ok = ok && hipMemcpy(h->d_dt_tile, dt_tile.data(), sizeof(uint32_t) * dt_tile.size(), hipMemcpyHostToDevice) == hipSuccess;
    for (int i = 0; i < h->P && ok; ++i) {
        const int32_t* m[2] = {pairs[i].map_left, pairs[i].map_right};
        const int cpp = p.rgbd ? 1 : 2;
        for (int s = 0; s < cpp; ++s) {
            if (!m[s]) continue;
            h->map_mask |= 1u << (cpp * i + s);
            ok = ok && hipMemcpy(h->d_maps + (size_t)(cpp * i + s) * W * H * 2, m[s], sizeof(int32_t) * (size_t)W * H * 2,
                                 hipMemcpyHostToDevice) == hipSuccess;
        }
    }
    if (!ok) {
        free_all(h);
        delete h;
        return fail(TSLAM_EHIP, "uploading tables / maps failed");
    }
    if (tslam_reset(h) != TSLAM_OK) {
        free_all(h);
        delete h;
        return TSLAM_EHIP;
    }
    *out = h;
    return TSLAM_OK;
}

int tslam_destroy(tslam_handle* h) {
    if (!h) return TSLAM_OK;
    (void)ba_flush(h);   // destroyed whatever the deferred BA reports
    loop_worker_stop(h);   // its queued jobs reach the loop stream before the device is drained
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    loop_destroy(h);
    for (hipEvent_t e : {h->ev_front, h->ev_back[0], h->ev_back[1], h->ev_prior[0], h->ev_prior[1], h->as_staged[0],
                         h->as_staged[1], h->as_res[0].ev, h->as_res[1].ev})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : {h->as_front, h->as_back, h->as_ba})
        if (st) (void)hipStreamDestroy(st);
    ba_destroy(h);   // its events, then the graph cache
    register_destroy(h);
    archive_destroy(h);
    free_all(h);
    delete h;
    return TSLAM_OK;
}

// Every subsystem resets the session state it owns (ba_reset, dense_reset, loop_reset); the dense
// stereo depth slots are no session state and stay.
int tslam_reset(tslam_handle* h) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    loop_worker_drain(h);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> eye(32 * (size_t)h->P, 0.0);   // every chain's (A, Q) = (I, I)
    for (int q = 0; q < 2 * h->P; ++q)
        for (int k = 0; k < 4; ++k) eye[(size_t)q * 16 + 5 * k] = 1.0;
    HIPCHK(hipMemcpy(h->d_state, eye.data(), sizeof(double) * eye.size(), hipMemcpyHostToDevice));
    if (h->d_rig_state) HIPCHK(hipMemcpy(h->d_rig_state, eye.data(), sizeof(double) * 32, hipMemcpyHostToDevice));
    h->frames_done = 0;
    // the speculative FAST threshold starts exact (t + 1) and learns from the first batch
    HIPCHK(hipMemset(h->buf[TSLAM_BUF_DET_THR].ptr, 0, sizeof(uint32_t) * (size_t)h->C * h->g.n_levels));
    HIPCHK(hipMemset(h->d_det_thr_acc, 0xFF, sizeof(uint32_t) * (size_t)h->C * h->g.n_levels));
    int rc = ba_reset(h);
    if (rc == TSLAM_OK) rc = dense_reset(h);
    if (rc == TSLAM_OK) rc = loop_reset(h);
    if (rc != TSLAM_OK) return rc;
    h->back_pending[0] = h->back_pending[1] = false;
    h->in_batch = false;
    h->cur_n = 0;
    for (auto& r : h->as_res) r.pending = false;   // results of batches before the reset are dropped
    h->as_last_pose_batch = h->as_batches - 1;
    // hipMemset runs on the null stream, which the handle's non-blocking streams do not wait for
    HIPCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

// -- asynchronous host boundary -------------------------------------------------------------------
static int64_t host_frame_bytes(const tslam_handle* h) {
    return h->prm.rgbd ? (int64_t)h->P * 5 * h->W * h->H : (int64_t)h->C * h->W * h->H;
}

// pinned result slots per batch parity (tslam_poll_batch / tslam_poll_pose read them)
static int ensure_result_slots(tslam_handle* h) {
    if (h->as_res[0].ev) return TSLAM_OK;
    const size_t B = h->B, P = h->P;
    for (int k = 0; k < 2; ++k) {
        auto& r = h->as_res[k];
        const size_t bytes[4] = {8 * B * P * TS_POSE_DOUBLES, 4 * B * P * TS_STATS_INTS, 8 * B * TS_POSE_DOUBLES,
                                 4 * B * TS_STATS_INTS};
        void** dst[4] = {(void**)&r.pose, (void**)&r.stats, (void**)&r.rig_pose, (void**)&r.rig_stats};
        for (int i = 0; i < 4; ++i) {
            HIPCHK(hipHostMalloc(dst[i], bytes[i], hipHostMallocDefault));
            h->host_allocs.push_back(*dst[i]);
        }
        r.ts.assign(B, 0.0);
        HIPCHK(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
    }
    return TSLAM_OK;
}

static int ensure_async(tslam_handle* h) {
    if (h->as_front) return TSLAM_OK;
    int rc = ensure_result_slots(h);
    if (rc != TSLAM_OK) return rc;
    int lo = 0, hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    if (h->prm.ba_window) {
        // local BA: its chain of small dependent launches (one-block solves, ~135-block Schur
        // passes) runs on a stream of its own, and the front / back kernels stay off the last
        // TS_BA_CU_RESERVE CUs so those launches find free CUs beside the next batch's front end
        // (C4: 15.1k -> 16.2k frames/s, bench.py --front-cu-reserve sweep)
        int n_cu = 0;
        HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, h->device));
        const int keep = n_cu > 2 * TS_BA_CU_RESERVE ? n_cu - TS_BA_CU_RESERVE : n_cu;
        std::vector<uint32_t> mask((size_t)(n_cu + 31) / 32, 0u);
        for (int cu = 0; cu < keep; ++cu) mask[(size_t)cu / 32] |= 1u << (cu % 32);
        HIPCHK(hipExtStreamCreateWithCUMask(&h->as_front, (uint32_t)mask.size(), mask.data()));
        HIPCHK(hipExtStreamCreateWithCUMask(&h->as_back, (uint32_t)mask.size(), mask.data()));
        HIPCHK(hipStreamCreateWithPriority(&h->as_ba, hipStreamNonBlocking, hi));
    } else {
        HIPCHK(hipStreamCreateWithPriority(&h->as_front, hipStreamNonBlocking, hi));   // front = critical path
        HIPCHK(hipStreamCreateWithFlags(&h->as_back, hipStreamNonBlocking));
    }
    const size_t in_bytes = (size_t)h->B * host_frame_bytes(h);
    for (int k = 0; k < 2; ++k) {
        void* p = nullptr;
        HIPCHK(hipHostMalloc(&p, in_bytes, hipHostMallocDefault));
        h->host_allocs.push_back(p);
        h->as_stage[k] = (uint8_t*)p;
        rc = dev_alloc(h, (void**)&h->as_input[k], in_bytes);
        if (rc != TSLAM_OK) return rc;
        HIPCHK(hipEventCreateWithFlags(&h->as_staged[k], hipEventDisableTiming));
    }
    return TSLAM_OK;
}

// The current batch's results into the pinned slot of its parity on stream s (an unread batch s-2
// there is dropped), for tslam_poll_batch / tslam_poll_pose.  Timestamps: `ts` or frame indices.
static int stash_results(tslam_handle* h, const double* ts, hipStream_t s) {
    int rc = ensure_result_slots(h);
    if (rc != TSLAM_OK) return rc;
    const int k = (int)(h->as_batches & 1);
    auto& r = h->as_res[k];
    const size_t n = h->cur_n, P = h->P;
    HIPCHK(hipMemcpyAsync(r.pose, h->buf[TSLAM_BUF_POSE].ptr, 8 * n * P * TS_POSE_DOUBLES, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(r.stats, h->buf[TSLAM_BUF_STATS].ptr, 4 * n * P * TS_STATS_INTS, hipMemcpyDeviceToHost, s));
    if (h->rig) {
        HIPCHK(hipMemcpyAsync(r.rig_pose, h->d_rig_pose, 8 * n * TS_POSE_DOUBLES, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(r.rig_stats, h->d_rig_stats, 4 * n * TS_STATS_INTS, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipEventRecord(r.ev, s));
    for (size_t i = 0; i < n; ++i) r.ts[i] = ts ? ts[i] : (double)(h->cur_g0 + (int64_t)i);
    r.batch = h->as_batches;
    r.g0 = h->cur_g0;
    r.n = (int)n;
    r.pending = true;
    h->as_batches += 1;
    return TSLAM_OK;
}

int tslam_host_stage(tslam_handle* h, uint8_t** stage, int64_t* frame_bytes) {
    if (!h || !stage) return fail(TSLAM_EINVAL, "bad argument");
    if (h->sh_world > 1 || h->sh_comm) return fail(TSLAM_ESTATE, "a sharded handle is driven stage by stage");
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_async(h);
    if (rc != TSLAM_OK) return rc;
    const int k = (int)(h->as_batches & 1);
    if (h->as_staged_armed[k]) {
        HIPCHK(hipEventSynchronize(h->as_staged[k]));
        h->as_staged_armed[k] = false;
    }
    *stage = (uint8_t*)h->as_stage[k];
    if (frame_bytes) *frame_bytes = host_frame_bytes(h);
    return TSLAM_OK;
}

int tslam_submit_host(tslam_handle* h, const uint8_t* host_images, const double* timestamps, int n_frames) {
    if (!h || !host_images) return fail(TSLAM_EINVAL, "bad argument");
    if (n_frames < 1 || n_frames > h->B) return fail(TSLAM_EINVAL, "n_frames must be in [1, max_batch]");
    if (h->sh_world > 1 || h->sh_comm) return fail(TSLAM_ESTATE, "a sharded handle is driven stage by stage");
    HIPCHK(hipSetDevice(h->device));
    int rc = ensure_async(h);
    if (rc != TSLAM_OK) return rc;
    const int k = (int)(h->as_batches & 1);
    const size_t bytes = (size_t)n_frames * host_frame_bytes(h);
    // the staging buffer of this parity is free once the DMA of batch s-2 out of it finished
    if (h->as_staged_armed[k]) HIPCHK(hipEventSynchronize(h->as_staged[k]));
    if (host_images != h->as_stage[k]) memcpy(h->as_stage[k], host_images, bytes);   // (tslam_host_stage: in place)
    // the device input of this parity: batch s-2's rectify read it earlier on the same stream
    HIPCHK(hipMemcpyAsync(h->as_input[k], h->as_stage[k], bytes, hipMemcpyHostToDevice, h->as_front));
    HIPCHK(hipEventRecord(h->as_staged[k], h->as_front));
    h->as_staged_armed[k] = true;
    if ((rc = tslam_begin_batch(h, h->as_input[k], n_frames)) != TSLAM_OK) return rc;
    const int stages[5] = {TSLAM_STAGE_RECTIFY, TSLAM_STAGE_DETECT, TSLAM_STAGE_DESCRIBE, TSLAM_STAGE_MATCH, TSLAM_STAGE_POSE};
    for (int i = 0; i < 5 && rc == TSLAM_OK; ++i) rc = tslam_run_stage(h, stages[i], i < 3 ? h->as_front : h->as_back);
    // results of this batch into the pinned slot of its parity, copied on the back stream right
    // after its pose stage: the next batch's back stages overwrite the pose buffers in that
    // stream's order, so the copies read this batch's records whatever the BA stream does
    if (rc == TSLAM_OK) rc = stash_results(h, timestamps, h->as_back);
    if (rc == TSLAM_OK && h->prm.ba_window) {
        // the BA stream waits for the back stream (ba_stage's event is recorded after the copies),
        // and the slot is ready once this batch's BA ran: the caller reads the window after polling
        rc = tslam_run_stage(h, TSLAM_STAGE_BA, h->as_ba);
        BA_FLUSH(h);   // the slot event below follows the BA's launches
        if (rc == TSLAM_OK) HIPCHK(hipEventRecord(h->as_res[(h->as_batches - 1) & 1].ev, h->as_ba));
    }
    const int rc2 = tslam_end_batch(h);
    return rc != TSLAM_OK ? rc : rc2;
}

static void unpack_records(const double* pose, int n, double* T_rel, double* T_abs, double* cov) {
    for (int i = 0; i < n; ++i) {
        const double* src = pose + (size_t)i * TS_POSE_DOUBLES;
        if (T_rel) memcpy(T_rel + 16 * (size_t)i, src, 16 * sizeof(double));
        if (T_abs) memcpy(T_abs + 16 * (size_t)i, src + 16, 16 * sizeof(double));
        if (cov) memcpy(cov + 36 * (size_t)i, src + 32, 36 * sizeof(double));
    }
}

int tslam_poll_batch(tslam_handle* h, int block, int max_frames, double* T_rel, double* T_abs, double* cov, int32_t* stats,
                     double* rig_T_rel, double* rig_T_abs, double* rig_cov, int32_t* rig_stats, double* ts,
                     int64_t* first_frame, int* n_frames) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    HIPCHK(hipSetDevice(h->device));
    // the oldest unread batch
    int k = -1;
    for (int i = 0; i < 2; ++i)
        if (h->as_res[i].pending && (k < 0 || h->as_res[i].batch < h->as_res[k].batch)) k = i;
    if (k < 0) return 0;
    auto& r = h->as_res[k];
    if (block) {
        HIPCHK(hipEventSynchronize(r.ev));
    } else {
        const hipError_t q = hipEventQuery(r.ev);
        if (q == hipErrorNotReady) return 0;
        if (q != hipSuccess) return fail(TSLAM_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
    }
    if (max_frames < r.n) return fail(TSLAM_EINVAL, "output capacity (max_frames) is smaller than the batch");
    const int np = r.n * h->P;
    unpack_records(r.pose, np, T_rel, T_abs, cov);
    if (stats) memcpy(stats, r.stats, sizeof(int32_t) * TS_STATS_INTS * np);
    if (h->rig) {
        unpack_records(r.rig_pose, r.n, rig_T_rel, rig_T_abs, rig_cov);
        if (rig_stats) memcpy(rig_stats, r.rig_stats, sizeof(int32_t) * TS_STATS_INTS * r.n);
    }
    if (ts) memcpy(ts, r.ts.data(), sizeof(double) * r.n);
    if (first_frame) *first_frame = r.g0;
    if (n_frames) *n_frames = r.n;
    r.pending = false;
    return 1;
}

int tslam_poll_pose(tslam_handle* h, double* T, double* cov, double* ts, int32_t* state, float* conf) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    HIPCHK(hipSetDevice(h->device));
    int k = -1;   // the newest completed batch
    for (int i = 0; i < 2; ++i) {
        const auto& r = h->as_res[i];
        if (r.batch < 0 || r.batch <= h->as_last_pose_batch || (k >= 0 && r.batch < h->as_res[k].batch)) continue;
        const hipError_t q = hipEventQuery(r.ev);
        if (q == hipErrorNotReady) continue;
        if (q != hipSuccess) return fail(TSLAM_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(q));
        k = i;
    }
    if (k < 0) return 0;
    const auto& r = h->as_res[k];
    const int f = r.n - 1;
    const double* rec = h->rig ? r.rig_pose + (size_t)f * TS_POSE_DOUBLES : r.pose + (size_t)f * h->P * TS_POSE_DOUBLES;
    const int32_t* st = h->rig ? r.rig_stats + (size_t)f * TS_STATS_INTS : r.stats + (size_t)f * h->P * TS_STATS_INTS;
    if (T) memcpy(T, rec + 16, 16 * sizeof(double));
    if (cov) memcpy(cov, rec + 32, 36 * sizeof(double));
    if (ts) *ts = r.ts[f];
    if (state) *state = st[0];
    if (conf) {   // isaac_ros.py:312: clamp(1 / (1 + trace(cov[:3, :3])), 0, 1); 1 when not tracked
        const double tr = rec[32] + rec[32 + 7] + rec[32 + 14];
        *conf = st[0] == TSLAM_POSE_OK ? (float)std::min(1.0, std::max(0.0, 1.0 / (1.0 + tr))) : 1.0f;
    }
    h->as_last_pose_batch = r.batch;
    return 1;
}

int64_t tslam_frames_done(tslam_handle* h) { return h ? h->frames_done : -1; }

int tslam_begin_batch(tslam_handle* h, const uint8_t* images, int n_frames) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!images) return fail(TSLAM_EINVAL, "null images");
    if (n_frames < 1 || n_frames > h->B) return fail(TSLAM_EINVAL, "n_frames must be in [1, max_batch]");
    if (h->in_batch) return fail(TSLAM_ESTATE, "previous batch not ended");
    h->cur_images = images;
    h->cur_n = n_frames;
    h->cur_g0 = h->frames_done;
    h->in_batch = true;
    h->batch_started = false;
    h->front_started = h->back_started = false;
    h->front_stream = h->back_stream = nullptr;
    return TSLAM_OK;
}

int tslam_end_batch(tslam_handle* h) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "no batch in progress");
    h->frames_done += h->cur_n;
    h->in_batch = false;
    if (h->prior_armed) {   // the prior slot of this parity is free once this batch's last stage ran
        const int par = (int)(h->batch_idx & 1);
        if (!h->ev_prior[par]) HIPCHK(hipEventCreateWithFlags(&h->ev_prior[par], hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->ev_prior[par], h->last_stream));
        h->prior_read_armed[par] = true;
    }
    h->prior_armed = false;   // a prior applies to one batch
    h->prior_copy_pending = false;
    if (h->back_started && h->front_started && h->back_stream != h->front_stream) {
        const int par = (int)(h->batch_idx & 1);
        HIPCHK(hipEventRecord(h->ev_back[par], h->back_stream));
        h->back_pending[par] = true;
    }
    h->batch_idx += 1;
    return TSLAM_OK;
}

int tslam_run_stage(tslam_handle* h, int stage, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "tslam_begin_batch first");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const bool front = stage == TSLAM_STAGE_ALL || stage == TSLAM_STAGE_RECTIFY || stage == TSLAM_STAGE_DETECT ||
                       stage == TSLAM_STAGE_DESCRIBE || (stage >= TSLAM_KERNEL_RECTIFY_PYRAMID && stage <= TSLAM_KERNEL_DESCRIBE);
    const bool back = stage == TSLAM_STAGE_ALL || stage == TSLAM_STAGE_MATCH || stage == TSLAM_STAGE_POSE ||
                      (stage >= TSLAM_KERNEL_MATCH && stage <= TSLAM_KERNEL_POSE_SOLVE);
    if (!h->ev_front) {
        HIPCHK(hipEventCreateWithFlags(&h->ev_front, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_back[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&h->ev_back[1], hipEventDisableTiming));
    }
    const int par = (int)(h->batch_idx & 1);
    if (back && !h->back_started) BA_FLUSH(h);   // a deferred BA of the previous batch: now, behind this batch's front
    if (stage != TSLAM_STAGE_BA && !h->batch_started) {
        if (h->ba_job.pending && h->ba_job.par == par) ba_flush(h);   // (that BA's event is recorded before this wait)
        // the first work of a batch: the BA of the batch two back (same ring slots) must be done
        if (h->ba_pending[par]) HIPCHK(hipStreamWaitEvent(s, h->ev_ba[par], 0));
        h->ba_pending[par] = false;
        h->batch_started = true;
    }
    if (front && !h->front_started) {
        // ... and so must the back stages of the batch two back (they read the frames whose ring
        // slots this batch's front stages overwrite)
        if (h->back_pending[par]) HIPCHK(hipStreamWaitEvent(s, h->ev_back[par], 0));
        h->back_pending[par] = false;
        h->front_started = true;
        h->front_stream = s;
    }
    if (back && !h->back_started) {
        if (h->front_started && h->front_stream != s) {   // this batch's features come from the front stream
            HIPCHK(hipEventRecord(h->ev_front, h->front_stream));
            HIPCHK(hipStreamWaitEvent(s, h->ev_front, 0));
        }
        h->back_started = true;
        h->back_stream = s;
    }
    if (back && h->prior_copy_pending) {   // this batch's prior (tslam_set_motion_prior), before its pose stage
        const size_t slot = (size_t)TS_PRIOR_DOUBLES * h->P * h->B;
        HIPCHK(hipMemcpyAsync(h->d_prior + (size_t)par * slot, h->h_prior_pin[par], sizeof(double) * slot,
                              hipMemcpyHostToDevice, s));
        h->prior_copy_pending = false;
    }
    if (front && h->front_started && s != h->front_stream && !back)
        return fail(TSLAM_ESTATE, "all front stages of a batch must use one stream");
    if (back && h->back_started && s != h->back_stream && !front)
        return fail(TSLAM_ESTATE, "all back stages of a batch must use one stream");
    if (stage != TSLAM_STAGE_BA) h->last_stream = s;
    const BatchCtx c = make_ctx(h);
    if (h->sh_world > 1 || h->sh_comm) return run_sharded_stage(h, c, stage, s);
    const BackView v{&c, nullptr, &c, true, true};   // the whole batch; POSE up to the chains and the loop store
    int rc = run_front_stage(h, c, stage, s);
    if (rc == 0) rc = run_back_stage(h, c, v, stage, s);
    if (rc < 0) return rc;
    if (rc == 0) {   // neither: the whole pipeline, the BA stage, the solver on injected correspondences
        switch (stage) {
            case TSLAM_STAGE_ALL:
                for (int st : {TSLAM_STAGE_RECTIFY, TSLAM_STAGE_DETECT, TSLAM_STAGE_DESCRIBE}) run_front_stage(h, c, st, s);
                for (int st : {TSLAM_STAGE_MATCH, TSLAM_STAGE_POSE}) run_back_stage(h, c, v, st, s);
                if (h->prm.ba_window && (rc = ba_inline(h, c, s)) != TSLAM_OK) return rc;
                break;
            case TSLAM_STAGE_BA:
                if ((rc = ba_stage(h, c, s)) != TSLAM_OK) return rc;
                break;
            case TSLAM_KERNEL_POSE_SOLVE: launch_pose_solve(c, s); break;
            default: return fail(TSLAM_EINVAL, "unknown stage");
        }
    }
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_submit(tslam_handle* h, const uint8_t* images, int n_frames, void* stream) {
    int rc = tslam_begin_batch(h, images, n_frames);
    if (rc != TSLAM_OK) return rc;
    rc = tslam_run_stage(h, TSLAM_STAGE_ALL, stream);
    const int rc2 = tslam_end_batch(h);
    return rc != TSLAM_OK ? rc : rc2;
}

int tslam_detect(tslam_handle* h, void* stream) {
    int rc = tslam_run_stage(h, TSLAM_STAGE_RECTIFY, stream);
    return rc != TSLAM_OK ? rc : tslam_run_stage(h, TSLAM_STAGE_DETECT, stream);
}
int tslam_describe(tslam_handle* h, void* stream) { return tslam_run_stage(h, TSLAM_STAGE_DESCRIBE, stream); }
int tslam_match(tslam_handle* h, void* stream) { return tslam_run_stage(h, TSLAM_STAGE_MATCH, stream); }
int tslam_pose(tslam_handle* h, void* stream) { return tslam_run_stage(h, TSLAM_STAGE_POSE, stream); }

int tslam_sync(tslam_handle* h) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

static int copy_pose_records(const double* dev_pose, const int32_t* dev_stats, int n, double* T_rel, double* T_abs,
                             double* cov, int32_t* stats) {
    std::vector<double> pose((size_t)n * TS_POSE_DOUBLES);
    HIPCHK(hipMemcpy(pose.data(), dev_pose, sizeof(double) * pose.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const double* src = pose.data() + (size_t)i * TS_POSE_DOUBLES;
        if (T_rel) memcpy(T_rel + 16 * (size_t)i, src, 16 * sizeof(double));
        if (T_abs) memcpy(T_abs + 16 * (size_t)i, src + 16, 16 * sizeof(double));
        if (cov) memcpy(cov + 36 * (size_t)i, src + 32, 36 * sizeof(double));
    }
    if (stats) HIPCHK(hipMemcpy(stats, dev_stats, sizeof(int32_t) * TS_STATS_INTS * (size_t)n, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_read_poses(tslam_handle* h, int max_frames, double* T_rel, double* T_abs, double* cov, int32_t* stats) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (h->cur_n == 0) return fail(TSLAM_ESTATE, "no batch has run since tslam_create / tslam_reset");
    if (max_frames < h->cur_n) return fail(TSLAM_EINVAL, "output capacity (max_frames) is smaller than the last batch");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    return copy_pose_records((const double*)h->buf[TSLAM_BUF_POSE].ptr, (const int32_t*)h->buf[TSLAM_BUF_STATS].ptr,
                             h->cur_n * h->P, T_rel, T_abs, cov, stats);
}

int tslam_select_mode(tslam_handle* h, int mode, int resident_cap) {
    if (!h || mode < 0 || mode > 2 || resident_cap < 0) return fail(TSLAM_EINVAL, "bad handle, select mode or capacity");
    h->sel_mode = mode;
    h->sel_rcap = resident_cap;
    return TSLAM_OK;
}

int tslam_match_mode(tslam_handle* h, int mode, int merge_cap) {
    if (!h || mode < 0 || mode > 2 || merge_cap < 0) return fail(TSLAM_EINVAL, "bad handle, match mode or capacity");
    h->match_mode = mode;
    h->match_cap = merge_cap;
    return TSLAM_OK;
}

int tslam_match_layout(tslam_handle* h, int layout) {
    if (!h || layout < 0 || layout > 1) return fail(TSLAM_EINVAL, "bad handle or match layout");
    h->match_split = layout;
    return TSLAM_OK;
}

int tslam_describe_mode(tslam_handle* h, int list_cap) {
    if (!h || list_cap < 0) return fail(TSLAM_EINVAL, "bad handle or list capacity");
    h->dt_list_cap = list_cap;
    return TSLAM_OK;
}

int tslam_match_counters(tslam_handle* h, uint32_t* counters16, int* blocks_per_cu) {
    if (!h) return fail(TSLAM_EINVAL, "bad handle");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    if (!h->d_match_cnt) {
        if ((rc = dev_alloc(h, (void**)&h->d_match_cnt, sizeof(uint32_t) * 16)) != TSLAM_OK) return rc;
    }
    if (counters16) HIPCHK(hipMemcpy(counters16, h->d_match_cnt, sizeof(uint32_t) * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->d_match_cnt, 0, sizeof(uint32_t) * 16));
    HIPCHK(hipDeviceSynchronize());
    if (blocks_per_cu) *blocks_per_cu = match_blocks_per_cu();
    return TSLAM_OK;
}

int tslam_detect_counters(tslam_handle* h, uint32_t* counters, int max_levels) {
    if (!h || max_levels < 0) return fail(TSLAM_EINVAL, "bad handle or level count");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    const size_t bytes = sizeof(uint32_t) * TS_MAX_LEVELS * TS_DCNT;
    if (!h->d_det_cnt) {
        if ((rc = dev_alloc(h, (void**)&h->d_det_cnt, bytes)) != TSLAM_OK) return rc;
    }
    const int nl = std::min(max_levels, (int)TS_MAX_LEVELS);
    if (counters && nl > 0)
        HIPCHK(hipMemcpy(counters, h->d_det_cnt, sizeof(uint32_t) * TS_DCNT * (size_t)nl, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->d_det_cnt, 0, bytes));
    HIPCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

int tslam_buffer_info(tslam_handle* h, int which, void** device_ptr, int64_t* bytes_total, int64_t* bytes_per_frame) {
    if (!h || which < 0 || which >= TSLAM_BUF_COUNT) return fail(TSLAM_EINVAL, "bad handle or buffer id");
    BA_FLUSH(h);
    if (device_ptr) *device_ptr = h->buf[which].ptr;
    if (bytes_total) *bytes_total = h->buf[which].bytes;
    if (bytes_per_frame) *bytes_per_frame = h->buf[which].per_frame;
    return TSLAM_OK;
}

int tslam_copy_out(tslam_handle* h, int which, int64_t offset, void* host_dst, int64_t bytes) {
    if (!h || which < 0 || which >= TSLAM_BUF_COUNT || !host_dst) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (offset < 0 || bytes < 0 || offset + bytes > h->buf[which].bytes) return fail(TSLAM_EINVAL, "range outside buffer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(host_dst, (const char*)h->buf[which].ptr + offset, (size_t)bytes, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_copy_in(tslam_handle* h, int which, int64_t offset, const void* host_src, int64_t bytes) {
    if (!h || which < 0 || which >= TSLAM_BUF_COUNT || !host_src) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (offset < 0 || bytes < 0 || offset + bytes > h->buf[which].bytes) return fail(TSLAM_EINVAL, "range outside buffer");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy((char*)h->buf[which].ptr + offset, host_src, (size_t)bytes, hipMemcpyHostToDevice));
    return TSLAM_OK;
}

int tslam_ring_slot(tslam_handle* h, int64_t global_frame) {
    if (!h || global_frame < 0) return fail(TSLAM_EINVAL, "bad argument");
    return (int)(global_frame % h->R);
}

int tslam_layout(tslam_handle* h, int64_t* out16, int32_t* level_info18) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (out16) {
        for (int i = 0; i < 16; ++i) out16[i] = 0;
        out16[0] = h->W;
        out16[1] = h->H;
        out16[2] = h->g.n_levels;
        out16[3] = h->g.K;
        out16[4] = h->R;
        out16[5] = h->B;
        out16[6] = h->P;
        out16[7] = h->g.pyr_bytes;
        for (int l = 0; l < h->g.n_levels; ++l) out16[8 + l] = h->g.pyr_off[l];
    }
    if (level_info18) {
        for (int i = 0; i < 18; ++i) level_info18[i] = 0;
        for (int l = 0; l < h->g.n_levels; ++l) {
            level_info18[3 * l] = h->g.W[l];
            level_info18[3 * l + 1] = h->g.H[l];
            level_info18[3 * l + 2] = h->g.Kq[l];
        }
    }
    return TSLAM_OK;
}

int tslam_set_motion_prior(tslam_handle* h, const double* prior, int n_frames) {
    if (!h || !prior) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_set_motion_prior inside a batch");
    if (n_frames < 1 || n_frames > h->B) return fail(TSLAM_EINVAL, "n_frames must be in [1, max_batch]");
    HIPCHK(hipSetDevice(h->device));
    const size_t slot = (size_t)TS_PRIOR_DOUBLES * h->P * h->B;
    if (!h->d_prior) {   // one slot per batch parity: batch s-1 may still be reading its prior
        const int rc = dev_alloc(h, (void**)&h->d_prior, sizeof(double) * 2 * slot);
        if (rc != TSLAM_OK) return rc;
    }
    if (h->rig && !h->d_rig_prior) {
        const int rc = dev_alloc(h, (void**)&h->d_rig_prior, sizeof(double) * 2 * TS_PRIOR_DOUBLES * h->B);
        if (rc != TSLAM_OK) return rc;
    }
    // the slot's previous reader is batch s-2 (pose + chain stages): wait for the event its last
    // stage recorded, not for the whole device
    const int par = (int)(h->batch_idx & 1);
    if (h->prior_read_armed[par]) {
        HIPCHK(hipEventSynchronize(h->ev_prior[par]));
        h->prior_read_armed[par] = false;
    }
    if (!h->h_prior_pin[par]) {
        HIPCHK(hipHostMalloc((void**)&h->h_prior_pin[par], sizeof(double) * slot, hipHostMallocDefault));
        h->host_allocs.push_back(h->h_prior_pin[par]);
    }
    // pinned staging (its previous DMA, batch s-2's, is covered by the event above); the copy is
    // enqueued on the batch's own back stream, so no host wait and no null-stream ordering
    const size_t nb = (size_t)TS_PRIOR_DOUBLES * h->P * n_frames;
    memcpy(h->h_prior_pin[par], prior, sizeof(double) * nb);
    std::fill(h->h_prior_pin[par] + nb, h->h_prior_pin[par] + slot, 0.0);   // frames past n: weight 0
    h->prior_armed = true;
    h->prior_copy_pending = true;
    return TSLAM_OK;
}

static int set_rig_E(tslam_handle* h, int q_total, const double* base_T_rect) {
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> e(32 * (size_t)q_total, 0.0);
    for (int q = 0; q < q_total; ++q) {
        const double* E = base_T_rect + 16 * q;
        double* inv = e.data() + 16 * (q_total + q);
        for (int i = 0; i < 16; ++i) e[16 * q + i] = E[i];
        if (E[12] != 0.0 || E[13] != 0.0 || E[14] != 0.0 || E[15] != 1.0) return fail(TSLAM_EINVAL, "base_T_rect must be rigid 4x4");
        for (int i = 0; i < 3; ++i) {   // [R^T | -R^T t]
            for (int j = 0; j < 3; ++j) inv[4 * i + j] = E[4 * j + i];
            inv[4 * i + 3] = -((E[i] * E[3] + E[4 + i] * E[7]) + E[8 + i] * E[11]);
        }
        inv[15] = 1.0;
    }
    if (q_total > h->rig_cap) {
        const int rc = dev_grow(h, (void**)&h->d_rig_E, sizeof(double) * 32 * q_total);
        if (rc != TSLAM_OK) return rc;
        h->rig_cap = q_total;
    }
    if (!h->d_rig_pose) {
        int rc = dev_alloc(h, (void**)&h->d_rig_pose, sizeof(double) * TS_POSE_DOUBLES * h->B);
        if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_rig_stats, sizeof(int32_t) * TS_STATS_INTS * h->B);
        if (rc == TSLAM_OK) rc = dev_alloc(h, (void**)&h->d_rig_state, sizeof(double) * 32);   // chain (A, Q)
        if (rc != TSLAM_OK) return rc;
        const double eye[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        HIPCHK(hipMemcpy(h->d_rig_state, eye, sizeof(eye), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(h->d_rig_E, e.data(), sizeof(double) * e.size(), hipMemcpyHostToDevice));
    h->rig_q = q_total;
    return TSLAM_OK;
}

int tslam_set_rig(tslam_handle* h, const double* base_T_rect) {
    if (!h || !base_T_rect) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_set_rig inside a batch");
    const int rc = set_rig_E(h, h->P, base_T_rect);
    if (rc != TSLAM_OK) return rc;
    h->rig = true;
    return TSLAM_OK;
}

int tslam_read_rig_poses(tslam_handle* h, int max_frames, double* T_rel, double* T_abs, double* cov, int32_t* stats) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (!h->rig) return fail(TSLAM_ESTATE, "no rig set (tslam_set_rig)");
    if (h->cur_n == 0) return fail(TSLAM_ESTATE, "no batch has run since tslam_create / tslam_reset");
    if (max_frames < h->cur_n) return fail(TSLAM_EINVAL, "output capacity (max_frames) is smaller than the last batch");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    return copy_pose_records(h->d_rig_pose, h->d_rig_stats, h->cur_n, T_rel, T_abs, cov, stats);
}

int tslam_internal_stash(tslam_handle* h, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "results are stashed inside a batch (before tslam_end_batch)");
    HIPCHK(hipSetDevice(h->device));
    return stash_results(h, nullptr, (hipStream_t)stream);
}

}  // extern "C"
