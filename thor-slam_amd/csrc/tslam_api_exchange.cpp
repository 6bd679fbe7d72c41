// tslam_api_exchange.cpp — the sharded rig on the host side: a rank's frame ranges, the stage
// views of a sharded handle, tslam_set_shard and the pack / unpack / import entry points of
// streams, pairs, peers, the partner camera and pose records (the driver is tslam_shard.cpp).
#include "tslam_handle.h"

// The back-end context of batch frames [lo, hi): frame lo is the context's frame 0 and every
// batch-indexed buffer is offset to batch frame lo, so results land where a whole-batch run puts
// them (ring-indexed buffers need no offset: they are addressed by global frame).
static BatchCtx range_ctx(const BatchCtx& c, int lo, int hi) {
    BatchCtx r = c;
    const size_t P = c.P, K = c.g.K, f = lo;
    ctx_set_first_frame(r, c.g0 + lo);
    r.n = hi - lo;
    r.qbest += f * P * 2 * K;
    r.qsecond += f * P * 2 * K;
    r.tbest += f * P * 2 * K;
    r.qtpos += f * P * 2 * K;
    r.tuv += f * P * K * 2;
    r.corr += f * P * K * TS_CORR_DOUBLES;
    r.pose += f * P * TS_POSE_DOUBLES;
    r.stats += f * P * TS_STATS_INTS;
    r.ransac += f * P * TS_MAX_SPLITS * TS_RANSAC_WORDS / 2;
    r.hyp += f * P * 4 * (size_t)c.pp.n_hyp * TS_HYP_DOUBLES;
    if (r.prior) r.prior += f * P * TS_PRIOR_DOUBLES;
    if (r.rig_prior) r.rig_prior += f * TS_PRIOR_DOUBLES;
    if (r.rig_pose) r.rig_pose += f * TS_POSE_DOUBLES;
    if (r.rig_stats) r.rig_stats += f * TS_STATS_INTS;
    return r;
}

// the rank's rig range: rig pose, pose records (and, without the pair split, its whole back end)
static void shard_range(const tslam_handle* h, int n, int* lo, int* hi) {
    peer_range(rig_slot(h->sh_rank, h->sh_world, h->sh_pairs), n, h->sh_world, lo, hi);
}
// pair split: the half of the batch whose frames this rank's pair back end solves
static void pair_half(const tslam_handle* h, int n, int* lo, int* hi) { peer_range(h->sh_cam_lo & 1, n, 2, lo, hi); }

// Stages of a sharded handle (tslam_set_shard, world > 1).  Front stages run on the handle's
// cameras for every frame of the batch; back stages on the rank's frame range [lo, hi) of the
// batch, after the exchange has filled the other cameras' ring slots for frames lo-1 .. hi-1:
// MATCH first re-derives the stereo disparities of frame lo-1 (the range's first frame
// triangulates from them; the rank that owns lo-1 computes the same values), POSE adds the rig
// pose of the range (no chaining), and CHAIN chains the whole batch once every rank's pose
// records are back (tslam_unpack_poses), identically on every rank.
//
// A camera-sharded RGB-D rig (each camera is a "pair": its back end needs no other camera) instead
// tracks its own cameras over the whole batch: MATCH and POSE run on the pair view of its cameras
// for every frame; the rig pose of its frame range (KERNEL_RIG) follows tslam_unpack_pairs of the
// other ranks' pair blocks (pose, stats, correspondences); then pose records and CHAIN as above.
static int run_sharded_rgbd_stage(tslam_handle* h, const BatchCtx& c, int stage, hipStream_t s) {
    int lo, hi;
    shard_range(h, c.n, &lo, &hi);
    BatchCtx own = c;   // pair view: this rank's cameras (cameras per pair = 1)
    ctx_set_views(own, own.cam0, own.ncam, h->sh_cam_lo, h->sh_cam_hi - h->sh_cam_lo);
    const BatchCtx cr = range_ctx(c, lo, hi);
    const BackView v{&own, nullptr, hi > lo ? &cr : nullptr, false, false};
    int rc = run_front_stage(h, c, stage, s);
    if (rc == 0) rc = run_back_stage(h, c, v, stage, s);
    if (rc < 0) return rc;
    if (rc == 0)
        return fail(TSLAM_ESTATE, "a camera-sharded RGB-D handle runs its stages one by one: RECTIFY..DESCRIBE, "
                                  "MATCH, POSE, pack/exchange/unpack pairs, KERNEL_RIG, pose records, CHAIN");
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int run_sharded_stage(tslam_handle* h, const BatchCtx& c, int stage, hipStream_t s) {
    if (h->prm.rgbd) return run_sharded_rgbd_stage(h, c, stage, s);
    int lo, hi;
    if (h->sh_pairs) pair_half(h, c.n, &lo, &hi);
    else shard_range(h, c.n, &lo, &hi);
    BatchCtx cb = range_ctx(c, lo, hi);
    const bool empty = hi <= lo;           // a short batch leaves this rank no frames
    const bool pre = !empty && c.g0 + lo - 1 >= 0;   // frame lo - 1 exists
    BatchCtx cp = c;                        // the pre-pass: frame lo - 1, batch scratch at frame 0
    ctx_set_first_frame(cp, c.g0 + lo - 1);
    cp.n = 1;
    BatchCtx cr = c;                        // pair split: the rig range
    BackView v{empty ? nullptr : &cb, pre ? &cp : nullptr, empty ? nullptr : &cb, true, false};   // POSE adds the rig pose
    if (h->sh_pairs) {   // pair split: this camera's pair only; the rig pose is its own step (KERNEL_RIG)
        ctx_set_views(cb, cb.cam0, cb.ncam, h->sh_cam_lo / 2, 1);
        ctx_set_views(cp, cp.cam0, cp.ncam, h->sh_cam_lo / 2, 1);
        int rl, rh;
        shard_range(h, c.n, &rl, &rh);   // every pair's blocks of the rig range are here (tslam_shard.cpp)
        cr = range_ctx(c, rl, rh);
        v.rig = rh > rl ? &cr : nullptr;
        v.pose_rig = false;
    }
    int rc = run_front_stage(h, c, stage, s);
    if (rc == 0) rc = run_back_stage(h, c, v, stage, s);
    if (rc < 0) return rc;
    if (rc == 0) {
        if (stage == TSLAM_STAGE_BA) return ba_stage(h, c, s);   // rank 0 of a gathering driver
        return fail(TSLAM_ESTATE, "a sharded handle runs its stages one by one around the exchange "
                                  "(RECTIFY..DESCRIBE, pack/exchange/unpack, MATCH, POSE, exchange, CHAIN)");
    }
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

extern "C" {

// -- sharded rig ------------------------------------------------------------------
int tslam_set_shard(tslam_handle* h, int cam_lo, int cam_hi, int rank, int world) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (h->in_batch) return fail(TSLAM_ESTATE, "tslam_set_shard inside a batch");
    if (cam_lo < 0 || cam_hi > h->C || cam_lo >= cam_hi) return fail(TSLAM_EINVAL, "camera range outside [0, cameras)");
    if (world < 1 || rank < 0 || rank >= world || world > h->B) return fail(TSLAM_EINVAL, "need 0 <= rank < world <= max_batch");
    if (world > 1 && h->prm.ba_window && h->prm.rgbd)
        return fail(TSLAM_EINVAL, "a camera-sharded RGB-D rig runs without local BA");
    h->sh_cam_lo = cam_lo;
    h->sh_cam_hi = cam_hi;
    h->sh_rank = rank;
    h->sh_world = world;
    h->sh_pairs = false;   // the driver sets the pair split after (tslam_shard_options)
    return TSLAM_OK;
}

int tslam_exchange_sizes(tslam_handle* h, int64_t* stream_block, int64_t* pose_record) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (stream_block) *stream_block = stream_block_bytes(h->g);
    if (pose_record) *pose_record = pose_record_bytes(h->P);
    return TSLAM_OK;
}

static int check_frames_cams(tslam_handle* h, int64_t first_frame, int n_frames, int cam_lo, int cam_hi) {
    if (n_frames < 1 || n_frames > h->R) return fail(TSLAM_EINVAL, "n_frames must be in [1, ring]");
    if (cam_lo < 0 || cam_hi > h->C || cam_lo >= cam_hi) return fail(TSLAM_EINVAL, "camera range outside [0, cameras)");
    if (first_frame + n_frames < 0) return fail(TSLAM_EINVAL, "frame range before the sequence start");
    return TSLAM_OK;
}

int tslam_pack_streams(tslam_handle* h, int64_t first_frame, int n_frames, int cam_lo, int cam_hi, void* dst, void* stream) {
    if (!h || !dst) return fail(TSLAM_EINVAL, "bad argument");
    int rc = check_frames_cams(h, first_frame, n_frames, cam_lo, cam_hi);
    if (rc != TSLAM_OK) return rc;
    HIPCHK(hipSetDevice(h->device));
    launch_stream_blocks(make_ctx(h), true, first_frame, n_frames, cam_lo, cam_hi - cam_lo, (uint8_t*)dst, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_unpack_streams(tslam_handle* h, int64_t first_frame, int n_frames, int cam_lo, int cam_hi, const void* src,
                         void* stream) {
    if (!h || !src) return fail(TSLAM_EINVAL, "bad argument");
    int rc = check_frames_cams(h, first_frame, n_frames, cam_lo, cam_hi);
    if (rc != TSLAM_OK) return rc;
    HIPCHK(hipSetDevice(h->device));
    launch_stream_blocks(make_ctx(h), false, first_frame, n_frames, cam_lo, cam_hi - cam_lo, (uint8_t*)src, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_import_raw(tslam_handle* h, const uint8_t* images, int64_t first_frame, int n_frames, int cam_lo, int cam_hi,
                     void* stream) {
    if (!h || !images) return fail(TSLAM_EINVAL, "bad argument");
    int rc = check_frames_cams(h, first_frame, n_frames, cam_lo, cam_hi);
    if (rc != TSLAM_OK) return rc;
    if (h->prm.rgbd) return fail(TSLAM_EINVAL, "tslam_import_raw takes gray stereo images");
    HIPCHK(hipSetDevice(h->device));
    BatchCtx c = make_ctx(h);
    const int ncam = cam_hi - cam_lo;
    const int64_t skip = first_frame < 0 ? -first_frame : 0;   // frames before the sequence start
    c.images = images + (size_t)skip * ncam * h->W * h->H;
    ctx_set_first_frame(c, first_frame + skip);
    c.n = (int)(n_frames - skip);
    ctx_set_views(c, cam_lo, ncam, c.pair0, c.npair);
    launch_rectify_pyramid(c, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_pair_block_bytes(tslam_handle* h, int64_t* bytes) {
    if (!h || !bytes) return fail(TSLAM_EINVAL, "bad argument");
    *bytes = pair_block_bytes(h->g);
    return TSLAM_OK;
}

static int pair_blocks(tslam_handle* h, bool pack, int f0, int n_frames, int pair_lo, int pair_hi, uint8_t* buf, void* stream) {
    if (!h || !buf) return fail(TSLAM_EINVAL, "bad argument");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "pair blocks are packed / unpacked inside a batch");
    if (f0 < 0 || n_frames < 1 || f0 + n_frames > h->cur_n) return fail(TSLAM_EINVAL, "frame range outside the batch");
    if (pair_lo < 0 || pair_hi > h->P || pair_lo >= pair_hi) return fail(TSLAM_EINVAL, "pair range outside [0, pairs)");
    HIPCHK(hipSetDevice(h->device));
    launch_pair_blocks(make_ctx(h), pack, f0, n_frames, pair_lo, pair_hi - pair_lo, buf, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_pack_pairs(tslam_handle* h, int f0, int n_frames, int pair_lo, int pair_hi, void* dst, void* stream) {
    return pair_blocks(h, true, f0, n_frames, pair_lo, pair_hi, (uint8_t*)dst, stream);
}

int tslam_unpack_pairs(tslam_handle* h, int f0, int n_frames, int pair_lo, int pair_hi, const void* src, void* stream) {
    return pair_blocks(h, false, f0, n_frames, pair_lo, pair_hi, (uint8_t*)src, stream);
}

int tslam_internal_info(tslam_handle* h, tslam_handle_info* o) {
    if (!h || !o) return fail(TSLAM_EINVAL, "bad argument");
    o->device = h->device;
    o->W = h->W;
    o->H = h->H;
    o->P = h->P;
    o->C = h->C;
    o->B = h->B;
    o->rgbd = h->prm.rgbd;
    o->rig = h->rig ? 1 : 0;
    o->ba = h->prm.ba_window;
    o->frames_done = h->frames_done;
    o->stream_block = stream_block_bytes(h->g);
    o->pose_record = pose_record_bytes(h->P);
    o->pair_block = pair_block_bytes(h->g);
    o->state_range = state_range_block_bytes(h->g);
    o->state_camera = state_camera_block_bytes(h->g);
    o->cam_lo = h->sh_cam_lo;
    o->cam_hi = h->sh_cam_hi;
    o->rank = h->sh_rank;
    o->world = h->sh_world;
    return TSLAM_OK;
}

int tslam_internal_attach_driver(tslam_handle* h, tslam_shard_driver* d, bool owned) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (h->drv && h->drv_owned && h->drv != d) tslam_internal_driver_destroy(h->drv);
    h->drv = d;
    h->drv_owned = d && owned;
    h->sh_comm = d != nullptr;
    return TSLAM_OK;
}

tslam_shard_driver* tslam_internal_driver(tslam_handle* h) { return h ? h->drv : nullptr; }

int tslam_internal_state_blocks(tslam_handle* h, int pack, int rank, int cam_lo, int cam_hi, void* buf, void* stream) {
    if (!h || !buf) return fail(TSLAM_EINVAL, "bad argument");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "state blocks are packed / unpacked inside a batch");
    if (h->prm.rgbd) return fail(TSLAM_ESTATE, "state blocks describe a stereo rig");
    HIPCHK(hipSetDevice(h->device));
    launch_state_blocks(make_ctx(h), pack != 0, h->cur_n, h->sh_world, rank, cam_lo, cam_hi, (uint8_t*)buf,
                        (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_perturb_temporal(tslam_handle* h, int percent, uint64_t seed, void* stream) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (!h->in_batch) return fail(TSLAM_ESTATE, "tslam_perturb_temporal inside a batch (after MATCH_REFINE)");
    if (percent < 0 || percent > 100) return fail(TSLAM_EINVAL, "percent must be in [0, 100]");
    if (h->sh_world > 1 || h->sh_comm) return fail(TSLAM_ESTATE, "tslam_perturb_temporal takes an unsharded handle");
    HIPCHK(hipSetDevice(h->device));
    if (percent > 0) launch_perturb_uv(make_ctx(h), percent, seed, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

// -- the all-to-all's peers in one launch each (alltoall layout [world][nr][S]) -------------------
static int check_peers(tslam_handle* h) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "peer exchange blocks are packed / imported inside a batch");
    if (h->sh_world < 2 || h->prm.rgbd) return fail(TSLAM_ESTATE, "a stereo handle sharded over world > 1");
    if ((h->sh_cam_hi - h->sh_cam_lo) * h->sh_world != h->C || h->sh_cam_lo != h->sh_rank * (h->sh_cam_hi - h->sh_cam_lo))
        return fail(TSLAM_EINVAL, "peer layout needs cameras [rank*S, (rank+1)*S)");
    return TSLAM_OK;
}
// the exchange plan's geometry of the current batch (tslam_xplan.h: the frame-range slot layout)
static XGeom peers_geom(tslam_handle* h) {
    tslam_handle_info in{};
    (void)tslam_internal_info(h, &in);
    return tslam_xgeom(in, h->sh_world, h->cur_n, false, false);
}

int tslam_pack_streams_peers(tslam_handle* h, void* dst, void* stream) {
    int rc = check_peers(h);
    if (rc != TSLAM_OK) return rc;
    if (!dst) return fail(TSLAM_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(h->device));
    const XGeom g = peers_geom(h);
    launch_stream_blocks_peers(make_ctx(h), true, h->cur_g0, g.n, g.world, xp_slot_frames(g), h->sh_rank, g.S, (uint8_t*)dst,
                               (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_stage_raw_peers(tslam_handle* h, const uint8_t* prev_raw, void* dst, void* stream) {
    int rc = check_peers(h);
    if (rc != TSLAM_OK) return rc;
    if (!prev_raw || !dst) return fail(TSLAM_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(h->device));
    const XGeom g = peers_geom(h);
    launch_stage_raw_peers(h->cur_images, prev_raw, (uint8_t*)dst, g.n, g.world, xp_slot_frames(g), h->sh_rank, g.S,
                           (int64_t)g.img, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_import_peers(tslam_handle* h, const uint8_t* raw, const void* streams, void* stream) {
    int rc = check_peers(h);
    if (rc != TSLAM_OK) return rc;
    if (!raw || !streams) return fail(TSLAM_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(h->device));
    const XGeom g = peers_geom(h);
    int lo;
    const int nr = xp_back_frames(g, h->sh_rank, &lo);
    if (nr == 0) return TSLAM_OK;   // an empty frame range: this rank's back end has nothing to do
    const int64_t first = h->cur_g0 + lo - 1;
    const int skip = first < 0 ? 1 : 0;   // frame -1 (before the sequence start) is not imported
    BatchCtx c = make_ctx(h);
    c.images = raw;
    ctx_set_first_frame(c, first + skip);
    c.n = nr - skip;
    c.peer_S = g.S;
    c.peer_me = h->sh_rank;
    c.peer_nbuf = xp_slot_frames(g);
    c.peer_skip = skip;
    if (c.n > 0) launch_rectify_pyramid(c, (hipStream_t)stream);
    launch_stream_blocks_peers(make_ctx(h), false, h->cur_g0, g.n, g.world, xp_slot_frames(g), h->sh_rank, g.S,
                               (uint8_t*)streams, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

// -- pair split (TSLAM_SHARD_PAIRS): the partner camera's frames of this rank's half -------------
int tslam_internal_set_pairs(tslam_handle* h, int on) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (h->in_batch) return fail(TSLAM_ESTATE, "the pair split is set outside a batch");
    if (on) {
        if (h->prm.rgbd) return fail(TSLAM_EINVAL, "the pair split shards a stereo rig");
        if (h->sh_world < 2 || h->sh_world != h->C || h->sh_cam_hi - h->sh_cam_lo != 1 || h->sh_cam_lo != h->sh_rank)
            return fail(TSLAM_EINVAL, "the pair split needs one camera per rank (world = cameras)");
        if (h->prm.ba_window) return fail(TSLAM_EINVAL, "the pair split runs without local BA (no state gather)");
    }
    h->sh_pairs = on != 0;
    return TSLAM_OK;
}

static int check_partner(tslam_handle* h) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "partner blocks are packed / imported inside a batch");
    if (!h->sh_pairs) return fail(TSLAM_ESTATE, "the handle is not pair-split (TSLAM_SHARD_PAIRS)");
    return TSLAM_OK;
}

int tslam_internal_pack_partner(tslam_handle* h, void* dst, void* stream) {
    int rc = check_partner(h);
    if (rc != TSLAM_OK) return rc;
    if (!dst) return fail(TSLAM_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(h->device));
    int lo, hi;
    peer_range((h->sh_cam_lo & 1) ^ 1, h->cur_n, 2, &lo, &hi);   // the partner's half
    if (hi > lo)   // frames lo - 1 .. hi - 1 of this camera (zeros before the sequence start)
        launch_stream_blocks(make_ctx(h), true, h->cur_g0 + lo - 1, hi - lo + 1, h->sh_cam_lo, 1, (uint8_t*)dst,
                             (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_internal_import_partner(tslam_handle* h, const uint8_t* raw, const void* streams, void* stream) {
    int rc = check_partner(h);
    if (rc != TSLAM_OK) return rc;
    if (!raw || !streams) return fail(TSLAM_EINVAL, "null buffer");
    HIPCHK(hipSetDevice(h->device));
    int lo, hi;
    pair_half(h, h->cur_n, &lo, &hi);
    if (hi <= lo) return TSLAM_OK;   // an empty half: this rank's back end has nothing to do
    const int partner = h->sh_cam_lo ^ 1, nf = hi - lo + 1;
    const int64_t first = h->cur_g0 + lo - 1;
    const int skip = first < 0 ? 1 : 0;   // frame -1 (before the sequence start) is not imported
    BatchCtx c = make_ctx(h);
    c.images = raw + (size_t)skip * h->W * h->H;
    ctx_set_first_frame(c, first + skip);
    c.n = nf - skip;
    ctx_set_views(c, partner, 1, c.pair0, c.npair);
    if (c.n > 0) launch_rectify_pyramid(c, (hipStream_t)stream);
    launch_stream_blocks(make_ctx(h), false, first, nf, partner, 1, (uint8_t*)streams, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_pack_poses(tslam_handle* h, void* dst, void* stream) {
    if (!h || !dst) return fail(TSLAM_EINVAL, "bad argument");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "tslam_pack_poses inside a batch (after its POSE stage)");
    HIPCHK(hipSetDevice(h->device));
    int lo, hi;
    shard_range(h, h->cur_n, &lo, &hi);
    launch_pose_records(make_ctx(h), true, lo, hi - lo, (uint8_t*)dst, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

int tslam_unpack_poses(tslam_handle* h, const void* src, void* stream) {
    if (!h || !src) return fail(TSLAM_EINVAL, "bad argument");
    if (!h->in_batch) return fail(TSLAM_ESTATE, "tslam_unpack_poses inside a batch (before its CHAIN stage)");
    HIPCHK(hipSetDevice(h->device));
    // rank q's records (its rig range) start at q * peer_records(n, world) (the all-gather pads
    // every range to the longest); with equal ranges, and no pair split, that is the batch order
    launch_pose_records_gathered(make_ctx(h), h->sh_world, h->sh_pairs, (const uint8_t*)src, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return TSLAM_OK;
}

}  // extern "C"
