// tslam_api_ba.cpp — local BA (A8) on the host side: the keyframe window's storage and slot
// bookkeeping, the graph cache of the keyframe chains, the deferred job, the BA stage of a batch
// and the tslam_ba_* entry points.
#include <algorithm>
#include <cmath>
#include <limits>

#include "tslam_handle.h"

// clear() of the two factor maps (ba_imu, ba_ine) out of line, as one translation unit emitted it:
// the library's dynamic symbol table stays exactly as it was
template void std::map<std::pair<int, int64_t>, std::array<double, 10>>::clear();
template void std::map<std::pair<int, int64_t>, std::array<double, TS_BA_INE + 3>>::clear();

// Storage pairs of A8: the P stereo pairs plus pair P, the body window of the rig-level solve
// (tslam_ba.h); every storage pair has its own solve scratch (strides as in ba_pair).
int alloc_ba(tslam_handle* h) {
    const size_t W = h->prm.ba_window, K = h->g.K, P = h->P + 1, WK = W * K, M = TS_BA_MAXW;
    BaStore& b = h->ba;
    struct A {
        void** p;
        size_t bytes;
    } list[] = {
        {(void**)&b.T, 8 * P * W * 16},      {(void**)&b.Tfe, 8 * P * W * 16},   {(void**)&b.u, 8 * P * WK},
        {(void**)&b.v, 8 * P * WK},          {(void**)&b.d, 8 * P * WK},         {(void**)&b.lm, 4 * P * WK},
        {(void**)&b.X, 8 * P * WK * 3},      {(void**)&b.kf_desc, 32 * P * WK},  {(void**)&b.gid, 8 * P * WK},
        {(void**)&b.remap, 4 * P * K},       {(void**)&b.cnt, 4 * P * WK},
        {(void**)&b.lm_id, 4 * P * WK},      {(void**)&b.keep, P * WK},          {(void**)&b.obs_Vg, 8 * P * WK * 9},
        {(void**)&b.lmask, 4 * P * (WK / 32 + 64)}, {(void**)&b.lpre, 4 * P * (WK / 32 + 64)},
        {(void**)&b.tc_fl, P * TS_BA_TILES * 256},  {(void**)&b.tc_ids, 4 * P * TS_BA_TILES * 2048},
        {(void**)&b.cam_off, 4 * P * (W + 1)},
        {(void**)&b.counts, 4 * 4 * P},      {(void**)&b.tiles, 4 * P * 2 * TS_BA_TILES}, {(void**)&b.done, 4 * P},
        {(void**)&b.lo_o, 4 * P * WK * M},   {(void**)&b.lo_uvd, 32 * P * WK * M}, {(void**)&b.lo_W, 8 * 18 * P * WK * M},
        {(void**)&b.Xc, 8 * P * WK * 3},
        {(void**)&b.lm_L, 8 * P * WK * 6},   {(void**)&b.lm_gp, 8 * P * WK * 3}, {(void**)&b.C, 8 * P * 64 * 64},
        {(void**)&b.part, 8 * P * (size_t)TS_BA_SPLIT * TS_BA_PART}, {(void**)&b.cam_U, 8 * P * W * 27}, {(void**)&b.dc, 8 * P * W * 6},
        {(void**)&b.flops, 8},               {(void**)&b.fe_pose, 8 * 2 * (size_t)h->B * h->P * 16},
        {(void**)&b.fe_body, 8 * 2 * (size_t)h->B * 16}, {(void**)&b.imu, 8 * P * W * 10},
        {(void**)&b.kf_assoc, 4 * 2 * (size_t)h->B * h->P * K},
        {(void**)&b.ine, 8 * P * W * TS_BA_INE}, {(void**)&b.vel, 8 * P * W * 3}, {(void**)&b.bias, 8 * P * W * 6},
    };
    for (const A& a : list) {
        const int rc = dev_alloc(h, a.p, a.bytes);
        if (rc != TSLAM_OK) return rc;
    }
    // scratch kept in its between-solves state by the kernels themselves (no per-solve memsets):
    // the slot table all -1 (k_ba_insert_gate clears the rows the last solve filled), remap all
    // 0x7F7F7F7F (k_ba_insert refills it after an eviction), cnt zero (dev_alloc; k_ba_backsub
    // re-zeroes it)
    HIPCHK(hipMemset(b.lo_o, 0xFF, 4 * P * WK * M));
    HIPCHK(hipMemset(b.remap, 0x7F, 4 * P * K));
    HIPCHK(hipDeviceSynchronize());
    h->ba_icfg.assign(h->P + 1, std::array<double, 12>{});   // pair windows + a rig's body window
    h->ba_ine_slot.assign(h->P + 1, std::array<uint8_t, TS_BA_MAXW>{});
    return TSLAM_OK;
}

static BaArgs ba_args(tslam_handle* h) {
    BaArgs a{};
    a.st = h->ba;
    a.W = h->prm.ba_window;
    a.interval = h->prm.ba_kf_interval;
    a.iters = h->prm.ba_iters;
    a.nsplit = TS_BA_SPLIT;
    a.lam = h->prm.ba_lambda;
    a.outlier_px = h->prm.ba_outlier_px;
    a.prev = -1;
    return a;
}

// Occupied slots, oldest keyframe first, without `skip`.
static int ba_order(const tslam_handle* h, int skip, int* out) {
    int n = 0;
    for (int s = 0; s < h->prm.ba_window; ++s)
        if (h->ba_frame[s] >= 0 && s != skip) out[n++] = s;
    std::sort(out, out + n, [h](int a, int b) { return h->ba_frame[a] < h->ba_frame[b]; });
    return n;
}

// Rig-level A8: a handle with tslam_set_rig over several pairs solves one body window.
static bool ba_rig(const tslam_handle* h) { return h->rig && h->P > 1 && h->prm.ba_window; }

static constexpr int BA_GRAPH_MAX = 32;   // instances per chain shape (keyframes of that shape in flight)

// One pair window's keyframe chain through the graph cache (see BaGraphInst): a finished instance
// of the chain's shape is re-pointed at this keyframe's record, a new one is captured only while
// every instance still has a replay in flight (the steady state needs two or three per shape).
static hipError_t ba_chain_graph(tslam_handle* h, const BaRec& r, bool evict, bool split, bool ine, hipStream_t s) {
    const std::array<int, 6> key{evict ? 1 : 0, evict ? r.evict.n_order : 0, r.a.n_order, ine ? 1 : 0, split ? 1 : 0,
                                 r.a.iters};
    tslam_handle::BaGraphSet* set = nullptr;
    for (auto& g : h->ba_graphs)
        if (g.key == key) set = &g;
    if (!set) {
        h->ba_graphs.emplace_back();
        set = &h->ba_graphs.back();
        set->key = key;
    }
    hipError_t e = hipSuccess;
    const int n = (int)set->inst.size();
    int pick = -1;
    for (int k = 0; k < n && pick < 0; ++k) {   // round robin from the oldest replay
        const int i = (set->next + k) % n;
        tslam_handle::BaGraphInst& in = set->inst[(size_t)i];
        if (!in.armed) {
            pick = i;
        } else {
            e = hipEventQuery(in.done);
            if (e == hipSuccess) pick = i;
            else if (e != hipErrorNotReady) return e;
        }
    }
    if (pick < 0 && n == BA_GRAPH_MAX) {   // every instance busy: wait for the oldest replay
        pick = set->next % n;
        if ((e = hipEventSynchronize(set->inst[(size_t)pick].done)) != hipSuccess) return e;
    }
    if (pick < 0) {   // a new instance: capture the chain on a private stream (nothing runs), instantiate it
        tslam_handle::BaGraphInst in;
        if (dev_alloc(h, (void**)&in.d_rec, sizeof(BaRec)) != TSLAM_OK) return hipErrorOutOfMemory;
        if (!h->ba_cap_stream && (e = hipStreamCreateWithFlags(&h->ba_cap_stream, hipStreamNonBlocking)) != hipSuccess)
            return e;
        if ((e = hipStreamBeginCapture(h->ba_cap_stream, hipStreamCaptureModeThreadLocal)) != hipSuccess) return e;
        launch_ba_setrec(r, in.d_rec, h->ba_cap_stream);
        launch_ba_chain_rec(r, in.d_rec, evict, split, ine, h->ba_cap_stream);
        if ((e = hipStreamEndCapture(h->ba_cap_stream, &in.graph)) != hipSuccess) return e;
        size_t n_root = 1;
        if ((e = hipGraphGetRootNodes(in.graph, &in.setrec, &n_root)) != hipSuccess) return e;
        if (n_root != 1) return hipErrorInvalidValue;
        if ((e = hipGraphInstantiate(&in.exec, in.graph, nullptr, nullptr, 0)) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&in.done, hipEventDisableTiming)) != hipSuccess) return e;
        set->inst.push_back(in);
        pick = n;
    } else if ((e = ba_graph_set_record(set->inst[(size_t)pick].exec, set->inst[(size_t)pick].setrec, r,
                                        set->inst[(size_t)pick].d_rec)) != hipSuccess) {
        return e;
    }
    tslam_handle::BaGraphInst& in = set->inst[(size_t)pick];
    set->next = (pick + 1) % (int)set->inst.size();
    if ((e = hipGraphLaunch(in.exec, s)) != hipSuccess) return e;
    if ((e = hipEventRecord(in.done, s)) != hipSuccess) return e;
    in.armed = true;
    return hipSuccess;
}

static void ba_graphs_destroy(tslam_handle* h) {
    for (auto& g : h->ba_graphs)
        for (auto& in : g.inst) {
            if (in.exec) (void)hipGraphExecDestroy(in.exec);
            if (in.graph) (void)hipGraphDestroy(in.graph);
            if (in.done) (void)hipEventDestroy(in.done);
        }
    h->ba_graphs.clear();
    if (h->ba_cap_stream) (void)hipStreamDestroy(h->ba_cap_stream);
    h->ba_cap_stream = nullptr;
}

// Keyframe g's factors of window `pair` — IMU rotation, inertial + initial velocity — popped out of
// ba_imu / ba_ine into the insertion's arguments; zeros where none was given, and for a rig's pairs
// (`use` false: a rig's inertial factor acts on its body window).  Marks the slot's inertial flag.
static void ba_take_factors(tslam_handle* h, int pair, int64_t g, bool use, BaArgs& a) {
    auto it = h->ba_imu.find({pair, g});
    const bool rot = use && it != h->ba_imu.end();
    for (int e = 0; e < 10; ++e) a.imu[e] = rot ? it->second[e] : 0.0;
    if (it != h->ba_imu.end()) h->ba_imu.erase(it);
    auto jt = h->ba_ine.find({pair, g});
    const bool has = use && jt != h->ba_ine.end();
    for (int e = 0; e < TS_BA_INE; ++e) a.ine[e] = has ? jt->second[e] : 0.0;
    for (int e = 0; e < 3; ++e) a.vel0[e] = has ? jt->second[TS_BA_INE + e] : 0.0;
    if (jt != h->ba_ine.end()) h->ba_ine.erase(jt);
    h->ba_ine_slot[pair][a.slot] = has && a.ine[28] > 0.0;
}

// The inertial kernels when a factor links two keyframes of the window (the oldest's points out of it).
static bool ba_window_inertial(const tslam_handle* h, int pair, const BaArgs& a) {
    bool ine = false;
    for (int k = 1; k < a.n_order; ++k) ine = ine || h->ba_ine_slot[pair][a.order[k]];
    return ine;
}

// A8: every keyframe of the current batch (g % ba_kf_interval == 0) enters each pair's window,
// evicting the oldest when the window is full, and the window is solved: per pair one keyframe chain
// (eviction + solve, issued directly or replayed from a graph), or for a rig every pair's eviction and
// one joint body solve.  Host bookkeeping of the slots only; nothing synchronises.  `fe_body`: the rig
// front end's snapshot of the batch (rig-level A8).
static hipError_t run_ba(tslam_handle* h, const BatchCtx& c, hipStream_t s, const double* fe, const double* fe_body,
                         const int32_t* kf_assoc) {
    const int W = h->prm.ba_window, iv = h->prm.ba_kf_interval;
    const bool rig = ba_rig(h);
    // pair windows replay their keyframe chains from graphs (not while Schur launches are timed)
    const bool graph = h->ba_graph && !rig && !h->ba_timing.ev;
    BaTiming* timing = h->ba_timing.ev ? &h->ba_timing : nullptr;
    for (int64_t g = c.g0; g < c.g0 + c.n; ++g) {
        if (g % iv != 0 || g <= h->ba_last) continue;
        BaArgs a = ba_args(h);
        a.fe = fe;
        a.kf_assoc = kf_assoc;
        a.frame = g;
        a.slot = (int)(h->ba_nkf % W);
        int ord[TS_BA_MAXW];
        const int nocc = ba_order(h, -1, ord);
        a.prev = nocc ? ord[nocc - 1] : -1;
        const bool evict = h->ba_frame[a.slot] >= 0;
        if (rig) {   // the body pose first, every pair's camera E_p^-1 B (and the body's inertial factor)
            a.fe_body = fe_body;
            a.pose_given = 1;
            ba_take_factors(h, h->P, g, true, a);
            launch_ba_rig_keyframe(c, a, s);
        }
        // the keyframe's record: the eviction's arguments (the remaining slots) from before the slot
        // bookkeeping moves, the solve's from after it
        BaRec r{c, a, a};
        if (evict) r.evict.n_order = ba_order(h, a.slot, r.evict.order);
        h->ba_frame[a.slot] = g;
        h->ba_nkf += 1;
        h->ba_last = g;
        r.a.n_order = ba_order(h, -1, r.a.order);
        h->ba_solved.resize(h->P);
        for (int p = 0; p < h->P; ++p) {
            r.evict.pair = r.a.pair = p;
            ba_take_factors(h, p, g, !rig, r.a);   // inserted by the solve's first launch (k_ba_insert_gate)
            if (!graph) launch_ba_keyframe(c, r.evict, evict, s);   // the eviction, by value
            if (rig) continue;   // every pair's eviction ahead of the joint solve
            for (int e = 0; e < 12; ++e) r.a.icfg[e] = h->ba_icfg[p][e];
            const bool ine = ba_window_inertial(h, p, r.a);
            if (!graph) launch_ba_solve(c, r.a, s, timing, h->ba_split, ine);
            else if (const hipError_t e = ba_chain_graph(h, r, evict, h->ba_split, ine, s); e != hipSuccess) return e;
            h->ba_solved[p] = r.a;
        }
        for (auto it = h->ba_imu.begin(); it != h->ba_imu.end();)   // factors of frames already past
            it = it->first.second < g ? h->ba_imu.erase(it) : std::next(it);
        for (auto it = h->ba_ine.begin(); it != h->ba_ine.end();)
            it = it->first.second < g ? h->ba_ine.erase(it) : std::next(it);
        if (rig) {
            for (int e = 0; e < 12; ++e) r.a.icfg[e] = h->ba_icfg[h->P][e];
            launch_ba_rig_solve(c, r.a, s, timing, ba_window_inertial(h, h->P, r.a));
            for (int p = 0; p < h->P; ++p) {
                h->ba_solved[p] = r.a;
                h->ba_solved[p].pair = p;
            }
        }
    }
    return hipSuccess;
}

// The deferred BA job (tslam_ba_defer): its stream already waits for its batch's back end, so
// issuing it later only moves the host work.
int ba_flush(tslam_handle* h) {
    if (!h->ba_job.pending) return TSLAM_OK;
    h->ba_job.pending = false;
    auto& j = h->ba_job;
    HIPCHK(hipSetDevice(h->device));   // flushed from any entry point, before it sets the device
    hipError_t e = run_ba(h, j.c, j.s, j.snap, j.snap_body, j.assoc);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(h->ev_ba[j.par], j.s);
    if (e != hipSuccess) {   // no event to wait for: the window's state is unknown, say so now
        h->ba_pending[j.par] = false;
        return fail(TSLAM_EHIP, std::string("deferred BA: ") + hipGetErrorString(e));
    }
    return TSLAM_OK;
}

// The batch's front-end results as A8 reads them, snapshotted on stream fs into the slots of the
// batch's parity: poses, the keyframes' match chains and, for a rig, the body poses.
struct BaSnap {
    double* snap;
    double* snap_body;
    int32_t* assoc;
    int par;
};
static BaSnap ba_snapshot(tslam_handle* h, const BatchCtx& c, hipStream_t fs) {
    const int par = (int)(h->batch_idx & 1);
    const BaSnap b{h->ba.fe_pose + (size_t)par * h->B * h->P * 16, h->ba.fe_body + (size_t)par * h->B * 16,
                   h->ba.kf_assoc + (size_t)par * h->B * h->P * h->g.K, par};
    launch_ba_snapshot(c, b.snap, fs);
    launch_ba_kf_assoc(c, b.assoc, h->prm.ba_kf_interval, fs);
    if (ba_rig(h)) launch_ba_snapshot_rig(c, b.snap_body, fs);
    return b;
}

// A8 of the current batch.  It may run on its own stream: it depends on this batch's poses (event
// on the stream of the last stage) and only reads ring buffers plus a snapshot of the batch's
// poses, so the next batch can start.  A sharded rank runs it once its ring holds every pair's
// keyframe data (rank 0 after the state gather, tslam_shard.cpp).
int ba_stage(tslam_handle* h, const BatchCtx& c, hipStream_t s) {
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    BA_FLUSH(h);   // the previous batch's deferred BA comes first (host state, event order)
    hipStream_t fs = h->last_stream;
    const BaSnap b = ba_snapshot(h, c, fs);
    const int par = b.par;
    const bool other = s != fs;
    if (other) {
        if (!h->ev_fe) {
            HIPCHK(hipEventCreateWithFlags(&h->ev_fe, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->ev_ba[0], hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&h->ev_ba[1], hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(h->ev_fe, fs));
        HIPCHK(hipStreamWaitEvent(s, h->ev_fe, 0));
        if (h->ba_defer) {   // enqueued at the next flush point (BA_FLUSH)
            h->ba_job.pending = true;
            h->ba_job.c = c;
            h->ba_job.s = s;
            h->ba_job.snap = b.snap;
            h->ba_job.snap_body = b.snap_body;
            h->ba_job.assoc = b.assoc;
            h->ba_job.par = par;
            h->ba_pending[par] = true;
            return TSLAM_OK;
        }
    }
    if (const hipError_t e = run_ba(h, c, s, b.snap, b.snap_body, b.assoc); e != hipSuccess)
        return fail(TSLAM_EHIP, std::string("BA: ") + hipGetErrorString(e));
    if (other) {
        HIPCHK(hipEventRecord(h->ev_ba[par], s));
        h->ba_pending[par] = true;
    }
    return TSLAM_OK;
}

// A8 as the last step of TSLAM_STAGE_ALL: snapshot and solve on the batch's own stream.  Not
// ba_stage: no deferred job is flushed here and the snapshot does not follow last_stream.
int ba_inline(tslam_handle* h, const BatchCtx& c, hipStream_t s) {
    const BaSnap b = ba_snapshot(h, c, s);
    if (const hipError_t e = run_ba(h, c, s, b.snap, b.snap_body, b.assoc); e != hipSuccess)
        return fail(TSLAM_EHIP, std::string("BA: ") + hipGetErrorString(e));
    return TSLAM_OK;
}

// tslam_reset: the window and its inertial state belong to the session
int ba_reset(tslam_handle* h) {
    for (int i = 0; i < TS_BA_MAXW; ++i) h->ba_frame[i] = -1;
    h->ba_nkf = 0;
    h->ba_last = -1;
    h->ba_solved.clear();
    if (h->prm.ba_window) {   // the inertial state of the window belongs to the session
        const size_t P = h->P + 1, W = h->prm.ba_window;
        HIPCHK(hipMemset(h->ba.ine, 0, 8 * P * W * TS_BA_INE));
        HIPCHK(hipMemset(h->ba.vel, 0, 8 * P * W * 3));
        HIPCHK(hipMemset(h->ba.bias, 0, 8 * P * W * 6));
        h->ba_ine.clear();
        h->ba_imu.clear();
        for (auto& f : h->ba_ine_slot) f.fill(0);
    }
    h->ba_pending[0] = h->ba_pending[1] = false;
    return TSLAM_OK;
}

// tslam_destroy, after the device is drained: the events, then the graph cache
void ba_destroy(tslam_handle* h) {
    for (hipEvent_t e : h->ba_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->ev_fe, h->ev_ba[0], h->ev_ba[1]})
        if (e) (void)hipEventDestroy(e);
    ba_graphs_destroy(h);
}

extern "C" {

int tslam_ba_read_map(tslam_handle* h, int pair, int64_t* gid, uint32_t* desc) {
    if (!h || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad handle or pair");
    BA_FLUSH(h);
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    const size_t WK = (size_t)h->prm.ba_window * h->g.K;
    if (gid) HIPCHK(hipMemcpy(gid, h->ba.gid + pair * WK, 8 * WK, hipMemcpyDeviceToHost));
    if (desc) HIPCHK(hipMemcpy(desc, h->ba.kf_desc + pair * WK * 8, 32 * WK, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_ba_imu_factor(tslam_handle* h, int pair, int64_t frame, const double* M, double weight) {
    if (!h || !M || pair < 0 || pair >= h->P) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    // non-finite inputs would poison the whole window's Schur system (k_ba_solve adds them to S, b)
    if (!(weight >= 0.0) || !std::isfinite(weight) || frame < 0)
        return fail(TSLAM_EINVAL, "weight must be finite and >= 0, frame >= 0");
    for (int e = 0; e < 9; ++e)
        if (!std::isfinite(M[e])) return fail(TSLAM_EINVAL, "rotation M must be finite");
    std::array<double, 10> f{};
    for (int e = 0; e < 9; ++e) f[e] = M[e];
    f[9] = weight;
    h->ba_imu[{pair, frame}] = f;
    return TSLAM_OK;
}

// A rig's inertial factors act on its body window (pair = n_pairs); a stereo pair's on its own.
static int ine_pair_check(tslam_handle* h, int pair) {
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    if (ba_rig(h) ? pair != h->P : (pair < 0 || pair >= h->P))
        return fail(TSLAM_EINVAL, ba_rig(h) ? "a rig's inertial factors go to its body window (pair = n_pairs)"
                                            : "bad pair");
    return TSLAM_OK;
}

int tslam_ba_inertial(tslam_handle* h, int pair, const double* gravity, const double* ba_prior, double ba_weight,
                      const double* bg_prior, double bg_weight) {
    if (!h || !gravity || !ba_prior || !bg_prior) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (int rc = ine_pair_check(h, pair); rc != TSLAM_OK) return rc;
    if (!(ba_weight >= 0.0) || !std::isfinite(ba_weight) || !(bg_weight >= 0.0) || !std::isfinite(bg_weight))
        return fail(TSLAM_EINVAL, "bias weights must be finite and >= 0");
    for (int e = 0; e < 3; ++e)
        if (!std::isfinite(gravity[e]) || !std::isfinite(ba_prior[e]) || !std::isfinite(bg_prior[e]))
            return fail(TSLAM_EINVAL, "non-finite input");
    auto& f = h->ba_icfg[pair];
    for (int e = 0; e < 3; ++e) {
        f[e] = gravity[e];
        f[3 + e] = ba_prior[e];
        f[7 + e] = bg_prior[e];
    }
    f[6] = ba_weight;
    f[10] = bg_weight;
    return TSLAM_OK;
}

int tslam_ba_inertial_factor(tslam_handle* h, int pair, int64_t frame, const double* record, const double* v0) {
    if (!h || !record || !v0 || frame < 0) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (int rc = ine_pair_check(h, pair); rc != TSLAM_OK) return rc;
    std::array<double, TS_BA_INE + 3> f{};
    for (int e = 0; e < TS_BA_INE; ++e) {
        if (!std::isfinite(record[e])) return fail(TSLAM_EINVAL, "non-finite factor record");
        f[e] = record[e];
    }
    if (!(f[27] > 0.0)) return fail(TSLAM_EINVAL, "dt must be > 0");
    for (int e : {28, 29, 30, 31, 71})
        if (!(f[e] >= 0.0)) return fail(TSLAM_EINVAL, "weights must be >= 0");
    for (int e = 0; e < 3; ++e) {
        if (!std::isfinite(v0[e])) return fail(TSLAM_EINVAL, "non-finite velocity");
        f[TS_BA_INE + e] = v0[e];
    }
    h->ba_ine[{pair, frame}] = f;
    return TSLAM_OK;
}

int tslam_ba_read_inertial(tslam_handle* h, int pair, double* velocity, double* bias) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (int rc = ine_pair_check(h, pair); rc != TSLAM_OK) return rc;
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    const size_t W = h->prm.ba_window;
    if (velocity) HIPCHK(hipMemcpy(velocity, h->ba.vel + pair * W * 3, 8 * W * 3, hipMemcpyDeviceToHost));
    if (bias) HIPCHK(hipMemcpy(bias, h->ba.bias + pair * W * 6, 8 * W * 6, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_ba_read(tslam_handle* h, int pair, int64_t* frames, double* cam_T_world, int32_t* landmark,
                  double* points, double* obs_uvd, int32_t* counts) {
    if (!h || pair < 0 || pair > h->P || (pair == h->P && !ba_rig(h))) return fail(TSLAM_EINVAL, "bad handle or pair");
    BA_FLUSH(h);
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    const size_t W = h->prm.ba_window, K = h->g.K, WK = W * K;
    const BaStore& b = h->ba;
    if (frames)
        for (size_t s = 0; s < W; ++s) frames[s] = h->ba_frame[s];
    if (pair == h->P) {   // the rig's body window: body_T_world per slot and the joint counts only
        if (cam_T_world) HIPCHK(hipMemcpy(cam_T_world, b.T + pair * W * 16, 8 * W * 16, hipMemcpyDeviceToHost));
        if (counts) HIPCHK(hipMemcpy(counts, b.counts + 4 * pair, 4 * 4, hipMemcpyDeviceToHost));
        if (landmark) std::fill(landmark, landmark + WK, -1);
        if (points) std::fill(points, points + WK * 3, 0.0);
        if (obs_uvd) std::fill(obs_uvd, obs_uvd + 3 * WK, std::numeric_limits<double>::quiet_NaN());
        return TSLAM_OK;
    }
    if (cam_T_world) HIPCHK(hipMemcpy(cam_T_world, b.T + pair * W * 16, 8 * W * 16, hipMemcpyDeviceToHost));
    if (landmark) HIPCHK(hipMemcpy(landmark, b.lm + pair * WK, 4 * WK, hipMemcpyDeviceToHost));
    if (points) HIPCHK(hipMemcpy(points, b.X + pair * WK * 3, 8 * WK * 3, hipMemcpyDeviceToHost));
    if (obs_uvd) {
        HIPCHK(hipMemcpy(obs_uvd, b.u + pair * WK, 8 * WK, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(obs_uvd + WK, b.v + pair * WK, 8 * WK, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(obs_uvd + 2 * WK, b.d + pair * WK, 8 * WK, hipMemcpyDeviceToHost));
    }
    if (counts) HIPCHK(hipMemcpy(counts, b.counts + 4 * pair, 4 * 4, hipMemcpyDeviceToHost));
    return TSLAM_OK;
}

int tslam_ba_replay_schur(tslam_handle* h, int pair, int reps, void* stream, double* us_per_launch,
                          double* flops_per_launch) {
    if (!h || pair < 0 || pair >= h->P || reps < 1) return fail(TSLAM_EINVAL, "bad argument");
    BA_FLUSH(h);
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    if ((int)h->ba_solved.size() <= pair) return fail(TSLAM_ESTATE, "no window solved yet");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    const double zero = 0.0;
    HIPCHK(hipMemcpy(h->ba.flops, &zero, sizeof(double), hipMemcpyHostToDevice));
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const BatchCtx c = make_ctx(h);
    HIPCHK(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) launch_ba_schur(c, h->ba_solved[pair], s);
    HIPCHK(hipEventRecord(e1, s));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    double fl = 0.0;
    HIPCHK(hipMemcpy(&fl, h->ba.flops, sizeof(double), hipMemcpyDeviceToHost));
    if (us_per_launch) *us_per_launch = 1e3 * ms / reps;
    if (flops_per_launch) *flops_per_launch = fl / reps;
    return TSLAM_OK;
}

int tslam_ba_defer(tslam_handle* h, int defer) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    h->ba_defer = defer != 0;
    return TSLAM_OK;
}

int tslam_ba_graph(tslam_handle* h, int enable) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    h->ba_graph = enable != 0;
    return TSLAM_OK;
}

int tslam_ba_split_solve(tslam_handle* h, int split) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    h->ba_split = split != 0;
    return TSLAM_OK;
}

int tslam_ba_profile(tslam_handle* h, int max_launches, double* schur_ms, int64_t* schur_launches, double* schur_flops) {
    if (!h) return fail(TSLAM_EINVAL, "null handle");
    BA_FLUSH(h);
    if (!h->prm.ba_window) return fail(TSLAM_ESTATE, "local BA is off (ba_window = 0)");
    int rc = tslam_sync(h);
    if (rc != TSLAM_OK) return rc;
    BaTiming& t = h->ba_timing;
    double ms = 0.0;
    for (int i = 0; i < t.used; ++i) {
        float e = 0.0f;
        HIPCHK(hipEventElapsedTime(&e, t.ev[2 * i], t.ev[2 * i + 1]));
        ms += e;
    }
    double fl = 0.0;
    HIPCHK(hipMemcpy(&fl, h->ba.flops, sizeof(double), hipMemcpyDeviceToHost));
    if (schur_ms) *schur_ms = ms;
    if (schur_launches) *schur_launches = t.used;
    if (schur_flops) *schur_flops = t.ev ? fl : 0.0;
    // restart: (re)arm with room for max_launches timed launches, or disarm with 0
    const double zero = 0.0;
    HIPCHK(hipMemcpy(h->ba.flops, &zero, sizeof(double), hipMemcpyHostToDevice));
    t.used = 0;
    if (max_launches < 0) return fail(TSLAM_EINVAL, "max_launches must be >= 0");
    if ((size_t)max_launches * 2 > h->ba_events.size()) {
        while (h->ba_events.size() < (size_t)max_launches * 2) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            h->ba_events.push_back(e);
        }
    }
    t.ev = max_launches ? h->ba_events.data() : nullptr;
    t.cap = max_launches;
    return TSLAM_OK;
}

}  // extern "C"
