// tslam_shard.cpp — the library's own driver of a sharded rig (one camera stream per
// GPU; replaces cuVSLAM's multicam mode, launch/thor_visual_slam.launch.py:49,81).
//
// A driver owns, per local rank, the exchange buffers (two sets, by batch parity), three streams and
// the events between them, and runs one batch of every local rank through the stages of a sharded
// handle (tslam_set_shard) with the exchanges in between:
//
//   stereo rig                                         camera-sharded RGB-D rig
//   x : raw images of the frames each peer solves ──┐   f : RECTIFY .. DESCRIBE (own cameras)
//   f : RECTIFY, DETECT, DESCRIBE, pack streams      │   b : MATCH, POSE (own cameras, whole batch),
//   x : ── exchange 1 (raw images, stream blocks) ◄──┘       pack pair blocks per peer range
//   b : import raw + unpack streams, MATCH, POSE(+rig)  b : ── exchange 1 (pair blocks)
//   b : [state blocks ── gather to rank 0 ── unpack]    b : unpack pairs, KERNEL_RIG (own range)
//   b : pack pose records ── exchange 2 (all-gather) ── unpack, CHAIN  (both)
//   b : [rank 0: local BA]; [results into pinned slots]
//
// f = front stream (high priority), x = exchange stream, b = back stream.  Batch s's raw exchange
// overlaps its front end and batch s+1's front end overlaps batch s's back end; a parity's receive
// buffers are reused once the imports of batch s-2 are done (event), its send buffers once the
// collectives that read them are.  Nothing here synchronises the host.
//
// Any batch of 1 .. max_batch frames: rank q's back end owns frames [q n / N, (q + 1) n / N) (ranges
// may differ by a frame or be empty).  Who sends what to whom, and where it lands, is the exchange
// plan (tslam_xplan.h): the slot layout of every buffer and each rank's ordered operations per
// exchange; this file allocates, packs, issues and unpacks by it.  Raw images go straight from the
// caller's input (and the previous batch's last frame) to the peers: no staging copy.
//
// Pair split (TSLAM_SHARD_PAIRS, one camera per rank): rank r's back end solves pair r / 2 over
// half r & 1 of the batch, so the raw images and stream blocks go to the partner (r ^ 1) only —
// half a batch + 1 frame instead of a range + 1 frame to each of world - 1 peers; the rig pose of a
// rank's rig range (tslam_ranges.h rig_slot, inside its half) then takes the other pairs' pair
// blocks (pose, stats, the 5 correspondence columns it reads) from the ranks of the same half.
// Fewer bytes per rank, all of the image traffic on the one partner link.
//
// State gather (TSLAM_SHARD_GATHER, implied by local BA): every rank sends rank 0 the temporal
// matches and disparities of its range and the keypoints + descriptors of its left cameras, so
// rank 0's ring holds what the one-handle path's local BA, loop closure and relocalisation read;
// rank 0 then runs the local BA itself (the other ranks keep no window).
//
// Transports: RCCL (ncclSend / ncclRecv / ncclAllGather over xGMI; two communicators per rank so
// the pose all-gather of batch s, on the back stream, never shares a communicator with batch s+1's
// exchange on the exchange stream), created per process (tslam_comm_init: one local rank) or for
// all devices of one process (tslam_group_create: ncclCommInitAll); or COPY (device-to-device
// copies pushed on the sender's stream: a group of ranks in one process, also several on one device,
// used to test world > 1 on one GPU).  Both issue the plan's operations: RCCL a rank's sends and
// receives in one group, COPY every rank's sends as copies to the plan's destination offsets.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "tslam_common.h"
#include "tslam_internal.h"

#define SHCHK(expr)                                                                                            \
    do {                                                                                                       \
        hipError_t e__ = (expr);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return tslam_internal_fail(TSLAM_EHIP, (std::string(#expr) + ": " + hipGetErrorString(e__)).c_str()); \
    } while (0)
#define NCCLCHK(expr)                                                                                          \
    do {                                                                                                       \
        ncclResult_t r__ = (expr);                                                                             \
        if (r__ != ncclSuccess)                                                                                \
            return tslam_internal_fail(TSLAM_EHIP, (std::string(#expr) + ": " + ncclGetErrorString(r__)).c_str()); \
    } while (0)
#define RC(expr)                          \
    do {                                  \
        const int rc__ = (expr);          \
        if (rc__ != TSLAM_OK) return rc__; \
    } while (0)

namespace {
struct Span {   // one timed segment of one batch (TSLAM_SHARD_PROFILE)
    int seg;
    hipEvent_t a, b;
};

struct Rank {
    tslam_handle* h = nullptr;
    int rank = 0, device = 0;
    ncclComm_t comm_x = nullptr, comm_p = nullptr;
    hipStream_t fs = nullptr, xs = nullptr, bs = nullptr;
    hipStream_t serial = nullptr;   // TSLAM_SHARD_SERIAL: the device's one stream (owned by its first rank)
    bool serial_owner = false;
    hipEvent_t ev_in = nullptr, ev_front = nullptr, ev_x = nullptr, ev_push = nullptr, ev_done = nullptr;
    hipEvent_t consumed[2] = {nullptr, nullptr};   // this parity's receive buffers were read
    bool consumed_armed[2] = {false, false};
    bool done_armed = false;
    uint8_t* send[X_KINDS][2] = {};   // the exchange buffers by kind and batch parity (tslam_xplan.h)
    uint8_t* recv[X_KINDS][2] = {};
    uint8_t* prev_raw = nullptr;      // the previous batch's last frame of this rank's cameras
    std::vector<void*> allocs;
    // profiling
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<Span> spans;
    double seg_us[TSLAM_SEG_COUNT] = {};
    int64_t timed_batches = 0;
};
}  // namespace

struct tslam_shard_driver {
    int transport = TSLAM_TRANSPORT_RCCL;
    XGeom g{};                           // the exchange plan's geometry: the rig, the options, this batch's n
    bool rig = false, ba = false;
    int flags = 0;                       // TSLAM_SHARD_* options
    bool ready[X_KINDS] = {};            // the kind's buffers are allocated
    int64_t batches = 0;
    std::vector<Rank> ranks;   // local ranks: all of a group, one after tslam_comm_init
    // TSLAM_SHARD_GATHER is implied by local BA; TSLAM_SHARD_PAIRS: rank r's back end solves pair
    // r / 2 over half r & 1 of the batch, the stereo exchange goes to the partner (r ^ 1) only
    void set_flags(int f) {
        flags = f;
        g.gather = g.world > 1 && !g.rgbd && (ba || (f & TSLAM_SHARD_GATHER));
        g.pairs = (f & TSLAM_SHARD_PAIRS) != 0;
    }
};

// The rank's streams: its own three, or with TSLAM_SHARD_SERIAL one stream per device shared by
// every rank on it (each kernel and copy then runs alone: the per-rank profile of a one-GPU
// rehearsal reports isolated durations)
static hipStream_t FS(const tslam_shard_driver* d, const Rank& r) { return (d->flags & TSLAM_SHARD_SERIAL) ? r.serial : r.fs; }
static hipStream_t XS(const tslam_shard_driver* d, const Rank& r) { return (d->flags & TSLAM_SHARD_SERIAL) ? r.serial : r.xs; }
static hipStream_t BS(const tslam_shard_driver* d, const Rank& r) { return (d->flags & TSLAM_SHARD_SERIAL) ? r.serial : r.bs; }

static void destroy_driver(tslam_shard_driver* d) {
    if (!d) return;
    for (Rank& r : d->ranks) {
        (void)hipSetDevice(r.device);
        (void)hipDeviceSynchronize();
        if (r.comm_p) (void)ncclCommDestroy(r.comm_p);
        if (r.comm_x) (void)ncclCommDestroy(r.comm_x);
        for (hipEvent_t e : {r.ev_in, r.ev_front, r.ev_x, r.ev_push, r.ev_done, r.consumed[0], r.consumed[1]})
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : r.ev_pool) (void)hipEventDestroy(e);
        for (hipStream_t s : {r.fs, r.xs, r.bs})
            if (s) (void)hipStreamDestroy(s);
        if (r.serial && r.serial_owner) (void)hipStreamDestroy(r.serial);
        for (void* p : r.allocs) (void)hipFree(p);
        r.allocs.clear();
    }
    delete d;
}

extern "C" void tslam_internal_driver_destroy(tslam_shard_driver* d) { destroy_driver(d); }

static int alloc(Rank& r, uint8_t** p, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes ? bytes : 16);
    if (e != hipSuccess) return tslam_internal_fail(TSLAM_ENOMEM, (std::string("hipMalloc: ") + hipGetErrorString(e)).c_str());
    r.allocs.push_back(q);
    *p = (uint8_t*)q;
    SHCHK(hipMemset(q, 0, bytes ? bytes : 16));
    return TSLAM_OK;
}

// Geometry of the driver from its ranks' handles (all the same rig, sharded by tslam_set_shard).
static int plan(tslam_shard_driver* d, tslam_handle* h, int world) {
    tslam_handle_info in{};
    RC(tslam_internal_info(h, &in));
    if (in.ba && in.rgbd) return tslam_internal_fail(TSLAM_EINVAL, "a camera-sharded RGB-D rig runs without local BA");
    if (in.C % world) return tslam_internal_fail(TSLAM_EINVAL, "the cameras must divide by world");
    if (world > in.B) return tslam_internal_fail(TSLAM_EINVAL, "world must be <= max_batch");
    d->rig = in.rig != 0;
    d->ba = in.ba != 0;
    d->g = tslam_xgeom(in, world, 0, false, false);
    d->set_flags(0);
    return TSLAM_OK;
}

// A rank's send and receive buffers of the exchanges in `kinds`, both parities, sized by the plan.
static int setup_buffers(tslam_shard_driver* d, Rank& r, std::initializer_list<int> kinds) {
    SHCHK(hipSetDevice(r.device));
    for (int k = 0; k < 2; ++k)
        for (int w : kinds) {
            if (size_t b = xp_buf_bytes(d->g, w, XB_SEND, r.rank)) RC(alloc(r, &r.send[w][k], b));
            if (size_t b = xp_buf_bytes(d->g, w, XB_RECV, r.rank)) RC(alloc(r, &r.recv[w][k], b));
        }
    SHCHK(hipDeviceSynchronize());   // the zeroing (null stream) lands before the rank's streams use them
    return TSLAM_OK;
}
// the buffers of an option (the state gather, the pair split's pair blocks), when first needed
static int setup_option(tslam_shard_driver* d, int w, bool on) {
    if (!on || d->ready[w]) return TSLAM_OK;
    for (Rank& r : d->ranks) RC(setup_buffers(d, r, {w}));
    d->ready[w] = true;
    return TSLAM_OK;
}

static int setup_rank(tslam_shard_driver* d, Rank& r) {
    tslam_handle_info in{};
    RC(tslam_internal_info(r.h, &in));
    r.device = in.device;
    SHCHK(hipSetDevice(r.device));
    int lo = 0, hi = 0;
    SHCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    SHCHK(hipStreamCreateWithPriority(&r.fs, hipStreamNonBlocking, hi));   // the front end is the critical path
    SHCHK(hipStreamCreateWithFlags(&r.xs, hipStreamNonBlocking));
    SHCHK(hipStreamCreateWithFlags(&r.bs, hipStreamNonBlocking));
    for (hipEvent_t* e : {&r.ev_in, &r.ev_front, &r.ev_x, &r.ev_push, &r.ev_done, &r.consumed[0], &r.consumed[1]})
        SHCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    RC(setup_buffers(d, r, {X_RAW, X_FEAT, X_POSE}));   // RGB-D: the plan gives RAW no bytes
    if (!d->g.rgbd) RC(alloc(r, &r.prev_raw, (size_t)d->g.S * d->g.img));
    SHCHK(hipDeviceSynchronize());
    return TSLAM_OK;
}

// ---- profiling (TSLAM_SHARD_PROFILE) ------------------------------------------------------------
static int span_begin(tslam_shard_driver* d, Rank& r, int seg, hipStream_t s) {
    if (!(d->flags & TSLAM_SHARD_PROFILE)) return TSLAM_OK;
    SHCHK(hipSetDevice(r.device));
    while (r.ev_pool.size() < r.ev_used + 2) {
        hipEvent_t e;
        SHCHK(hipEventCreate(&e));
        r.ev_pool.push_back(e);
    }
    Span sp{seg, r.ev_pool[r.ev_used], r.ev_pool[r.ev_used + 1]};
    r.ev_used += 2;
    SHCHK(hipEventRecord(sp.a, s));
    r.spans.push_back(sp);
    return TSLAM_OK;
}
static int span_end(tslam_shard_driver* d, Rank& r, hipStream_t s) {
    if (!(d->flags & TSLAM_SHARD_PROFILE)) return TSLAM_OK;
    SHCHK(hipEventRecord(r.spans.back().b, s));
    return TSLAM_OK;
}
// the span between an event already recorded on one stream and now on another
static int span_between(tslam_shard_driver* d, Rank& r, int seg, hipStream_t from, hipStream_t to) {
    RC(span_begin(d, r, seg, from));
    return span_end(d, r, to);
}
static int run_timed(tslam_shard_driver* d, Rank& r, int seg, int stage, hipStream_t s) {
    RC(span_begin(d, r, seg, s));
    RC(tslam_run_stage(r.h, stage, s));
    return span_end(d, r, s);
}

// ---- exchanges (the plan: tslam_xplan.h) --------------------------------------------------------
// The stream an exchange runs on (sender and receiver side): stereo raw images and stream blocks
// on the exchange stream, pair blocks, state blocks and pose records on the back stream.
static hipStream_t xstream(const tslam_shard_driver* d, const Rank& r, int w) {
    return (w >= X_PAIRB || d->g.rgbd) ? BS(d, r) : XS(d, r);
}
static uint8_t* buffer(const Rank& r, int w, int buf, int k, const uint8_t* images) {
    return buf == XB_INPUT ? (uint8_t*)images : buf == XB_PREV ? r.prev_raw : buf == XB_SEND ? r.send[w][k] : r.recv[w][k];
}

static int exchange(tslam_shard_driver* d, int w, int k, const uint8_t* const* images) {
    const XGeom& g = d->g;
    if (d->transport == TSLAM_TRANSPORT_RCCL) {   // every local rank's operations, in plan order
        ncclResult_t send_recv = ncclSuccess;
        NCCLCHK(ncclGroupStart());
        for (size_t i = 0; i < d->ranks.size(); ++i) {
            Rank& r = d->ranks[i];
            hipStream_t s = xstream(d, r, w);
            if (w == X_POSE) {
                NCCLCHK(ncclAllGather(r.send[w][k], r.recv[w][k], xp_pose_bytes(g), ncclUint8, r.comm_p, s));
                continue;
            }
            xp_ops(g, w, r.rank, [&](const XOp& o) {
                uint8_t* p = buffer(r, w, o.buf, k, images[i]) + o.off;
                ncclComm_t comm = o.comm == XC_P ? r.comm_p : r.comm_x;
                if (send_recv != ncclSuccess) return;
                send_recv = o.send ? ncclSend(p, o.bytes, ncclUint8, o.peer, comm, s) : ncclRecv(p, o.bytes, ncclUint8, o.peer, comm, s);
            });
        }
        NCCLCHK(send_recv);
        NCCLCHK(ncclGroupEnd());
        return TSLAM_OK;
    }
    // COPY: each sender pushes its sends into its peers' receive buffers on its own exchange-side
    // stream, once the peer has consumed that parity's previous use (its imports of batch s-2; on the
    // back stream, the end of its batch s-1); the receivers wait for every push
    hipError_t copy = hipSuccess;
    for (size_t i = 0; i < d->ranks.size(); ++i) {
        Rank& src = d->ranks[i];
        SHCHK(hipSetDevice(src.device));
        hipStream_t s = xstream(d, src, w);
        for (Rank& dst : d->ranks) {
            if (!xp_linked(g, w, src.rank, dst.rank)) continue;
            if (w <= X_FEAT ? dst.consumed_armed[k] : dst.done_armed && &dst != &src)
                SHCHK(hipStreamWaitEvent(s, w <= X_FEAT ? dst.consumed[k] : dst.ev_done, 0));
            xp_sends(g, w, src.rank, dst.rank, [&](const XOp& o) {
                if (copy == hipSuccess)
                    copy = hipMemcpyAsync(dst.recv[w][k] + o.dst_off, buffer(src, w, o.buf, k, images[i]) + o.off, o.bytes,
                                        hipMemcpyDeviceToDevice, s);
            });
            SHCHK(copy);
        }
        SHCHK(hipEventRecord(src.ev_push, s));
    }
    for (Rank& dst : d->ranks) {
        if (w == X_STATE && dst.rank != 0) continue;
        SHCHK(hipSetDevice(dst.device));
        hipStream_t s = xstream(d, dst, w);
        for (Rank& src : d->ranks)
            if (&src != &dst) SHCHK(hipStreamWaitEvent(s, src.ev_push, 0));
    }
    return TSLAM_OK;
}

static int submit(tslam_shard_driver* d, const uint8_t* const* images, int n, void* const* streams) {
    if (n < 1 || n > d->g.B) return tslam_internal_fail(TSLAM_EINVAL, "a sharded batch needs 1 <= n_frames <= max_batch");
    RC(setup_option(d, X_STATE, d->g.gather));
    RC(setup_option(d, X_PAIRB, d->g.pairs));
    d->g.n = n;
    const XGeom& g = d->g;
    const int k = (int)(d->batches & 1), N = g.world, S = g.S;
    const bool prof = (d->flags & TSLAM_SHARD_PROFILE) != 0;
    // TSLAM_SHARD_SOLO: rank 0's work only, no exchange (the receive buffers keep what the last
    // full batch left): rank 0's step on a GPU of its own with the exchange hidden
    const bool solo = (d->flags & TSLAM_SHARD_SOLO) != 0;
    const bool xchg = N > 1 && !solo;
    auto idle = [&](const Rank& r) { return solo && r.rank != 0; };
    for (size_t i = 0; i < d->ranks.size(); ++i) {   // inputs, buffer reuse
        Rank& r = d->ranks[i];
        if (idle(r)) continue;
        SHCHK(hipSetDevice(r.device));
        SHCHK(hipEventRecord(r.ev_in, streams ? (hipStream_t)streams[i] : nullptr));
        for (hipStream_t s : {FS(d, r), XS(d, r), BS(d, r)}) SHCHK(hipStreamWaitEvent(s, r.ev_in, 0));
        if (r.consumed_armed[k])
            for (hipStream_t s : {FS(d, r), XS(d, r)}) SHCHK(hipStreamWaitEvent(s, r.consumed[k], 0));
        RC(tslam_begin_batch(r.h, images[i], n));
    }
    if (!g.rgbd && xchg) RC(exchange(d, X_RAW, k, images));   // straight from the inputs
    for (size_t i = 0; i < d->ranks.size(); ++i) {   // this batch's last frame becomes prev_raw (after the sends)
        Rank& r = d->ranks[i];
        if (g.rgbd || idle(r)) continue;
        SHCHK(hipSetDevice(r.device));
        const size_t frame = (size_t)S * g.img;
        SHCHK(hipMemcpyAsync(r.prev_raw, images[i] + (size_t)(n - 1) * frame, frame, hipMemcpyDeviceToDevice, XS(d, r)));
    }
    for (Rank& r : d->ranks) {   // front end of the rank's cameras (+ its stream blocks per peer)
        if (idle(r)) continue;
        if (prof) {
            RC(run_timed(d, r, TSLAM_SEG_RECTIFY, TSLAM_KERNEL_RECTIFY_PYRAMID, FS(d, r)));
            RC(run_timed(d, r, TSLAM_SEG_DETECT, TSLAM_KERNEL_DETECT, FS(d, r)));
            RC(run_timed(d, r, TSLAM_SEG_SELECT, TSLAM_KERNEL_SELECT, FS(d, r)));
            RC(run_timed(d, r, TSLAM_SEG_DESCRIBE, TSLAM_KERNEL_DESCRIBE, FS(d, r)));
        } else {
            for (int st : {TSLAM_STAGE_RECTIFY, TSLAM_STAGE_DETECT, TSLAM_STAGE_DESCRIBE}) RC(tslam_run_stage(r.h, st, FS(d, r)));
        }
        if (g.rgbd) continue;
        if (N > 1) {
            RC(span_begin(d, r, TSLAM_SEG_PACK, FS(d, r)));
            if (g.pairs) RC(tslam_internal_pack_partner(r.h, r.send[X_FEAT][k], FS(d, r)));   // the partner's half
            else RC(tslam_pack_streams_peers(r.h, r.send[X_FEAT][k], FS(d, r)));   // every peer's frames, one launch
            RC(span_end(d, r, FS(d, r)));
        }
        SHCHK(hipSetDevice(r.device));
        SHCHK(hipEventRecord(r.ev_front, FS(d, r)));
        SHCHK(hipStreamWaitEvent(XS(d, r), r.ev_front, 0));
    }
    if (!g.rgbd && xchg) RC(exchange(d, X_FEAT, k, images));
    for (Rank& r : d->ranks) {   // back end
        if (idle(r)) continue;
        if (!g.rgbd) {
            // the other cameras of frames lo-1 .. hi-1 of this rank's range into the ring
            SHCHK(hipSetDevice(r.device));
            SHCHK(hipEventRecord(r.ev_x, XS(d, r)));
            SHCHK(hipStreamWaitEvent(BS(d, r), r.ev_x, 0));
            if (prof && N > 1) RC(span_between(d, r, TSLAM_SEG_EXCHANGE_WAIT, FS(d, r), BS(d, r)));   // front done -> data landed
            if (N > 1) {
                RC(span_begin(d, r, TSLAM_SEG_IMPORT, BS(d, r)));
                if (g.pairs) RC(tslam_internal_import_partner(r.h, r.recv[X_RAW][k], r.recv[X_FEAT][k], BS(d, r)));
                else RC(tslam_import_peers(r.h, r.recv[X_RAW][k], r.recv[X_FEAT][k], BS(d, r)));
                RC(span_end(d, r, BS(d, r)));
            }
            SHCHK(hipEventRecord(r.consumed[k], BS(d, r)));
            r.consumed_armed[k] = true;
        }
        if (prof) {
            RC(run_timed(d, r, TSLAM_SEG_MATCH, TSLAM_KERNEL_MATCH, BS(d, r)));
            RC(run_timed(d, r, TSLAM_SEG_MATCH_REFINE, TSLAM_KERNEL_MATCH_REFINE, BS(d, r)));
            RC(run_timed(d, r, TSLAM_SEG_POSE, TSLAM_KERNEL_POSE, BS(d, r)));
            if (d->rig && !g.rgbd && !g.pairs) RC(run_timed(d, r, TSLAM_SEG_RIG, TSLAM_KERNEL_RIG, BS(d, r)));
        } else {
            RC(tslam_run_stage(r.h, TSLAM_STAGE_MATCH, BS(d, r)));
            RC(tslam_run_stage(r.h, TSLAM_STAGE_POSE, BS(d, r)));
        }
        if (g.rgbd)   // this rank's cameras over every peer's frame range
            for (int q = 0; q < N; ++q) {
                int lo;
                const int nf = xp_rig_range(g, q, &lo);
                if (q != r.rank && nf > 0)
                    RC(tslam_pack_pairs(r.h, lo, nf, r.rank * S, (r.rank + 1) * S,
                                        r.send[X_FEAT][k] + xp_slot_off(g, X_FEAT, XB_SEND, q), BS(d, r)));
            }
    }
    if (g.rgbd) {
        if (xchg) RC(exchange(d, X_FEAT, k, images));
        for (Rank& r : d->ranks) {
            if (idle(r)) continue;
            int lo;
            const int nf = xp_rig_range(g, r.rank, &lo);
            for (int q = 0; q < N; ++q)
                if (q != r.rank && nf > 0)
                    RC(tslam_unpack_pairs(r.h, lo, nf, q * S, (q + 1) * S, r.recv[X_FEAT][k] + xp_slot_off(g, X_FEAT, XB_RECV, q),
                                          BS(d, r)));
            SHCHK(hipSetDevice(r.device));
            SHCHK(hipEventRecord(r.consumed[k], BS(d, r)));
            r.consumed_armed[k] = true;
            if (d->rig) RC(run_timed(d, r, TSLAM_SEG_RIG, TSLAM_KERNEL_RIG, BS(d, r)));
        }
    }
    if (g.pairs) {   // every pair's blocks of a rank's rig range from the ranks of its half, then the rig pose
        if (g.P > 1) {
            for (Rank& r : d->ranks) {
                if (idle(r)) continue;
                RC(span_begin(d, r, TSLAM_SEG_PAIR_BLOCKS, BS(d, r)));
                for (int q = 0; q < N; ++q) {
                    int lo;
                    const int nf = xp_rig_range(g, q, &lo);
                    if (xp_linked(g, X_PAIRB, r.rank, q) && nf > 0)
                        RC(tslam_pack_pairs(r.h, lo, nf, r.rank / 2, r.rank / 2 + 1,
                                            r.send[X_PAIRB][k] + xp_slot_off(g, X_PAIRB, XB_SEND, q), BS(d, r)));
                }
            }
            if (!solo) RC(exchange(d, X_PAIRB, k, images));
            for (Rank& r : d->ranks) {
                if (idle(r)) continue;
                int lo;
                const int nf = xp_rig_range(g, r.rank, &lo);
                for (int q = 0; q < N; ++q)
                    if (xp_linked(g, X_PAIRB, q, r.rank) && nf > 0)
                        RC(tslam_unpack_pairs(r.h, lo, nf, q / 2, q / 2 + 1, r.recv[X_PAIRB][k] + xp_slot_off(g, X_PAIRB, XB_RECV, q),
                                              BS(d, r)));
                RC(span_end(d, r, BS(d, r)));
            }
        }
        if (d->rig)
            for (Rank& r : d->ranks)
                if (!idle(r)) RC(run_timed(d, r, TSLAM_SEG_RIG, TSLAM_KERNEL_RIG, BS(d, r)));
    }
    if (g.gather) {   // every rank's share of the pairs' state into rank 0's ring
        for (Rank& r : d->ranks) {
            if (r.rank == 0 || idle(r)) continue;
            RC(span_begin(d, r, TSLAM_SEG_STATE, BS(d, r)));
            RC(tslam_internal_state_blocks(r.h, 1, r.rank, r.rank * S, (r.rank + 1) * S, r.send[X_STATE][k], BS(d, r)));
            RC(span_end(d, r, BS(d, r)));
        }
        if (!solo) RC(exchange(d, X_STATE, k, images));
        for (Rank& r : d->ranks) {
            if (r.rank != 0) continue;
            RC(span_begin(d, r, TSLAM_SEG_STATE, BS(d, r)));
            for (int q = 1; q < N; ++q)
                RC(tslam_internal_state_blocks(r.h, 0, q, q * S, (q + 1) * S, r.recv[X_STATE][k] + xp_slot_off(g, X_STATE, XB_RECV, q),
                                               BS(d, r)));
            RC(span_end(d, r, BS(d, r)));
        }
    }
    for (Rank& r : d->ranks) {
        if (idle(r)) continue;
        RC(tslam_pack_poses(r.h, r.send[X_POSE][k], BS(d, r)));
        RC(span_begin(d, r, TSLAM_SEG_POSE_GATHER, BS(d, r)));
    }
    if (!solo) RC(exchange(d, X_POSE, k, images));
    for (size_t i = 0; i < d->ranks.size(); ++i) {
        Rank& r = d->ranks[i];
        if (idle(r)) continue;
        RC(span_end(d, r, BS(d, r)));
        RC(tslam_unpack_poses(r.h, r.recv[X_POSE][k], BS(d, r)));
        RC(run_timed(d, r, TSLAM_SEG_CHAIN, TSLAM_KERNEL_CHAIN, BS(d, r)));
        // local BA on rank 0 once its ring holds every pair (the back stream keeps it ordered before
        // the next batch's imports; tslam_run_stage orders it after the next-but-one front end)
        if (d->ba && (r.rank == 0 || N == 1) && (g.gather || N == 1))
            RC(run_timed(d, r, TSLAM_SEG_BA, TSLAM_STAGE_BA, BS(d, r)));
        if (d->flags & TSLAM_SHARD_RESULTS) RC(tslam_internal_stash(r.h, BS(d, r)));
        RC(tslam_end_batch(r.h));
        SHCHK(hipSetDevice(r.device));
        SHCHK(hipEventRecord(r.ev_done, BS(d, r)));
        r.done_armed = true;
        // the caller's stream orders after the batch (results in stream order), or with
        // TSLAM_SHARD_PIPELINE after the batch's last read of its input and receive buffers, so
        // that the next batch's front end overlaps this batch's back end
        SHCHK(hipStreamWaitEvent(streams ? (hipStream_t)streams[i] : nullptr,
                                 (d->flags & TSLAM_SHARD_PIPELINE) ? r.consumed[k] : r.ev_done, 0));
        if (prof) r.timed_batches += 1;
    }
    d->batches += 1;
    return TSLAM_OK;
}

// Sum the finished spans into the per-segment totals (synchronises the rank's device).
static int collect(Rank& r) {
    if (r.spans.empty()) return TSLAM_OK;
    SHCHK(hipSetDevice(r.device));
    SHCHK(hipDeviceSynchronize());
    for (const Span& sp : r.spans) {
        float ms = 0.0f;
        SHCHK(hipEventElapsedTime(&ms, sp.a, sp.b));
        r.seg_us[sp.seg] += 1e3 * (double)ms;
    }
    r.spans.clear();
    r.ev_used = 0;
    return TSLAM_OK;
}

static Rank* rank_of(tslam_shard_driver* d, tslam_handle* h) {
    for (Rank& r : d->ranks)
        if (r.h == h) return &r;
    return nullptr;
}

extern "C" {

int tslam_comm_unique_id(void* id128) {
    if (!id128) return tslam_internal_fail(TSLAM_EINVAL, "null id");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return TSLAM_OK;
}

int tslam_comm_init(tslam_handle* h, const void* id128, int rank, int world) {
    if (!h || !id128) return tslam_internal_fail(TSLAM_EINVAL, "bad argument");
    if (tslam_internal_driver(h)) return tslam_internal_fail(TSLAM_ESTATE, "communicator already set");
    if (world < 1 || rank < 0 || rank >= world) return tslam_internal_fail(TSLAM_EINVAL, "need 0 <= rank < world");
    auto* d = new tslam_shard_driver();
    int rc = plan(d, h, world);
    if (rc == TSLAM_OK) rc = tslam_set_shard(h, rank * d->g.S, (rank + 1) * d->g.S, rank, world);
    if (rc != TSLAM_OK) {
        delete d;
        return rc;
    }
    d->transport = TSLAM_TRANSPORT_RCCL;
    d->ranks.resize(1);
    Rank& r = d->ranks[0];
    r.h = h;
    r.rank = rank;
    rc = setup_rank(d, r);
    if (rc == TSLAM_OK) {
        ncclUniqueId id;
        memcpy(&id, id128, sizeof(id));
        ncclResult_t nr = ncclCommInitRank(&r.comm_x, world, id, rank);
        // the pose all-gather's (and the state gather's) own communicator (same ranks)
        if (nr == ncclSuccess) nr = ncclCommSplit(r.comm_x, 0, rank, &r.comm_p, nullptr);
        if (nr != ncclSuccess) rc = tslam_internal_fail(TSLAM_EHIP, (std::string("RCCL communicator: ") + ncclGetErrorString(nr)).c_str());
    }
    if (rc == TSLAM_OK) rc = tslam_internal_attach_driver(h, d, true);
    if (rc != TSLAM_OK) {
        (void)tslam_set_shard(h, 0, (int)(d->g.S * world), 0, 1);
        destroy_driver(d);
    }
    return rc;
}

int tslam_submit_sharded(tslam_handle* h, const uint8_t* images, int n_frames, void* stream) {
    if (!h || !images) return tslam_internal_fail(TSLAM_EINVAL, "bad argument");
    tslam_shard_driver* d = tslam_internal_driver(h);
    if (!d || d->ranks.size() != 1) return tslam_internal_fail(TSLAM_ESTATE, "tslam_comm_init first");
    void* streams[1] = {stream};
    return submit(d, &images, n_frames, streams);
}

int tslam_shard_options(tslam_handle* h, int flags) {
    if (!h) return tslam_internal_fail(TSLAM_EINVAL, "null handle");
    tslam_shard_driver* d = tslam_internal_driver(h);
    if (!d) return tslam_internal_fail(TSLAM_ESTATE, "the handle is not driven (tslam_comm_init / tslam_group_create)");
    if (flags & ~(TSLAM_SHARD_GATHER | TSLAM_SHARD_RESULTS | TSLAM_SHARD_PROFILE | TSLAM_SHARD_SERIAL |
                  TSLAM_SHARD_PIPELINE | TSLAM_SHARD_SOLO | TSLAM_SHARD_PAIRS))
        return tslam_internal_fail(TSLAM_EINVAL, "unknown TSLAM_SHARD_* flag");
    if ((flags & TSLAM_SHARD_SOLO) && (int)d->ranks.size() != d->g.world)
        return tslam_internal_fail(TSLAM_EINVAL, "TSLAM_SHARD_SOLO needs every rank in this process (tslam_group_create)");
    if ((flags & TSLAM_SHARD_GATHER) && d->g.rgbd)
        return tslam_internal_fail(TSLAM_EINVAL, "the state gather describes a stereo rig");
    if ((flags & TSLAM_SHARD_PAIRS) && (d->g.rgbd || d->g.S != 1 || d->g.world < 2))
        return tslam_internal_fail(TSLAM_EINVAL, "the pair split shards a stereo rig with one camera per rank");
    if ((flags & TSLAM_SHARD_PAIRS) && (d->ba || (flags & TSLAM_SHARD_GATHER)))
        return tslam_internal_fail(TSLAM_EINVAL, "the pair split runs without the state gather (no local BA)");
    // the streams may change (TSLAM_SHARD_SERIAL): everything enqueued so far finishes first
    for (Rank& r : d->ranks) {
        SHCHK(hipSetDevice(r.device));
        SHCHK(hipDeviceSynchronize());
    }
    if (flags & TSLAM_SHARD_SERIAL)
        for (size_t i = 0; i < d->ranks.size(); ++i) {
            Rank& r = d->ranks[i];
            if (r.serial) continue;
            for (size_t j = 0; j < i && !r.serial; ++j)
                if (d->ranks[j].device == r.device) r.serial = d->ranks[j].serial;
            if (!r.serial) {
                SHCHK(hipSetDevice(r.device));
                SHCHK(hipStreamCreateWithFlags(&r.serial, hipStreamNonBlocking));
                r.serial_owner = true;
            }
        }
    for (Rank& r : d->ranks) RC(tslam_internal_set_pairs(r.h, (flags & TSLAM_SHARD_PAIRS) ? 1 : 0));
    d->set_flags(flags);
    return TSLAM_OK;
}

int tslam_shard_timing(tslam_handle* h, double* out_us, int n_out) {
    if (!h || !out_us || n_out < 1) return tslam_internal_fail(TSLAM_EINVAL, "bad argument");
    tslam_shard_driver* d = tslam_internal_driver(h);
    Rank* r = d ? rank_of(d, h) : nullptr;
    if (!r) return tslam_internal_fail(TSLAM_ESTATE, "the handle is not driven (tslam_comm_init / tslam_group_create)");
    RC(collect(*r));
    const int64_t nb = r->timed_batches;
    for (int i = 0; i < std::min(n_out, (int)TSLAM_SEG_COUNT); ++i) out_us[i] = nb ? r->seg_us[i] / (double)nb : 0.0;
    for (double& v : r->seg_us) v = 0.0;
    r->timed_batches = 0;
    return (int)nb;
}

struct tslam_group {
    tslam_shard_driver* d = nullptr;
};

int tslam_group_create(tslam_handle* const* handles, int n, int transport, tslam_group** out) {
    if (!handles || n < 1 || !out) return tslam_internal_fail(TSLAM_EINVAL, "bad argument");
    if (transport != TSLAM_TRANSPORT_RCCL && transport != TSLAM_TRANSPORT_COPY)
        return tslam_internal_fail(TSLAM_EINVAL, "transport must be TSLAM_TRANSPORT_RCCL or TSLAM_TRANSPORT_COPY");
    tslam_handle_info in0{};
    RC(tslam_internal_info(handles[0], &in0));
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        tslam_handle_info in{};
        if (!handles[i]) return tslam_internal_fail(TSLAM_EINVAL, "null handle");
        RC(tslam_internal_info(handles[i], &in));
        if (in.C != in0.C || in.P != in0.P || in.B != in0.B || in.W != in0.W || in.H != in0.H || in.rgbd != in0.rgbd ||
            in.rig != in0.rig || in.ba != in0.ba)
            return tslam_internal_fail(TSLAM_EINVAL, "a group's handles must describe the same rig and batch");
        if (tslam_internal_driver(handles[i])) return tslam_internal_fail(TSLAM_ESTATE, "handle already driven");
        devs[i] = in.device;
        for (int j = 0; j < i; ++j)
            if (transport == TSLAM_TRANSPORT_RCCL && devs[j] == devs[i])
                return tslam_internal_fail(TSLAM_EINVAL, "an RCCL group needs one device per handle (COPY allows sharing)");
    }
    auto* d = new tslam_shard_driver();
    int rc = plan(d, handles[0], n);
    d->transport = transport;
    d->ranks.resize(n);
    for (int i = 0; i < n && rc == TSLAM_OK; ++i) {
        d->ranks[i].h = handles[i];
        d->ranks[i].rank = i;
        rc = tslam_set_shard(handles[i], i * d->g.S, (i + 1) * d->g.S, i, n);
        if (rc == TSLAM_OK) rc = setup_rank(d, d->ranks[i]);
    }
    if (rc == TSLAM_OK && transport == TSLAM_TRANSPORT_RCCL) {
        std::vector<ncclComm_t> cx(n), cp(n);
        ncclResult_t nr = ncclCommInitAll(cx.data(), n, devs.data());
        if (nr == ncclSuccess) nr = ncclCommInitAll(cp.data(), n, devs.data());
        if (nr != ncclSuccess) {
            rc = tslam_internal_fail(TSLAM_EHIP, (std::string("ncclCommInitAll: ") + ncclGetErrorString(nr)).c_str());
        } else {
            for (int i = 0; i < n; ++i) {
                d->ranks[i].comm_x = cx[i];
                d->ranks[i].comm_p = cp[i];
            }
        }
    }
    for (int i = 0; i < n && rc == TSLAM_OK; ++i) rc = tslam_internal_attach_driver(handles[i], d, false);
    if (rc != TSLAM_OK) {
        for (int i = 0; i < n; ++i) {
            (void)tslam_internal_attach_driver(handles[i], nullptr, false);
            (void)tslam_set_shard(handles[i], 0, in0.C, 0, 1);
        }
        destroy_driver(d);
        return rc;
    }
    *out = new tslam_group{d};
    return TSLAM_OK;
}

int tslam_group_submit(tslam_group* g, const uint8_t* const* images, int n_frames, void* const* streams) {
    if (!g || !g->d || !images) return tslam_internal_fail(TSLAM_EINVAL, "bad argument");
    for (size_t i = 0; i < g->d->ranks.size(); ++i)
        if (!images[i]) return tslam_internal_fail(TSLAM_EINVAL, "null images");
    return submit(g->d, images, n_frames, streams);
}

int tslam_group_destroy(tslam_group* g) {
    if (!g) return TSLAM_OK;
    if (g->d) {
        const int C = g->d->g.S * g->d->g.world;
        for (Rank& r : g->d->ranks) {
            (void)tslam_internal_attach_driver(r.h, nullptr, false);
            (void)tslam_set_shard(r.h, 0, C, 0, 1);
        }
        destroy_driver(g->d);
    }
    delete g;
    return TSLAM_OK;
}

}  // extern "C"
