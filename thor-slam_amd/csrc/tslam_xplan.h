// tslam_xplan.h — the exchange plan of a sharded rig: the one definition of the
// exchange buffers' slot layout and of who sends what to whom, shared by the driver
// (tslam_shard.cpp, both transports), the pack / import entry points (tslam_api_exchange.cpp) and
// the checker (tests/c/host_check.cpp `schedule`, `make sanitize`).  Host arithmetic only.
//
// A buffer is an array of slots, a slot per peer, sized for a full batch.  A send buffer holds a
// slot per destination (STATE, POSE: one payload), a receive buffer a slot per source.
#pragma once

#include <stddef.h>

#include "tslam_ranges.h"

enum { X_RAW = 0, X_FEAT, X_PAIRB, X_STATE, X_POSE, X_KINDS };   // raw images; stream (RGB-D: pair) blocks; ...
enum { XB_INPUT = 0, XB_PREV, XB_SEND, XB_RECV };   // the batch's input, prev_raw, the kind's send / receive buffer
enum { XC_X = 0, XC_P };                            // communicator: the exchange stream's, the back stream's

struct XGeom {
    int world, S, P, B, n;   // ranks, cameras per rank, pairs, max_batch, this batch's frames
    size_t img, sblk, pblk, rec, st_range, st_cam;   // bytes: image, stream / pair block, pose record, state units
    bool rgbd, pairs, gather;
};
struct XOp {   // one point-to-point operation of a rank
    bool send;
    int peer, comm, buf;   // XC_*, XB_*
    size_t off, bytes;     // in the local buffer
    size_t dst_off;        // send: where it lands in the peer's receive buffer (the copy transport)
};

// The frames rank q's stereo back end solves: its frame range, or under the pair split its pair's
// half of the batch; it reads the other cameras of frames lo - 1 .. hi - 1 (none when empty).
static inline int xp_back_frames(const XGeom& g, int q, int* lo) {
    int hi;
    if (g.pairs) peer_range(q & 1, g.n, 2, lo, &hi);
    else peer_range(q, g.n, g.world, lo, &hi);
    return hi > *lo ? hi - *lo + 1 : 0;
}
// rank q's rig range (rig pose + pose records; under the pair split inside its pair's half)
static inline int xp_rig_range(const XGeom& g, int q, int* lo) {
    int hi;
    peer_range(rig_slot(q, g.world, g.pairs), g.n, g.world, lo, &hi);
    return hi - *lo;
}
// sender q's state payload of an n-frame batch: its range of every pair, its left cameras of every frame
static inline size_t xp_state_bytes(const XGeom& g, int n, int q) {
    int lo, hi;
    peer_range(q, n, g.world, &lo, &hi);
    const int left0 = (q * g.S + 1) & ~1, nleft = (q + 1) * g.S > left0 ? ((q + 1) * g.S - left0 + 1) / 2 : 0;
    return (size_t)(hi - lo) * g.P * g.st_range + (size_t)n * nleft * g.st_cam;
}
static inline size_t xp_pose_bytes(const XGeom& g) { return (size_t)peer_records(g.n, g.world) * g.rec; }   // per rank, padded

// ---- slot layout --------------------------------------------------------------------------------
// frames of a RAW / stereo FEAT slot; under the pair split the partner's half (max_batch / 2 + 1
// frames) takes the whole buffer as its one slot
static inline int xp_slot_frames(const XGeom& g) { return (g.pairs ? g.world : 1) * peer_cap(g.B, g.world); }
static inline size_t xp_slot(const XGeom& g, int kind) {   // bytes of one peer slot
    if (kind == X_RAW) return (size_t)xp_slot_frames(g) * g.S * g.img;
    if (kind == X_FEAT) return g.rgbd ? (size_t)(xp_slot_frames(g) - 1) * g.S * g.pblk : (size_t)xp_slot_frames(g) * g.S * g.sblk;
    if (kind == X_STATE) {
        size_t cap = 0;
        for (int q = 0; q < g.world; ++q) cap = xp_state_bytes(g, g.B, q) > cap ? xp_state_bytes(g, g.B, q) : cap;
        return (cap + 255) / 256 * 256;
    }
    return (size_t)peer_records(g.B, g.world) * (kind == X_PAIRB ? g.pblk : g.rec);
}
// offset of peer q's slot in a rank's send (q = destination) or receive (q = source) buffer
static inline size_t xp_slot_off(const XGeom& g, int kind, int buf, int q) {
    if (kind >= X_STATE && buf == XB_SEND) return 0;                  // one payload, whoever receives it
    if (kind == X_POSE) return (size_t)q * xp_pose_bytes(g);          // the all-gather packs this batch's records
    if (kind <= X_FEAT && g.pairs) return 0;                          // the partner's only
    return (size_t)q * xp_slot(g, kind);
}
static inline size_t xp_buf_bytes(const XGeom& g, int kind, int buf, int rank) {   // what rank allocates
    int slots = kind <= X_FEAT && g.pairs ? 1 : g.world;
    if (kind == X_RAW && (buf == XB_SEND || g.rgbd)) slots = 0;       // sent from the input; no image moves
    if (kind == X_STATE) slots = buf == XB_SEND ? rank != 0 : rank == 0 ? g.world : 0;
    if (kind == X_POSE && buf == XB_SEND) slots = 1;
    return (size_t)slots * xp_slot(g, kind);
}

// ---- schedule -----------------------------------------------------------------------------------
// does exchange `kind` carry data from rank src to rank dst
static inline bool xp_linked(const XGeom& g, int kind, int src, int dst) {
    if (kind == X_POSE) return true;                                  // all-gather: every slot to every rank
    if (src == dst) return false;
    if (kind == X_STATE) return g.gather && dst == 0;
    if (kind == X_PAIRB) return g.pairs && ((src ^ dst) & 1) == 0;    // the ranks of the same half
    if (g.rgbd) return kind == X_FEAT;
    return !g.pairs || dst == (src ^ 1);                              // pair split: the partner only
}
// The sends of rank src to rank dst, in order (at most two), as f(const XOp&).  POSE is the copy
// transport's rendering of the all-gather (RCCL issues ncclAllGather of xp_pose_bytes).
template <class F>
static inline void xp_sends(const XGeom& g, int kind, int src, int dst, F&& f) {
    if (!xp_linked(g, kind, src, dst)) return;
    const int comm = kind <= X_FEAT ? XC_X : XC_P;
    const size_t at = xp_slot_off(g, kind, XB_RECV, src);
    int lo = 0;
    size_t bytes = xp_pose_bytes(g);
    if (kind == X_RAW) bytes = (size_t)xp_back_frames(g, dst, &lo) * g.S * g.img;
    if (kind == X_FEAT) bytes = g.rgbd ? (size_t)xp_rig_range(g, dst, &lo) * g.S * g.pblk : (size_t)xp_back_frames(g, dst, &lo) * g.S * g.sblk;
    if (kind == X_PAIRB) bytes = (size_t)xp_rig_range(g, dst, &lo) * g.pblk;   // one pair's blocks of dst's rig range
    if (kind == X_STATE) bytes = xp_state_bytes(g, g.n, src);
    if (bytes == 0) return;
    if (kind != X_RAW) return f(XOp{true, dst, comm, XB_SEND, xp_slot_off(g, kind, XB_SEND, dst), bytes, at});
    const size_t frame = (size_t)g.S * g.img;
    if (lo > 0) return f(XOp{true, dst, comm, XB_INPUT, (lo - 1) * frame, bytes, at});   // contiguous in the input
    f(XOp{true, dst, comm, XB_PREV, 0, frame, at});   // frame -1: the previous batch's last frame
    f(XOp{true, dst, comm, XB_INPUT, 0, bytes - frame, at + frame});
}
// The point-to-point operations of rank r, in order: per peer its sends, then the receives of
// what the peer sends it (the peer's sends, mirrored).
template <class F>
static inline void xp_ops(const XGeom& g, int kind, int r, F&& f) {
    for (int q = 0; q < g.world; ++q) {
        xp_sends(g, kind, r, q, f);
        xp_sends(g, kind, q, r, [&](const XOp& o) { f(XOp{false, q, o.comm, XB_RECV, o.dst_off, o.bytes, 0}); });
    }
}
