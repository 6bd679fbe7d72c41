// k_match.hip — row A6 of SURVEY.md §8a: brute-force Hamming matching (stereo L<->R with a row
// band and positive disparity; temporal L(t)<->L(t-1) with a window), ratio test, mutual check,
// and the integer-SAD sub-pixel refinements (A6b stereo disparity, A7a temporal position).
// Bit-exact with oracle.match / oracle.stereo_subpixel / oracle.temporal_subpixel.
//
// k_match: the Hamming distances come from the matrix cores.  A block holds 128 y-sorted queries
// of one level, one 32-query MFMA row tile per wave, and matches them on both sides: the setup
// (the query load round, the deal of the queries to the waves, the slot sort, |q|, the A operand
// and the wave's column extent) runs once, then one pass per side, temporal first, each with its
// own early-outs, gate words, train rows, walk, (best, second) reduction, stores and tbest flush;
// the ring, the reduction rows, the merge array and best / second serve one side after the other.
// The queries are dealt by x, so each wave holds an x-quartile: its column box admits about half
// of a temporal window's trains, and on either side it walks the block's rows.  A block that owns
// the stereo side only (the stereo-only launch of a sharded rig, and the split layout of
// tslam_match_layout, one side per block, which the tests compare against) keeps its queries in
// y order and each wave walks its own row band.  Results do not depend on the deal: the query
// side's best and second are order-free minima, the train side's minimum goes by query index.
// Each wave walks the train rows its queries can reach in chunks of 64 y-sorted positions,
// compacts the trains inside its column box into an LDS ring (ballot + mbcnt), and scores every
// full ring tile of 32 trains with four FP4 block-scaled MFMAs:
//   Hamming(q, t) = |q| + sum_k (1 - 2 q_k) t_k
// The query side is +-1 (e2m1 0b0010 / 0b1010), the train side the descriptor bits in place
// (w & (0x11111111 << s): fp4 0.5 / 1 / 2, step 3 shifted to 2), undone by the E8M0 block scales
// 2 / 1 / 0.5 / 0.5, and C starts at |q| of the row — every partial sum is a small integer, so
// the f32 result is the exact distance (tools/mfma_hamming_probe.hip checks the encoding).
// One tile costs 4 MFMAs + ~20 VALU of bit unpacking per lane where the VALU kernel spent 16
// v_xor/v_bcnt per lane and pair; the remaining per-pair VALU is the geometric gate and the
// best / second / mutual bookkeeping (9 ops).
//
// Keys.  A non-negative integer-valued f32 orders like its bits and leaves the low 15 mantissa
// bits zero, so (distance, index) keys are bits(H) | index (index < 8192): the query side's best
// is a v_min, its second a v_med3; an ineligible pair gets +inf bits (0x7F800000), above every
// eligible key.  The train side's (distance, query) minimum for the mutual check uses the wave
// slot (0..31) as the index: a wave's queries take their slots in keypoint-index order, so slot
// order is query order.  Slot 2 * reg + h is MFMA row (reg & 3) + 8 (reg >> 2) + 4 h, i.e. the
// row accumulator register reg of lane half h holds, so the slot's low bit is the lane half (ORed
// in after the register minimum).  It is published in the (distance << 16 | query) format the
// refinement kernels read: the waves of a block first combine their minima in LDS, by the train's
// y-sorted position inside the block's window (ds_min), and after the walk the block sends one
// global atomicMin per touched position; a position past the array's capacity (and every position
// on the direct path, tslam_match_mode) goes to tbest from the wave that found it.  Global atomics
// run at the memory side, one 64-byte request per lane when the addresses scatter: merging removes
// a block's repeats of a train, and tbest is indexed by the train's y-sorted position (koff[l] +
// position), so a block's flush covers one contiguous range.  The query's best-train key keeps the
// keypoint index (the tie-break orders by it); the epilogue looks its position up in ypos (written
// by select beside ys) and stores it beside qbest (qtpos), where the refinement finds tbest's word
// (profiles/match_tbest_probe.txt).
#include "tslam_common.h"

#define TS_MQ 128          // queries per k_match block (4 waves x one 32-row MFMA tile)
#define TS_MRED_PITCH 33   // (best, second) rows of the final per-slot reduction, padded
#define TS_MRING 1024      // compacted trains per walk round (the ring shares the reduction's LDS)
#define TS_MCHUNKS 6       // 64-position chunks whose record loads are in flight together
// tslam_match_counters: per mode (stereo 0..7, temporal 8..15)
#define TS_MCNT_MERGED 0   // train minima merged in LDS
#define TS_MCNT_DIRECT 1   // ... sent straight to tbest (past the merge capacity, or the direct path)
#define TS_MCNT_FLUSHED 2  // global atomics of the blocks' merged positions
#define TS_MCNT_EMPTY 3    // blocks that had nothing to match and wrote "no match"
#define TS_MCNT_WALKED 4   // blocks that matched

typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef float v16f_t __attribute__((ext_vector_type(16)));
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// the geometric gate of one (query row, train column) pair: both 16-bit halves of
// (query gate word - train xy) within the spans (v_pk_sub_u16, v_pk_min_u16, v_cmp)
__device__ __forceinline__ bool gate_ok(uint32_t qgate, uint32_t txy, uint32_t span) {
    const u16x2_t d = __builtin_bit_cast(u16x2_t, qgate) - __builtin_bit_cast(u16x2_t, txy);
    const u16x2_t m = __builtin_elementwise_min(d, __builtin_bit_cast(u16x2_t, span));
    return __builtin_bit_cast(uint32_t, m) == __builtin_bit_cast(uint32_t, d);
}

__device__ __forceinline__ uint32_t key_dist(uint32_t key) {   // distance of a finite key
    return (uint32_t)__uint_as_float(key & 0xFFFF8000u);
}

// CNT: the build that counts its paths for tslam_match_counters (k_match_counted); the shipped
// kernel holds none of that code
template <bool CNT>
__device__ __forceinline__ void match_body(const BatchCtx& c) {
    TS_BACK_PRIO;
    // per wave: the compacted-train ring during the walk, then the (best, second) reduction
    __shared__ __attribute__((aligned(16))) uint2 s_red[4][32 * TS_MRED_PITCH];
    __shared__ __attribute__((aligned(16))) uint32_t s_key[2][TS_MQ];  // the deal by x: (x, thread) sort keys, then the dealt positions
    __shared__ __attribute__((aligned(16))) uint32_t s_wk[4][32];   // per wave: query-index sort keys
    // the block's query records and descriptors (one load round), in the ring's LDS: they are dead
    // once every wave has built its A operand (the barrier before the walk)
    uint4* const s_qrec = reinterpret_cast<uint4*>(&s_red[0][0]);
    uint4* const s_qdesc = s_qrec + TS_MQ;
    __shared__ uint32_t s_sq[4][32];      // per wave slot: query keypoint index (~0: empty slot)
    __shared__ uint32_t s_si[4][32];      // ... its block-local index
    // ... its y << 16 | x, [32 wave + slot], in the deal's sort keys: those are dead after the
    // barrier that publishes the dealt positions
    uint32_t* const s_sxy = s_key[0];
    // ... gate word (qy + gy_tol) << 16 | (qx - gx_lo) and |q| (popcount of the descriptor), by
    // [wave][slot & 1][slot >> 1]: lane half h reads its 16 accumulator rows as four 16-byte words
    __shared__ __attribute__((aligned(16))) uint32_t s_sg[4][2][16];
    __shared__ __attribute__((aligned(16))) float s_spc[4][2][16];
    // The block's train-side minima (distance << 16 | query) by y-sorted train position minus the
    // block's window base: the waves of a block reach the same trains (temporal: the x-quartile
    // boxes overlap 2:1), so they meet here (ds_min) and each touched position leaves the CU as
    // one global atomic after the walk.  TS_MTB fills the 40 KB that keep 4 blocks on a CU.
    __shared__ uint32_t s_tb[TS_MTB];
    // The sides a block owns (bit 0 stereo, bit 1 temporal).  Fused layout (the default): grid
    // (total_qtiles, n * npair), blockIdx.y = f * npair + (p - pair0), and the block matches its
    // tile on every side of c.match_modes.  Split layout (tslam_match_layout, the tests' reference):
    // one side per block, blockIdx.y the temporal blocks of every frame first, then the stereo
    // blocks.  Stereo-only launches (match_modes == 1) have one stereo block per tile either way.
    const int npb = c.n * c.npair;
    const int z = blockIdx.y;
    const int sides = c.match_modes == 1 ? 1 : !c.mp.split ? 3 : z < npb ? 2 : 1;
    const int fl = z < npb ? z : z - npb;     // f * npair + (p - pair0)
    const int f = div_small(fl, c.npair_rcp);
    const int p = c.pair0 + (fl - f * c.npair);
    const int64_t g = c.g0 + f;
    int l = 0;
    while (l + 1 < c.g.n_levels && (int)blockIdx.x >= c.g.qtile_start[l + 1]) ++l;
    const int tile = blockIdx.x - c.g.qtile_start[l];
    const int q0 = tile * TS_MQ;
    const int K = c.g.K;
    const size_t mbase0 = ((size_t)f * c.P + p) * 2 * K;   // the stereo side's words; temporal at + K
    const int slot = batch_slot(c, f);
    const int pslot = prev_slot(c, slot);
    const int qcam = c.cpp * p;
    const int row_tol = c.mp.row_tol, dmax = c.mp.max_disp >> l, win = c.mp.window >> l;
    const int qn = c.kcount[((size_t)slot * c.C + qcam) * c.g.n_levels + l];
    const int tn_s = c.rgbd ? 0 : c.kcount[((size_t)slot * c.C + qcam + 1) * c.g.n_levels + l];
    const int tn_t = c.kcount[((size_t)pslot * c.C + qcam) * c.g.n_levels + l];
    // A side with nothing to match writes "no match" for the tile's positions of the level itself
    // (qbest is not cleared before the launch): no previous frame, RGB-D (depth replaces stereo
    // matching), a tile past the image's count, no train, or an empty disparity range at this
    // level.  All of it is block-uniform; a block whose sides all end here returns before the setup.
    int live = 0;
#pragma unroll
    for (int mode = 0; mode < 2; ++mode) {
        if (!(sides >> mode & 1)) continue;
        const bool dead = q0 >= qn || (mode == 1 ? g == 0 || tn_t == 0 : c.rgbd || tn_s == 0 || dmax < 1);
        if (!dead) {
            live |= 1 << mode;
        } else if ((int)threadIdx.x < TS_MQ && q0 + (int)threadIdx.x < c.g.Kq[l]) {
            c.qbest[mbase0 + (size_t)mode * K + c.g.koff[l] + q0 + threadIdx.x] = 0xFFFFFFFFu;
        }
        if (CNT && threadIdx.x == 0) atomicAdd(&c.match_cnt[8 * mode + (dead ? TS_MCNT_EMPTY : TS_MCNT_WALKED)], 1u);
    }
    if (!live) return;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ci = lane & 31, h = lane >> 5;  // MFMA column / row index, lane half (k half)
    const size_t qbase = ((size_t)slot * c.C + qcam) * K;
    const uint4* qys = c.ys + qbase + c.g.koff[l];           // y-sorted records of the level
    const uint4* qdesc = reinterpret_cast<const uint4*>(c.desc_ys + (qbase + c.g.koff[l]) * 8);
    const int Hl = c.g.H[l];
    const uint32_t mcap = (uint32_t)min(c.mp.merge_cap, TS_MTB);

    // ---- the setup, once per block ----
    // The block's 128 query records and descriptors land in LDS in one round of global loads, so
    // every later setup step reads LDS; the records are y-sorted, so the train rows of every side
    // (and the row-start loads for them) are known at once.
    const int nq = min(TS_MQ, qn - q0);
    {
        const int t = threadIdx.x & (TS_MQ - 1), half = threadIdx.x >> 7;
        const int pos = q0 + min(t, nq - 1);   // past nq: a clamped duplicate, never active
        if (half == 0) s_qrec[t] = qys[pos];
        s_qdesc[2 * t + half] = qdesc[2 * pos + half];
    }
    __syncthreads();
    // this wave's 32 queries (block-local indices): the block's x-ranks 32 wave .. 32 wave + 31
    // where the block owns the temporal side (either side then walks the block's rows), or
    // 32 wave + i in y order (a stereo-only block: the wave walks its own row band); active ones
    // come first in either order
    const bool dealx = (sides & 2) != 0;
    const bool wave_active = 32 * wave < nq;
    // rows of the block's queries, and of the wave's: uniform, they index the sides' row starts
    const int by0 = __builtin_amdgcn_readfirstlane((int)(s_qrec[0].x >> 16));
    const int by1 = __builtin_amdgcn_readfirstlane((int)(s_qrec[nq - 1].x >> 16));
    const int wy0 = dealx ? by0 : __builtin_amdgcn_readfirstlane((int)(s_qrec[min(32 * wave, nq - 1)].x >> 16));
    const int wy1 = dealx ? by1 : __builtin_amdgcn_readfirstlane((int)(s_qrec[min(32 * wave + 31, nq - 1)].x >> 16));
    int bi = 32 * wave + ci;
    if (dealx) {
        if (threadIdx.x < TS_MQ) {
            const int t = threadIdx.x;
            s_key[0][t] = t < nq ? (s_qrec[t].x & 0xFFFF) << 8 | (uint32_t)t : 0x1000000u | (uint32_t)t;
        }
        __syncthreads();
        if (threadIdx.x < TS_MQ) {
            const uint32_t key = s_key[0][threadIdx.x];
            int rank = 0;
            const uint4* k4 = reinterpret_cast<const uint4*>(s_key[0]);
#pragma unroll 4
            for (int i = 0; i < TS_MQ / 4; ++i) {
                const uint4 v = k4[i];
                rank += (v.x < key) + (v.y < key) + (v.z < key) + (v.w < key);
            }
            s_key[1][rank] = threadIdx.x;   // keys are distinct: a permutation
        }
        __syncthreads();
        bi = (int)s_key[1][32 * wave + ci];
    }
    const bool active = bi < nq;
    int qx = 0, qy = 0;
    uint32_t qi = 0, pc = 0;
    if (active) {
        const uint4 rec = s_qrec[bi];
        const uint4 d = s_qdesc[2 * bi + h];
        qi = rec.z;
        qx = rec.x & 0xFFFF;
        qy = rec.x >> 16;
        pc = __popc(d.x) + __popc(d.y) + __popc(d.z) + __popc(d.w);
    }
    pc += (uint32_t)__shfl_xor((int)pc, 32, 64);
    // slots in query-index order (the mutual check's tie-break): rank among the wave's 32
    if (h == 0) s_wk[wave][ci] = active ? qi : 0x10000u | (uint32_t)ci;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    {
        const uint32_t key = active ? qi : 0x10000u | (uint32_t)ci;
        int rank = 0;
        const uint4* k4 = reinterpret_cast<const uint4*>(s_wk[wave]);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 v = k4[i];
            rank += (v.x < key) + (v.y < key) + (v.z < key) + (v.w < key);
        }
        if (h == 0) {
            s_sq[wave][rank] = active ? qi : 0xFFFFFFFFu;
            s_si[wave][rank] = (uint32_t)bi;
            s_sxy[32 * wave + rank] = (uint32_t)qy << 16 | (uint32_t)qx;   // the sides' gate words come from it
            s_spc[wave][rank & 1][rank >> 1] = (float)pc;
        }
    }
    // the columns of this wave's queries
    int wx0, wx1;
    {
        int ax = active ? qx : (1 << 20), bx = active ? qx : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ax = min(ax, __shfl_xor(ax, o, 64));
            bx = max(bx, __shfl_xor(bx, o, 64));
        }
        wx0 = __builtin_amdgcn_readfirstlane(ax);   // equal in every lane: make it provably uniform
        wx1 = __builtin_amdgcn_readfirstlane(bx);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // A operand (rows = slots): lane (row ci, half h) holds, for MFMA step s, bit s of every nibble
    // of descriptor words 4h .. 4h+3 of the query in slot(ci), as +-1
    uint32_t qa[4][4];
    {
        const int srow = 2 * ((ci & 3) + 4 * (ci >> 3)) + ((ci >> 2) & 1);
        uint4 d = {0u, 0u, 0u, 0u};
        if (s_sq[wave][srow] != 0xFFFFFFFFu) d = s_qdesc[2 * (int)s_si[wave][srow] + h];
        const uint32_t w4[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) qa[s][j] = 0x22222222u | (((w4[j] >> s) & 0x11111111u) << 3);
    }
    // per accumulator register: the slot's |q| (the MFMA's C) and gate word, re-read from LDS per
    // tile (32 VGPRs fewer across the walk: 4 waves per SIMD instead of 3)
    const float4* const spc4 = reinterpret_cast<const float4*>(s_spc[wave][h]);
    const uint4* const sg4 = reinterpret_cast<const uint4*>(s_sg[wave][h]);

    // ---- the pass of one side: temporal (the heavy one) first ----
    // The ring, the reduction rows, the merge array and best / second serve one side after the other.
    bool first = true;
    for (int mode = 1; mode >= 0; --mode) {
        if (!(live >> mode & 1)) continue;
        // the previous side's flush has read the merge array before this side clears it
        if (!first) __syncthreads();
        first = false;
        const size_t mbase = mbase0 + (size_t)mode * K;
        const int tslot = mode == 0 ? slot : pslot;
        const int tcam = mode == 0 ? qcam + 1 : qcam;
        const size_t tbase = ((size_t)tslot * c.C + tcam) * K;
        const uint4* tys = c.ys + tbase + c.g.koff[l];
        uint32_t* const tb = c.tbest + mbase + c.g.koff[l];   // the level's train minima, by y-sorted position
        const uint4* tdesc = reinterpret_cast<const uint4*>(c.desc_ys + (tbase + c.g.koff[l]) * 8);
        const uint16_t* trs = c.rowstart + ((size_t)tslot * c.C + tcam) * c.g.rs_total + c.g.rs_off[l];
        // the geometric gate as one box: stereo 1 <= x_q - x_t <= max_disp and |y_q - y_t| <= row_tol;
        // temporal |x_q - x_t| <= window and |y_q - y_t| <= window
        const int gx_lo = mode == 0 ? 1 : -win, gx_hi = mode == 0 ? dmax : win, gy_tol = mode == 0 ? row_tol : win;
        const uint32_t span = (uint32_t)(2 * gy_tol) << 16 | (uint32_t)(gx_hi - gx_lo);
        // train rows: the block's (the base and extent of the merge array) and the wave's, which are
        // the block's too where the queries are dealt by x (an x-quartile spans the block's rows)
        const int bt0 = (int)trs[max(0, by0 - gy_tol)], bt1 = (int)trs[min(Hl - 1, by1 + gy_tol) + 1];
        int wt0 = 0, wt1 = 0;
        if (wave_active) {
            wt0 = dealx ? bt0 : (int)trs[max(0, wy0 - gy_tol)];
            wt1 = dealx ? bt1 : (int)trs[min(Hl - 1, wy1 + gy_tol) + 1];
        }
        for (int i = threadIdx.x; i < min((int)mcap, bt1 - bt0); i += 256) s_tb[i] = 0xFFFFFFFFu;
        // the slots' gate words; inactive: 0xFFFF halves fail every gate
        if (h == 0) {
            const uint32_t xy = s_sxy[32 * wave + ci];
            s_sg[wave][ci & 1][ci >> 1] = s_sq[wave][ci] != 0xFFFFFFFFu
                ? ((xy >> 16) + (uint32_t)gy_tol) << 16 | ((xy - (uint32_t)gx_lo) & 0xFFFFu) : 0xFFFFFFFFu;
        }
        // a train column some query of the wave can reach: qx - tx in [gx_lo, gx_hi] for a wave qx
        const uint32_t bx0 = (uint32_t)(wx0 - gx_hi), bx_span = (uint32_t)(wx1 - gx_lo - (wx0 - gx_hi));
        // every wave's A operand is built (s_qrec / s_qdesc become ring space), the merge array is clear
        __syncthreads();
        uint32_t best[16], second[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) best[r] = second[r] = 0xFFFFFFFFu;

        // The walk in rounds: compact the trains inside the wave's column box into the ring (chunks of
        // 64 y-sorted positions, TS_MCHUNKS chunks' record loads in flight at a time) until it holds
        // TS_MRING - 64 TS_MCHUNKS or more (every round but a rare last one: all of them), then score
        // the ring's 32-train tiles, each tile's entries and descriptors loaded one tile ahead (two
        // tiles per loop trip measured slower: 173 VGPRs, 2 waves/SIMD).
        // Every load is unconditional (indices clamped into the ring; a padding column only gets the
        // gate-failing xy) and the train-side minima go back into the ring entries (the flush's global
        // atomics come after the round's last tile), so the loop body is straight-line code whose
        // vmcnt waits cover exactly the tile being scored.
        uint2* ring = s_red[wave];   // {txy, tidx << 16 | position}; after scoring {tmin, ...}
        auto score = [&](const uint4& d, const uint2& e, uint32_t k, uint32_t n) {
            const uint32_t w4[4] = {d.x, d.y, d.z, d.w};
            v16f_t acc;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 v = spc4[i];
                acc[4 * i] = v.x;
                acc[4 * i + 1] = v.y;
                acc[4 * i + 2] = v.z;
                acc[4 * i + 3] = v.w;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                v8i_t a, b;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = (int)qa[s][j];
                    b[j] = (int)(s < 3 ? (w4[j] & (0x11111111u << s)) : ((w4[j] >> 1) & 0x44444444u));
                    a[j + 4] = 0;
                    b[j + 4] = 0;
                }
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 4, 4, 0, 127, 0, s == 0 ? 128 : s == 1 ? 127 : 126);
                // b stays live past the MFMA, so the destination never lands on it: the compiler does
                // not keep vdst of the block-scaled MFMA apart from its sources (no early-clobber), and
                // a build that spilled put vdst over srcA and half of srcC — wrong stereo matches
                // (DESIGN.md §5).  isa_guard.py checks every build's MFMA operands.
                asm volatile("" ::"v"(b));
            }
            const uint32_t txy = k < n ? e.x : 0x80008000u;   // padding fails every gate
            const uint32_t tidx = e.y >> 16;
            uint32_t tmin = 0xFFFFFFFFu;
            uint32_t qgate[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 v = sg4[i];
                qgate[4 * i] = v.x;
                qgate[4 * i + 1] = v.y;
                qgate[4 * i + 2] = v.z;
                qgate[4 * i + 3] = v.w;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t hb = gate_ok(qgate[r], txy, span) ? __float_as_uint(acc[r]) : 0x7F800000u;
                const uint32_t key = hb | tidx;
                second[r] = med3_u32(best[r], second[r], key);   // = min(second, max(best, key)): best <= second
                best[r] = min(best[r], key);
                tmin = min(tmin, hb | (uint32_t)(2 * r));
            }
            tmin |= (uint32_t)h;
            tmin = min(tmin, (uint32_t)__shfl_xor((int)tmin, 32, 64));
            if (h == 0 && k < n) ring[k].x = tmin;
        };
        for (int jt = wt0; jt < wt1;) {
            uint32_t n = 0;
            for (; jt < wt1 && n <= TS_MRING - 64 * TS_MCHUNKS; jt += 64 * TS_MCHUNKS) {
                uint4 r4[TS_MCHUNKS];
#pragma unroll
                for (int u = 0; u < TS_MCHUNKS; ++u) r4[u] = tys[min(jt + 64 * u + lane, wt1 - 1)];
#pragma unroll
                for (int u = 0; u < TS_MCHUNKS; ++u) {
                    const int j = jt + 64 * u + lane;
                    const bool inbox = j < wt1 && (uint32_t)((int)(r4[u].x & 0xFFFF) - (int)bx0) <= bx_span;
                    const uint64_t m = __ballot(inbox);
                    if (inbox)
                        ring[n + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] =
                            uint2{r4[u].x, r4[u].z << 16 | (uint32_t)j};
                    n += (uint32_t)__popcll(m);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (n > 0) {
                const uint32_t last = n - 1;
                uint2 e0 = ring[min((uint32_t)ci, last)];
                uint4 d0 = tdesc[2 * (int)(e0.y & 0xFFFFu) + h];
                for (uint32_t k = (uint32_t)ci; k - (uint32_t)ci < n; k += 32u) {
                    const uint2 e1 = ring[min(k + 32u, last)];
                    const uint4 d1 = tdesc[2 * (int)(e1.y & 0xFFFFu) + h];
                    score(d0, e0, k, n);
                    e0 = e1;
                    d0 = d1;
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // flush: each train's (distance, query) minimum over the wave's queries, into the block's
                // merge array or, past its capacity, straight into tbest (both by position)
                for (uint32_t k = (uint32_t)lane; k < n; k += 64) {
                    const uint2 e = ring[k];
                    const bool hit = e.x < 0x7F800000u;
                    const uint32_t rel = (e.y & 0xFFFFu) - (uint32_t)bt0;
                    if (hit) {
                        const uint32_t v = key_dist(e.x & ~31u) << 16 | s_sq[wave][e.x & 31u];
                        if (rel < mcap)
                            atomicMin(&s_tb[rel], v);
                        else
                            atomicMin(&tb[e.y & 0xFFFFu], v);
                    }
                    if (CNT) {
                        const uint32_t nm = (uint32_t)__popcll(__ballot(hit && rel < mcap)), nd = (uint32_t)__popcll(__ballot(hit && rel >= mcap));
                        if (lane == 0 && nm) atomicAdd(&c.match_cnt[8 * mode + TS_MCNT_MERGED], nm);
                        if (lane == 0 && nd) atomicAdd(&c.match_cnt[8 * mode + TS_MCNT_DIRECT], nd);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the ring is refilled by the next round
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }

        // per slot: merge the 32 columns' (best, second) — best = min, second = min(s1, s2, max(b1, b2))
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint2* red = s_red[wave];
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(2 * r + h) * TS_MRED_PITCH + ci] = uint2{best[r], second[r]};
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t b = 0xFFFFFFFFu, s2 = 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint2 v = red[ci * TS_MRED_PITCH + 16 * h + i];
            s2 = min(min(s2, v.y), max(b, v.x));
            b = min(b, v.x);
        }
        {
            const uint32_t ob = (uint32_t)__shfl_xor((int)b, 32, 64), os = (uint32_t)__shfl_xor((int)s2, 32, 64);
            s2 = min(min(s2, os), max(b, ob));
            b = min(b, ob);
        }
        // stored by the query's y-sorted position (the refinement kernels load them beside its record)
        // An empty slot stands for a position past the image's count: inside the level it gets the "no
        // match" word (no memset of qbest: every position of a level is some block's to write).
        const uint32_t qk = s_sq[wave][ci];
        const int qpos = q0 + (int)s_si[wave][ci];
        if (h == 0 && qpos < c.g.Kq[l]) {
            const size_t qp = mbase + c.g.koff[l] + qpos;
            const bool found = qk != 0xFFFFFFFFu && b < 0x7F800000u;
            c.qbest[qp] = found ? key_dist(b) << 16 | (b & 0x7FFFu) : 0xFFFFFFFFu;
            if (qk != 0xFFFFFFFFu) c.qsecond[qp] = s2 < 0x7F800000u ? key_dist(s2) : 256u;
            // where the best train's tbest word lies (the key carries its keypoint index: the tie-break
            // orders by index); one gather per wave, so the refinement loads tbest in its second round
            c.qtpos[qp] = found ? c.ypos[tbase + (b & 0x7FFFu)] : (uint16_t)0;
        }
        // the block's merged train minima: one global atomic per position that any wave touched
        if (mcap) {
            __syncthreads();
            const int len = min((int)mcap, bt1 - bt0);
            uint32_t na = 0;
            for (int i = threadIdx.x; i < len; i += 256) {
                const uint32_t v = s_tb[i];
                if (v != 0xFFFFFFFFu) {
                    atomicMin(&tb[bt0 + i], v);   // a contiguous range of tbest
                    ++na;
                }
            }
            if (CNT && na) atomicAdd(&c.match_cnt[8 * mode + TS_MCNT_FLUSHED], na);
        }
    }   // the side
}

// Sub-pixel offset of a discrete minimum from three integer costs (exact double division).
__device__ __forceinline__ double parabola(int sm, int s0, int sp) {
    const int den = sm - 2 * s0 + sp;
    return den > 0 ? (double)(sm - sp) / (2.0 * (double)den) : 0.0;
}

// The 11 bytes of row `y` starting at column `x0` as three dwords (byte 12 zeroed), from aligned
// dword loads + v_alignbyte (any alignment of the level base, row pitch and x0).
__device__ __forceinline__ void row11(const uint8_t* img, int W, int y, int x0, uint32_t* w) {
    const uint8_t* a = img + (size_t)y * W + x0;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3u);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a - sh);   // pointer arithmetic keeps global loads
    const uint32_t d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3];
    w[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
    w[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    w[2] = __builtin_amdgcn_alignbyte(d3, d2, sh) & 0x00FFFFFFu;
}

// One staged LDS row (16 bytes): the 11 patch bytes of row `y` from column `x0`, the rest zero ...
__device__ __forceinline__ uint4 stage_row11(const uint8_t* img, int W, int y, int x0) {
    uint32_t w3[3];
    row11(img, W, y, x0, w3);
    return uint4{w3[0], w3[1], w3[2], 0u};
}

// ... or the 15 window bytes (byte 15 zero): 5 aligned dwords `d` + v_alignbyte by the address's low bits.
// A row that starts in byte 0 or 1 of its first dword ends inside the fourth: its lane skips the fifth load
// (the refinement is bound by its address path; one unaligned 16-byte load per row instead was as fast
// alone and 0.07 ms slower in the pipelined C2 step)
__device__ __forceinline__ uint4 align_row15(const uint32_t* d, uint32_t sh) {
    return uint4{__builtin_amdgcn_alignbyte(d[1], d[0], sh), __builtin_amdgcn_alignbyte(d[2], d[1], sh),
                 __builtin_amdgcn_alignbyte(d[3], d[2], sh), __builtin_amdgcn_alignbyte(d[4], d[3], sh) & 0x00FFFFFFu};
}
__device__ __forceinline__ uint4 stage_row15(const uint8_t* img, int W, int y, int x0) {
    const uint8_t* a = img + (size_t)y * W + x0;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - sh);
    const uint32_t d[5] = {q[0], q[1], q[2], q[3], sh >= 2u ? q[4] : 0u};
    return align_row15(d, sh);
}

// Bytes kx .. kx+10 (kx = 0..4) of a staged 15-byte row as three dwords (byte 12 zeroed).
// kx == 4: start one word later with no byte shift (the 4th word is then unused)
__device__ __forceinline__ void shift_row11(const uint4* row, int kx, uint32_t* w) {
    const uint32_t* wb = reinterpret_cast<const uint32_t*>(row);
    const int kh = kx >> 2;
    const uint32_t sh = (uint32_t)(kx & 3);
    const uint32_t d0 = wb[kh], d1 = wb[kh + 1], d2 = wb[kh + 2], d3 = wb[3 - kh];
    w[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
    w[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
    w[2] = __builtin_amdgcn_alignbyte(d3, d2, sh) & 0x00FFFFFFu;
}

__device__ __forceinline__ uint32_t sad_row11(const uint32_t* a, const uint32_t* w, uint32_t s) {
    s = __builtin_amdgcn_sad_u8(a[0], w[0], s);
    s = __builtin_amdgcn_sad_u8(a[1], w[1], s);
    return __builtin_amdgcn_sad_u8(a[2], w[2], s);
}

// Stereo SAD of one offset: the 11x11 left patch against bytes kx .. kx+10 of the 11 staged right
// window rows (right patch centred at xr + kx - 2).  The left rows are staged patch rows (ASH < 0)
// or rows of the staged 15x15 temporal window, whose bytes ASH .. ASH+10 are the patch row.
template <int ASH>
__device__ __forceinline__ uint32_t stereo_sad(const uint4* a, const uint4* b, int kx) {
    uint32_t s = 0;
#pragma unroll
    for (int dy = 0; dy < 11; ++dy) {
        uint32_t la[3], w[3];
        if (ASH < 0) {
            const uint4 ra = a[dy];
            la[0] = ra.x, la[1] = ra.y, la[2] = ra.z;
        } else {
            shift_row11(a + dy, ASH, la);
        }
        shift_row11(b + dy, kx, w);
        s = sad_row11(la, w, s);
    }
    return s;
}

// The stereo result of one live query: match j (or -1) and, from the 5 costs and the first
// minimum ks, the disparity (NaN: rejected, minimum at the range's edge, or not positive).
__device__ __forceinline__ void stereo_store(const BatchCtx& c, size_t out, int j, int l, int qx, int xr, int ks,
                                             const int* cost) {
    double d0 = __builtin_nan("");
    if (j >= 0 && ks > 0 && ks < 4) {
        const double delta = parabola(cost[ks - 1], cost[ks], cost[ks + 1]);
        const double sc = (double)(1 << l);
        const double v = ((double)qx - ((double)(xr + (ks - TS_SAD_RANGE)) + delta)) * sc;
        if (v > 0.0) d0 = v;
    }
    c.stereo[out] = j;
    c.disp[out] = d0;
}

// Temporal SAD of the 5 offsets (kx, ky = 0..4) of column shift kx: each of the 15 staged window
// rows `b` is realigned once (its 11 bytes from kx on) and serves every ky it meets (patch row
// dy = r - ky of `a`); the sums are integers, so the costs equal a per-offset loop's
#define TS_RT_AROWS 11
#define TS_RT_BROWS 15
__device__ __forceinline__ void temporal_sad(const uint4* a, const uint4* b, int kx, uint32_t* s) {
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) s[ky] = 0u;
#pragma unroll
    for (int r = 0; r < TS_RT_BROWS; ++r) {
        uint32_t w[3];
        shift_row11(b + r, kx, w);
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
            const int dy = r - ky;
            if (dy < 0 || dy >= TS_RT_AROWS) continue;   // compile-time
            const uint4 ra = a[dy];
            const uint32_t la[3] = {ra.x, ra.y, ra.z};
            s[ky] = sad_row11(la, w, s[ky]);
        }
    }
}

// The temporal result of one live query from the 25 costs and the first minimum `a` (ky * 5 + kx):
// (u, v) at t in level-0 pixels, NaN when rejected or the minimum lies on the search border.
__device__ __forceinline__ void temporal_store(double* out_uv, int j, int l, int qx, int qy, int a, const int* cq) {
    double u = __builtin_nan(""), v = u;
    if (j >= 0) {
        const int c0 = cq[a];
        const int cl = cq[max(a - 1, 0)], cr = cq[min(a + 1, 24)];
        const int cu = cq[max(a - 5, 0)], cd = cq[min(a + 5, 24)];
        const int ky = a / 5, kx = a % 5;
        if (kx > 0 && kx < 4 && ky > 0 && ky < 4) {
            const double ddx = parabola(cl, c0, cr);
            const double ddy = parabola(cu, c0, cd);
            const double sc = (double)(1 << l);
            u = (((double)(qx + (kx - TS_SAD_RANGE)) + ddx) + 0.5) * sc - 0.5;
            v = (((double)(qy + (ky - TS_SAD_RANGE)) + ddy) + 0.5) * sc - 0.5;
        }
    }
    out_uv[0] = u;
    out_uv[1] = v;
}

// The match of the query at y-sorted position `pos` (keypoint qi): k_match stores (qbest, qsecond)
// by position, so they load beside the query's record, and the train side's best query and the
// train's keypoint word {x | y << 16} (image base tkb) load together once the best train j is
// known — two dependent rounds instead of three.  Returns j when the match passes max distance,
// ratio and the mutual check (and `ok`), else -1.
// The lookup comes in its two load rounds and the test (k_refine_pair issues each round for both
// modes at once); the test's terms are all evaluated (&, not &&), so that no load sinks into a
// branch behind another load's wait.
struct MatchRef {
    uint32_t qb, sd, tb;
    int j, tp;
};
__device__ __forceinline__ void match_query(const BatchCtx& c, size_t mbase, int pos, MatchRef* m) {
    m->qb = c.qbest[mbase + pos];
    m->sd = c.qsecond[mbase + pos];
    m->tp = c.qtpos[mbase + pos];   // < K always: a position, or 0 beside "no match"
    m->j = m->qb == 0xFFFFFFFFu ? 0 : (int)(m->qb & 0xFFFF);
}
__device__ __forceinline__ void match_train(const BatchCtx& c, size_t mbase, size_t tkb, MatchRef* m, uint32_t* tkp) {
    m->tb = c.tbest[mbase + m->tp];
    *tkp = c.kps[(tkb + m->j) * 2];
}
__device__ __forceinline__ int match_accept(const BatchCtx& c, const MatchRef& m, int qi, bool ok) {
    const int bd = (int)(m.qb >> 16);
    return ((int)ok & (int)(m.qb != 0xFFFFFFFFu) & (int)(bd <= c.mp.max_hamming) &
            (int)(bd * 100 < c.mp.ratio_pct * (int)m.sd) & (int)((int)(m.tb & 0xFFFF) == qi)) ? m.j : -1;
}
__device__ __forceinline__ int match_lookup(const BatchCtx& c, size_t mbase, int pos, int qi, bool ok, size_t tkb,
                                            uint32_t* tkp) {
    MatchRef m;
    match_query(c, mbase, pos, &m);
    match_train(c, mbase, tkb, &m, tkp);
    return match_accept(c, m, qi, ok);
}

// Stereo refinement (A6b): validity + disparity by 5-offset SAD + parabola.  Eight queries per
// wave, 8 lanes each (lane = query slot * 8 + sub), as the temporal refinement: the query's 11x11
// left patch and the 15x11 right window (offsets -2..+2 around the matched x) are staged in LDS,
// 22 rows dealt over the 8 lanes, so a query costs ~27 row loads instead of 5 x 88 scattered
// dword gathers (the texture-address path, not the VALU, bound the per-lane version); sub-lanes
// 0..4 score the 5 offsets from LDS; the first minimum is an xor-shuffle over the 8 lanes.
// grid xcd_grid3(n*P, ceil(K/32)), block 256.
#define TS_RS_QPB 32   // queries per block
__global__ __launch_bounds__(256) void k_refine_stereo(BatchCtx c) {
    TS_BACK_PRIO;
    __shared__ uint4 s_a[TS_RS_QPB][11];   // left patch rows: 11 bytes used
    __shared__ uint4 s_b[TS_RS_QPB][11];   // right window rows: 15 bytes used
    __shared__ int s_cost[TS_RS_QPB][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = c.g.K;
    int z, local;
    if (!xcd_image_block3(c.n * c.npair, (K + TS_RS_QPB - 1) / TS_RS_QPB, &z, &local)) return;
    const int f = div_small(z, c.npair_rcp), p = c.pair0 + (z - f * c.npair);
    const int slot = batch_slot(c, f);
    const int sub = lane & 7;
    const int qslot = wave * 8 + (lane >> 3);
    const int pos = local * TS_RS_QPB + qslot;
    const bool live = pos < K;
    const size_t mbase = (((size_t)f * c.P + p) * 2 + 0) * K;
    const int qcam = c.cpp * p;
    const size_t qkb = ((size_t)slot * c.C + qcam) * K;
    int l = 0, qi = 0, j = -1;
    uint32_t qxy = 0, tkp = 0;
    if (live) {
        const uint4 rec = c.ys[qkb + pos];
        qi = (int)rec.z;
        l = (int)(rec.y & 0xFFu);
        qxy = rec.x;
        j = match_lookup(c, mbase, pos, qi, rec.w != 0, ((size_t)slot * c.C + qcam + 1) * K, &tkp);
    }
    int qx = 0, xr = 0;
    if (j >= 0) {
        const int W = c.g.W[l];
        qx = qxy & 0xFFFF;
        const int qy = qxy >> 16;
        xr = tkp & 0xFFFF;
        const uint8_t* Lp = c.pyr + ((size_t)slot * c.C + qcam) * c.g.pyr_bytes + c.g.pyr_off[l];
        const uint8_t* Rp = c.pyr + ((size_t)slot * c.C + qcam + 1) * c.g.pyr_bytes + c.g.pyr_off[l];
        for (int hl = sub; hl < 22; hl += 8) {
            if (hl < 11)
                s_a[qslot][hl] = stage_row11(Lp, W, qy - TS_SAD_HALF + hl, qx - TS_SAD_HALF);
            else
                s_b[qslot][hl - 11] = stage_row15(Rp, W, qy - TS_SAD_HALF + hl - 11, xr - TS_SAD_HALF - TS_SAD_RANGE);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // staged rows before the reads (own wave)
    uint32_t key = 0xFFFFFFFFu;
    if (j >= 0 && sub < 5) {
        const uint32_t s = stereo_sad<-1>(s_a[qslot], s_b[qslot], sub);
        s_cost[qslot][sub] = (int)s;
        key = (s << 5) | (uint32_t)sub;
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, m, 64));
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // costs of the 5 lanes before the reads
    if (live && sub == 0) stereo_store(c, ((size_t)slot * c.P + p) * K + qi, j, l, qx, xr, (int)(key & 31u), s_cost[qslot]);
}

// Temporal refinement (A7a): validity + position by 5x5 SAD search + 2-D parabola.  Eight queries
// per wave, 8 lanes each (lane = query slot * 8 + sub), so the dependent chain of loads (record ->
// match validity -> previous keypoint -> image rows) is paid once per 8 queries, not per 2.  The
// query's 11x11 patch at t-1 and its 15x15 search window at t are staged in LDS (sub-lane s loads
// rows s, s+8, .. of the 26), rows padded to 16 bytes and read back as ds_read_b128; sub-lane s
// scores offsets s, s+8, s+16, s+24 of the 25; the first minimum is an xor-shuffle over the 8
// lanes.  grid xcd_grid3(n*P, ceil(K/32)), block 256.
#define TS_RT_QPB 32   // queries per block
__global__ __launch_bounds__(256) void k_refine_temporal(BatchCtx c) {
    TS_BACK_PRIO;
    __shared__ uint4 s_a[TS_RT_QPB][TS_RT_AROWS];   // [query slot][row]: 11 bytes used (+ zero pad)
    __shared__ uint4 s_b[TS_RT_QPB][TS_RT_BROWS];   // 15 bytes used
    __shared__ int s_cost[TS_RT_QPB][25];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = c.g.K;
    int z, local;
    if (!xcd_image_block3(c.n * c.npair, (K + TS_RT_QPB - 1) / TS_RT_QPB, &z, &local)) return;
    const int f = div_small(z, c.npair_rcp), p = c.pair0 + (z - f * c.npair);
    const bool has_prev = c.g0 + f > 0;   // frame 0 of the sequence: nothing matches
    const int slot = batch_slot(c, f);
    const int sub = lane & 7;
    const int qslot = wave * 8 + (lane >> 3);
    const int pos = local * TS_RT_QPB + qslot;
    const bool live = pos < K;
    const size_t mbase = (((size_t)f * c.P + p) * 2 + 1) * K;
    const int qcam = c.cpp * p;
    const size_t qkb = ((size_t)slot * c.C + qcam) * K;
    int l = 0, qi = 0, j = -1;
    uint32_t qxy = 0, pxy = 0;
    const int pslot = has_prev ? prev_slot(c, slot) : slot;
    if (live) {
        const uint4 rec = c.ys[qkb + pos];
        qi = (int)rec.z;
        l = (int)(rec.y & 0xFFu);
        qxy = rec.x;
        j = match_lookup(c, mbase, pos, qi, rec.w != 0 && has_prev, ((size_t)pslot * c.C + qcam) * K, &pxy);
    }
    int32_t* out_idx = c.temporal + ((size_t)slot * c.P + p) * K;
    double* out_uv = c.tuv + (((size_t)f * c.P + p) * K + qi) * 2;
    if (live && sub == 0) out_idx[qi] = j;
    int qx = 0, qy = 0;
    if (j >= 0) {
        const int W = c.g.W[l];
        qx = qxy & 0xFFFF;
        qy = qxy >> 16;
        const int px = pxy & 0xFFFF, py = pxy >> 16;
        const uint8_t* A = c.pyr + ((size_t)pslot * c.C + qcam) * c.g.pyr_bytes + c.g.pyr_off[l];
        const uint8_t* B = c.pyr + ((size_t)slot * c.C + qcam) * c.g.pyr_bytes + c.g.pyr_off[l];
        // stage: rows 0..10 the patch (3 dwords via row11), rows 11..25 the window (15 bytes from
        // 5 aligned dwords + alignbyte); row r by sub-lane r % 8
        for (int hl = sub; hl < TS_RT_AROWS + TS_RT_BROWS; hl += 8) {
            if (hl < TS_RT_AROWS)
                s_a[qslot][hl] = stage_row11(A, W, py - TS_SAD_HALF + hl, px - TS_SAD_HALF);
            else
                s_b[qslot][hl - TS_RT_AROWS] = stage_row15(B, W, qy - TS_SAD_HALF - TS_SAD_RANGE + hl - TS_RT_AROWS,
                                                           qx - TS_SAD_HALF - TS_SAD_RANGE);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // staged rows before the reads (own wave)
    // sub-lane kx < 5 scores the 5 offsets (kx, ky = 0..4) of its column shift
    uint32_t key = 0xFFFFFFFFu;   // first minimum of (cost << 5 | offset) over this lane's offsets
    if (j >= 0 && sub < 5) {
        uint32_t s[5];
        temporal_sad(s_a[qslot], s_b[qslot], sub, s);
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
            const int o = ky * 5 + sub;
            s_cost[qslot][o] = (int)s[ky];
            key = min(key, (s[ky] << 5) | (uint32_t)o);
        }
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, m, 64));
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // costs of the 8 lanes before the reads
    if (live && sub == 0) temporal_store(out_uv, j, l, qx, qy, (int)(key & 31u), s_cost[qslot]);
}

// Both refinements of a stereo frame in one pass over the left queries (the stereo rig's default:
// launch_match_refine).  The two kernels above share the query's record, walk the same kind of
// lookup chain and gather overlapping pixels: the stereo kernel's 11x11 left patch is rows 2..12,
// bytes 2..12 of the temporal kernel's 15x15 window.  Here a query loads its record and both
// modes' (qbest, qsecond) in one round and both trains' (tbest, keypoint word) in the next, then
// stages each image region once, its rows dealt over the 8 sub-lanes with every round's loads in
// flight together (one instruction stream: any row is 15 bytes from 4 or 5 aligned dwords; the t-1
// patch rows are cut to 11):
//   rows  0..14  the window at t (temporal match), or its rows 2..12 only (stereo match alone)
//   rows 15..25  the 11x11 patch at t-1            (temporal match)
//   rows 26..36  the 15x11 right window            (stereo match)
// 37 rows in 5 rounds with both matches, where the two kernels gather 22 + 26.  Sub-lanes 0..4 then
// score the temporal column shifts and the 5 stereo offsets (the lanes of a wave share one
// instruction stream, so handing the stereo offsets to sub-lanes 5..7 would add their 2 x 11 rows
// to every wave's time instead of 11).  Outputs are bit for bit the two kernels'.
#define TS_RP_QPB 32   // queries per block
#define TS_RP_ROWS (TS_RT_BROWS + TS_RT_AROWS + 11)
#define TS_RP_ROUNDS ((TS_RP_ROWS + 7) / 8)
__global__ __launch_bounds__(256) void k_refine_pair(BatchCtx c) {
    TS_BACK_PRIO;
    __shared__ uint4 s_rows[TS_RP_QPB][TS_RP_ROWS];
    __shared__ int s_ct[TS_RP_QPB][25];
    __shared__ int s_cs[TS_RP_QPB][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = c.g.K;
    int z, local;
    if (!xcd_image_block3(c.n * c.npair, (K + TS_RP_QPB - 1) / TS_RP_QPB, &z, &local)) return;
    const int f = div_small(z, c.npair_rcp), p = c.pair0 + (z - f * c.npair);
    const bool has_prev = c.g0 + f > 0;   // frame 0 of the sequence: nothing matches
    const int slot = batch_slot(c, f);
    const int pslot = has_prev ? prev_slot(c, slot) : slot;
    const int sub = lane & 7;
    const int qslot = wave * 8 + (lane >> 3);
    const int pos = local * TS_RP_QPB + qslot;
    const bool live = pos < K;
    const size_t mbase = ((size_t)f * c.P + p) * 2 * K;   // stereo; temporal at + K
    const int qcam = c.cpp * p;
    const size_t qkb = ((size_t)slot * c.C + qcam) * K;
    int l = 0, qi = 0, js = -1, jt = -1;
    uint32_t qxy = 0, tkp = 0, pxy = 0;
    if (live) {
        const uint4 rec = c.ys[qkb + pos];
        qi = (int)rec.z;
        l = (int)(rec.y & 0xFFu);
        qxy = rec.x;
        MatchRef ms, mt;
        match_query(c, mbase, pos, &ms);
        match_query(c, mbase + K, pos, &mt);
        match_train(c, mbase, ((size_t)slot * c.C + qcam + 1) * K, &ms, &tkp);
        match_train(c, mbase + K, ((size_t)pslot * c.C + qcam) * K, &mt, &pxy);
        js = match_accept(c, ms, qi, rec.w != 0);
        jt = match_accept(c, mt, qi, rec.w != 0 && has_prev);
    }
    const size_t out = ((size_t)slot * c.P + p) * K + qi;
    if (live && sub == 0) c.temporal[out] = jt;
    const int qx = qxy & 0xFFFF, qy = qxy >> 16, xr = tkp & 0xFFFF;
    {
        // the level's pitch and offset by selects over the (uniform) table: indexing it by the
        // lane's level is a load, one more dependent round
        int W = c.g.W[0], loff = c.g.pyr_off[0];
#pragma unroll
        for (int i = 1; i < TS_MAX_LEVELS; ++i)
            if (l >= i) W = c.g.W[i], loff = c.g.pyr_off[i];
        const int px = pxy & 0xFFFF, py = pxy >> 16;
        const uint8_t* cur = c.pyr + ((size_t)slot * c.C + qcam) * c.g.pyr_bytes + loff;
        const uint8_t* rgt = cur + c.g.pyr_bytes;
        const uint8_t* prv = c.pyr + ((size_t)pslot * c.C + qcam) * c.g.pyr_bytes + loff;
        const int nw = jt >= 0 ? TS_RT_BROWS : js >= 0 ? 11 : 0, w0 = jt >= 0 ? 0 : TS_SAD_RANGE;
        const int np = jt >= 0 ? TS_RT_AROWS : 0;
        const int total = nw + np + (js >= 0 ? 11 : 0);
        uint32_t d[TS_RP_ROUNDS][5], sh[TS_RP_ROUNDS];
#pragma unroll
        for (int k = 0; k < TS_RP_ROUNDS; ++k) {
            const int hl = sub + 8 * k;
            const bool inw = hl < nw, inp = !inw && hl < nw + np;
            const int r = inw ? hl + w0 : inp ? hl - nw : hl - nw - np;
            const uint8_t* img = inw ? cur : inp ? prv : rgt;
            const int y = inw ? qy - TS_SAD_HALF - TS_SAD_RANGE + r : inp ? py - TS_SAD_HALF + r : qy - TS_SAD_HALF + r;
            const int x0 = inw ? qx - TS_SAD_HALF - TS_SAD_RANGE : inp ? px - TS_SAD_HALF : xr - TS_SAD_HALF - TS_SAD_RANGE;
            // a lane with no row left loads the level's first bytes (unconditional loads: no
            // branch, so no wait, between the rounds)
            const uint8_t* a = hl < total ? img + (size_t)y * W + x0 : cur;
            sh[k] = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3u);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a - sh[k]);
#pragma unroll
            for (int i = 0; i < 4; ++i) d[k][i] = q[i];
            // the fifth dword only where a 15-byte row reaches into it (the t - 1 patch rows are 11 bytes)
            d[k][4] = (!inp && sh[k] >= 2u) ? q[4] : 0u;
        }
#pragma unroll
        for (int k = 0; k < TS_RP_ROUNDS; ++k) {
            const int hl = sub + 8 * k;
            const bool inw = hl < nw, inp = !inw && hl < nw + np;
            uint4 v = align_row15(d[k], sh[k]);
            if (inp) v.z &= 0x00FFFFFFu, v.w = 0u;
            const int row = inw ? hl + w0 : inp ? TS_RT_BROWS + hl - nw : TS_RT_BROWS + TS_RT_AROWS + hl - nw - np;
            if (hl < total) s_rows[qslot][row] = v;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // staged rows before the reads (own wave)
    const uint4* rows = s_rows[qslot];
    uint32_t kt = 0xFFFFFFFFu, ks = 0xFFFFFFFFu;   // first minima of (cost << 5 | offset)
    if (jt >= 0 && sub < 5) {
        uint32_t s[5];
        temporal_sad(rows + TS_RT_BROWS, rows, sub, s);
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
            const int o = ky * 5 + sub;
            s_ct[qslot][o] = (int)s[ky];
            kt = min(kt, (s[ky] << 5) | (uint32_t)o);
        }
    }
    if (js >= 0 && sub < 5) {
        const uint32_t s = stereo_sad<TS_SAD_RANGE>(rows + TS_SAD_RANGE, rows + TS_RT_BROWS + TS_RT_AROWS, sub);
        s_cs[qslot][sub] = (int)s;
        ks = (s << 5) | (uint32_t)sub;
    }
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) {
        kt = min(kt, (uint32_t)__shfl_xor((int)kt, m, 64));
        ks = min(ks, (uint32_t)__shfl_xor((int)ks, m, 64));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // costs of the 5 lanes before the reads
    if (live && sub == 0) {
        temporal_store(c.tuv + (((size_t)f * c.P + p) * K + qi) * 2, jt, l, qx, qy, (int)(kt & 31u), s_ct[qslot]);
        stereo_store(c, out, js, l, qx, xr, (int)(ks & 31u), s_cs[qslot]);
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_match(BatchCtx c) { match_body<false>(c); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_match_counted(BatchCtx c) { match_body<true>(c); }

static void launch_k_match(const BatchCtx& c, dim3 grid, hipStream_t s) {
    if (c.match_cnt)
        hipLaunchKernelGGL(k_match_counted, grid, dim3(256), 0, s, c);
    else
        hipLaunchKernelGGL(k_match, grid, dim3(256), 0, s, c);
}

int match_blocks_per_cu() {
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_match, 256, 0) == hipSuccess ? n : -1;
}

// tbest takes atomic minima, so it starts from all ones; qbest needs no clearing: k_match writes
// every position of every level it is launched for
void launch_match(const BatchCtx& c, hipStream_t s) {
    (void)hipMemsetAsync(c.tbest, 0xFF, sizeof(uint32_t) * (size_t)c.n * c.P * 2 * c.g.K, s);
    // one block per tile and frame pair serves both sides; the split layout has one per side
    dim3 grid(c.g.total_qtiles, c.n * c.npair * (c.match_modes != 1 && c.mp.split ? 2 : 1));
    launch_k_match(c, grid, s);
}

// Stereo matching + refinement only (the sharded rig's pre-pass for the frame before a rank's
// range, whose disparities the range's first frame triangulates from).
void launch_match_stereo(const BatchCtx& c, hipStream_t s) {
    BatchCtx st = c;
    st.match_modes = 1;
    (void)hipMemsetAsync(st.tbest, 0xFF, sizeof(uint32_t) * (size_t)st.n * st.P * 2 * st.g.K, s);
    launch_k_match(st, dim3(st.g.total_qtiles, st.n * st.npair), s);
    hipLaunchKernelGGL(k_refine_stereo, xcd_grid3(st.n * st.npair, (st.g.K + TS_RS_QPB - 1) / TS_RS_QPB), dim3(256), 0, s, st);
}

void launch_match_refine(const BatchCtx& c, hipStream_t s) {
    const int K = c.g.K;
    // a stereo frame's two refinements in one kernel, unless tslam_params.match_refine asks for the two
    if (!c.rgbd && c.match_modes == 3 && c.mp.refine_split == 0) {
        hipLaunchKernelGGL(k_refine_pair, xcd_grid3(c.n * c.npair, (K + TS_RP_QPB - 1) / TS_RP_QPB), dim3(256), 0, s, c);
        return;
    }
    if (c.rgbd)
        launch_rgbd_depth(c, s);
    else
        hipLaunchKernelGGL(k_refine_stereo, xcd_grid3(c.n * c.npair, (K + TS_RS_QPB - 1) / TS_RS_QPB), dim3(256), 0, s, c);
    hipLaunchKernelGGL(k_refine_temporal, xcd_grid3(c.n * c.npair, (K + TS_RT_QPB - 1) / TS_RT_QPB), dim3(256), 0, s, c);
}
