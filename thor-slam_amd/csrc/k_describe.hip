// k_describe.hip — row A5 of SURVEY.md §8a: intensity-centroid orientation + rotated BRIEF-256.
//
// Tile-staged: a block owns a 128 x 64 tile of one level.  It copies the tile plus halo of the
// raw level (orientation) and of the smoothed level (BRIEF) into LDS with 16-byte LDS-DMA loads,
// then serves every keypoint inside the tile from LDS, one wave per keypoint.  A wave-per-
// keypoint design that fetched each 37x37 patch from L2 issued ~10 cache-line requests per
// wave-load and ran L2-request-bound; staging reads every line of the tile once (the patches of
// neighbouring keypoints overlap ~3-4x).
//  * keypoints of the tile: the y-sorted records of the tile's rows (rowstart), filtered by x and
//    compacted into an LDS list of (xy, position | index << 16), TS_DT_LIST positions at a time, so
//    the keypoint loop starts from one LDS read and never loads a record;
//  * orientation: lane (row, word) holds the realigned word at dx = 4w - 15 .. 4w - 12 of disc
//    row dy = row - 15; m10 = dot4(wx, I) - 15 dot4(mask, I), m01 = dy dot4(mask, I) with
//    per-lane constant byte weights (3 ops per word); bin by 30 wedge tests in parallel lanes;
//  * BRIEF: the rotated pattern is a table of byte offsets for the tile pitch (built by the host),
//    2 ds_read_u8 + 1 compare per test, four wave ballots per descriptor;
//  * stores: a wave collects eight keypoints' descriptors in one VGPR (keypoint i in lanes 8 i ..)
//    and stores desc, desc_ys and the orientation bytes of kps once per eight, after the keypoint
//    loop: vmcnt counts stores too, and a store inside the loop is waited for by the next table
//    load.  The loop has no branch: a wave's instruction stream, not a unit's throughput, is what
//    the kernel's time follows (describe).
// Bit-exact with oracle.orientation_bins / oracle.brief.
#include "tslam_common.h"

// shared with the host (tslam_api.cpp builds the BRIEF offset table for TS_DT_P)
#include "tslam_describe.h"

// 16-byte async global -> LDS copy; `wave_dst` is the wave-uniform LDS base, lane k lands at +16k
__device__ __forceinline__ void glds16d(const void* src, void* wave_dst) {
    __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)wave_dst, 16, 0, 0);
}

// Copy rows [r0, r0 + nrows) x the first NLD of the NCH 16-byte chunks of columns [cs, cs + 16 NCH)
// of a level (pitch W, H rows) into an LDS image of pitch 16 NCH (lane-linear: the LDS-DMA lands a
// wave's 64 chunks contiguously; chunks NLD.. of a row are LDS pitch padding).  Rows outside the
// level and chunks outside [0, W) are skipped (the keypoint margin guarantees no keypoint reads
// them).
template <int NCH, int NLD = NCH>
__device__ __forceinline__ void stage_tile(const uint8_t* level, int W, int H, int r0, int cs, int nrows,
                                           uint8_t* lds, bool wide16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wide16) {
        const int n = nrows * NCH;
        for (int i0 = wave * 64; i0 < n; i0 += TS_DT_THREADS) {
            const int i = i0 + lane;
            if (i < n) {
                const int r = i / NCH, q = i - r * NCH;
                const int y = r0 + r, x = cs + 16 * q;
                if (q < NLD && y >= 0 && y < H && x >= 0 && x + 16 <= W) glds16d(level + (size_t)y * W + x, lds + 16 * i0);
            }
        }
    } else {
        for (int i = threadIdx.x; i < nrows * 16 * NCH; i += TS_DT_THREADS) {
            const int r = i / (16 * NCH), q = i - r * (16 * NCH);
            const int y = r0 + r, x = cs + q;
            if (y >= 0 && y < H && x >= 0 && x < W) lds[i] = level[(size_t)y * W + x];
        }
    }
}

// Per-lane orientation disc constants of slot s = lane + 64 i (i < 5): byte weights dx + 15,
// dy + 15 and the 0/1 mask of the 4 pixels of dword w = s % 9 in disc row r = s / 9 (pixel
// dx = 4w - 15 + j, dy = r - 15, inside the radius-15 disc), and the word's LDS offset in the raw
// tile.  Built at compile time: one 16-byte load per slot instead of the per-block disc
// arithmetic.  The offset weights keep all three moment sums on v_dot4_u32_u8 (no 32-bit
// multiplies): m10 = sum (dx + 15) I - 15 sum I, m01 = sum (dy + 15) I - 15 sum I.
struct DiscSlot {
    uint32_t wx, mk, wy;
    int32_t rofs;
};
struct DiscTable {
    DiscSlot e[320];
};
constexpr DiscTable make_disc_table() {
    DiscTable t{};
    for (int s = 0; s < 320; ++s) {
        const int r = s / 9, w = s - 9 * r;
        uint32_t a = 0, m = 0, b = 0;
        for (int j = 0; j < 4; ++j) {
            const int dx = 4 * w - 15 + j, dy = r - 15;
            if (r < 31 && dx <= 15 && dx * dx + dy * dy <= 225) {
                a |= (uint32_t)(dx + 15) << (8 * j);
                m |= 1u << (8 * j);
                b |= (uint32_t)(dy + 15) << (8 * j);
            }
        }
        t.e[s] = DiscSlot{a, m, b, (r < 30 ? r : 30) * TS_DT_RAW_P + 4 * w};
    }
    return t;
}
__constant__ DiscTable c_disc = make_disc_table();

// Per-lane wedge directions of the orientation bins as doubles: lane b < 30 tests bin b against the
// directions b and b + 1 of the table the host ships to the device (tslam_tables.h); lanes 30.. hold
// zeros and never hit.  Built at compile time like c_disc: two 16-byte loads per lane.
#include "tslam_tables.h"
struct WedgeTable {
    double e[64][4];
};
constexpr WedgeTable make_wedge_table() {
    WedgeTable t{};
    for (int b = 0; b < 30; ++b)
        for (int j = 0; j < 4; ++j) t.e[b][j] = (double)TSLAM_WEDGES[2 * b + j];
    return t;
}
__constant__ WedgeTable c_wedge = make_wedge_table();

// keeps the four values (and the reads behind them) in front of whatever follows
__device__ __forceinline__ void bar4(int& a, int& b, int& c, int& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }

// dst's lane base + J = word (word and base wave-uniform).  Two scalar registers in one VALU
// instruction exceed gfx9's constant bus, so the lane select travels in m0, which does not count.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"   // m0 is reserved; nothing after the tile copies reads it
template <int J>
__device__ __forceinline__ void writelane_m0(uint32_t& dst, uint32_t word, int base) {
    asm volatile("s_add_u32 m0, %2, %3\n\tv_writelane_b32 %0, %1, m0" : "+v"(dst) : "s"(word), "s"(base), "n"(J) : "m0", "scc");
}
#pragma clang diagnostic pop

__global__ __launch_bounds__(TS_DT_THREADS) void k_describe(BatchCtx c) {
    // raw tile: the orientation discs' columns [x0 - 16, x0 + 144) only (10 chunks), + 1 row of
    // slack for the masked bytes the last disc row's dword window reads past the row end
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[(TS_DT_RAW_ROWS + 1) * TS_DT_RAW_P];
    __shared__ __attribute__((aligned(16))) uint8_t s_smo[TS_DT_SMO_ROWS * TS_DT_P];
    __shared__ uint2 s_list[TS_DT_LIST];   // xy word, y-sorted position | keypoint index << 16
    __shared__ uint32_t s_n[2];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // block -> (image, level, tile) from the grid (8, dt_total, image groups) and the host's tile
    // table: all tiles of one image on one XCD, no division and no level search
    int img, local;
    if (!xcd_image_block3(c.n * c.ncam, c.g.dt_total, &img, &local)) return;
    const uint32_t tile = c.dt_tile[local];
    const int l = (int)(tile & 0xFFu), tx = (int)((tile >> 8) & 0xFFu), ty = (int)(tile >> 16);
    const bool first = local == c.g.dt_start[l];   // the level's first tile
    const int W = c.g.W[l], H = c.g.H[l];
    const int x0 = tx * TS_DT_W, y0 = ty * TS_DT_H;
    int cam, f;
    view_image(c, img, &f, &cam);
    const int slot = batch_slot(c, f);
    const size_t ib = (size_t)slot * c.C + cam;
    const int koff = c.g.koff[l];
    const uint8_t* raw = c.pyr + ib * c.g.pyr_bytes + c.g.pyr_off[l];
    const uint8_t* smo = c.smo + ((size_t)f * c.C + cam) * c.g.pyr_bytes + c.g.pyr_off[l];
    uint32_t* kps = c.kps + ib * c.g.K * 2;
    uint32_t* desc = c.desc + ib * c.g.K * 8;
    uint32_t* desc_ys = c.desc_ys + (ib * c.g.K + koff) * 8;   // the level's y-sorted descriptors
    const uint4* ys = c.ys + ib * c.g.K + koff;
    // the tile's range of y-sorted records: two u16 of the row-start table, each read as its
    // aligned dword (the image's table starts on 16 bytes) so that the uniform loads can take the
    // scalar path and are not waited for together with the tile copies below
    const size_t ra = ib * c.g.rs_total + c.g.rs_off[l] + y0, rb = ra + (min(y0 + TS_DT_H, H) - y0);
    const uint32_t* rs32 = reinterpret_cast<const uint32_t*>(c.rowstart);
    const uint32_t wa = rs32[ra >> 1], wb = rs32[rb >> 1];
    const int kn = first ? c.kcount[ib * c.g.n_levels + l] : 0;
    if (threadIdx.x == 0) s_n[0] = 0;
    __syncthreads();   // before any copy is in flight: a barrier waits for the block's loads

    // both tiles on their way before anything is waited for: the list and the constants run while
    // the LDS-DMA is in flight
    const bool wide16 = ((W & 15) == 0) && ((c.g.pyr_off[l] & 15) == 0) && ((c.g.pyr_bytes & 15) == 0);
    const int c0 = x0 - TS_DT_HX;        // smoothed tile's column origin (pitch TS_DT_P)
    const int cr = x0 - 16;              // raw tile's column origin (pitch TS_DT_RAW_P)
    stage_tile<TS_DT_RAW_P / 16>(raw, W, H, y0 - 15, cr, TS_DT_RAW_ROWS, s_raw, wide16);
    // smoothed tile: BRIEF reads columns [x0 - 18, x0 + 146): chunks 0..11; chunk 12 is the pad
    stage_tile<TS_DT_P / 16, (TS_DT_W + 2 * TS_DT_HX) / 16>(smo, W, H, y0 - 18, c0, TS_DT_SMO_ROWS, s_smo, wide16);

    const int pa = (int)((wa >> (16 * (ra & 1))) & 0xFFFFu), pb = (int)((wb >> (16 * (rb & 1))) & 0xFFFFu);
    if (pa < pb) {
        // per-lane disc constants (slot s = lane + 64 i; see DiscTable)
        uint32_t wx[5], mk[5], wy[5];
        int rofs[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const uint4 d = reinterpret_cast<const uint4*>(&c_disc)[lane + 64 * i];
            wx[i] = d.x;
            mk[i] = d.y;
            wy[i] = d.z;
            rofs[i] = (int)d.w;
        }
        // wedge directions as doubles: |u| < 2^25 and |m| < 2^23, so every product and difference
        // below is an exact integer in f64 (< 2^53) and the sign tests equal the int64 ones
        const double wa0 = c_wedge.e[lane][0], wa1 = c_wedge.e[lane][1], wb0 = c_wedge.e[lane][2], wb1 = c_wedge.e[lane][3];

        // up to 8 finished keypoints of the wave, keypoint i in lanes 8 i .. 8 i + 7: the descriptor
        // word per lane, position | index << 16 and the orientation bin per lane group
        uint32_t acc = 0, a_pk = 0, a_bin = 0;
        const int cap = (unsigned)(c.dt_list_cap - 1) < (unsigned)TS_DT_LIST ? c.dt_list_cap : TS_DT_LIST;
        // the tile's rows in chunks of `cap` y-sorted positions (one chunk unless the rows hold more
        // records than the list; chunk k counts in s_n[k & 1], zeroed while chunk k - 1 is served)
        int k = 0;
        for (int ca = pa; ca < pb; ca += cap, k ^= 1) {
            const int cb = min(ca + cap, pb);
            // keypoints of the tile: the records of its rows filtered by x, compacted into an LDS
            // list so the waves get equal shares (order is irrelevant: every keypoint is
            // independent).  An entry is all the loop needs of the record.
            for (int p = ca + threadIdx.x; p < cb; p += TS_DT_THREADS) {
                uint4 r = ys[p];
                asm volatile("" : "+v"(r.z));   // one load for both words, not a second one behind the x test
                const int x = r.x & 0xFFFF;
                if (x >= x0 && x < x0 + TS_DT_W) s_list[atomicAdd(&s_n[k], 1u)] = uint2{r.x, (uint32_t)p | (r.z << 16)};
            }
            __syncthreads();   // tiles landed (drains the LDS-DMA) and the list is complete
            const int n = (int)s_n[k];
            if (cb < pb && threadIdx.x == 0) s_n[k ^ 1] = 0;
            // a wave's keypoints eight at a time: no global access but the table rows inside the
            // keypoint loop, one set of stores per eight
            for (int g0 = wave; g0 < n; g0 += TS_DT_THREADS / 8) {
                const int g1 = min(g0 + TS_DT_THREADS / 8, n);
                int sl = 0;
                for (int g = g0; g < g1; g += TS_DT_THREADS / 64, ++sl) {
                    const uint2 e = s_list[g];
                    const int x = e.x & 0xFFFF, y = e.x >> 16;
                    // orientation: disc origin (x - 15, y - 15) in the raw tile
                    const int ob = (int)__umul24((uint32_t)(y - y0), TS_DT_RAW_P) + (x - 15 - cr);   // both < 2^24
                    const uint32_t sh = (uint32_t)ob & 3u;
                    const uint8_t* obase = s_raw + (ob & ~3);
                    uint32_t sx = 0, s1 = 0, sy = 0;
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        const uint32_t* wp = reinterpret_cast<const uint32_t*>(obase + rofs[i]);
                        const uint32_t v = __builtin_amdgcn_alignbyte(wp[1], wp[0], sh);
                        s1 = __builtin_amdgcn_udot4(mk[i], v, s1, false);
                        sx = __builtin_amdgcn_udot4(wx[i], v, sx, false);
                        sy = __builtin_amdgcn_udot4(wy[i], v, sy, false);
                    }
                    // per-lane sums < 2^17: 15 * s1 as one full-rate 24-bit multiply
                    const int s15 = (int)__umul24(s1, 15u);
                    const int m10 = wave_sum_dpp((int)sx - s15);
                    const int m01 = wave_sum_dpp((int)sy - s15);
                    const double d01 = (double)m01, d10 = (double)m10;
                    // no branch: lanes 30.. hold zero directions and fail the second test
                    const bool hit = ((wa0 * d01 - wa1 * d10) >= 0.0) & ((wb0 * d01 - wb1 * d10) < 0.0);
                    const uint64_t hm = __ballot(hit);
                    const int bin = hm ? (int)__builtin_ctzll(hm) : 0;
                    uint32_t t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) t[j] = c.brief_table[bin * 256 + 64 * j + lane];
                    // BRIEF: patch origin (x - 18, y - 18) in the smoothed tile
                    const uint8_t* pbase = s_smo + ((int)__umul24((uint32_t)(y - y0), TS_DT_P) + (x - 18 - c0));
                    // all eight reads in flight together, then word j (wave-uniform) into lane 8 sl + j
                    int a[4], b[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a[j] = pbase[t[j] & 0xFFFFu];
                        b[j] = pbase[t[j] >> 16];
                    }
                    bar4(a[0], a[1], a[2], a[3]);
                    const uint64_t bm0 = __ballot(a[0] < b[0]), bm1 = __ballot(a[1] < b[1]);
                    const uint64_t bm2 = __ballot(a[2] < b[2]), bm3 = __ballot(a[3] < b[3]);
                    writelane_m0<0>(acc, (uint32_t)bm0, 8 * sl);
                    writelane_m0<1>(acc, (uint32_t)(bm0 >> 32), 8 * sl);
                    writelane_m0<2>(acc, (uint32_t)bm1, 8 * sl);
                    writelane_m0<3>(acc, (uint32_t)(bm1 >> 32), 8 * sl);
                    writelane_m0<4>(acc, (uint32_t)bm2, 8 * sl);
                    writelane_m0<5>(acc, (uint32_t)(bm2 >> 32), 8 * sl);
                    writelane_m0<6>(acc, (uint32_t)bm3, 8 * sl);
                    writelane_m0<7>(acc, (uint32_t)(bm3 >> 32), 8 * sl);
                    if ((lane >> 3) == sl) {
                        a_pk = e.y;
                        a_bin = (uint32_t)bin;
                    }
                }
                // the group's stores.  k_select left level | score << 16 in the keypoint's second
                // word (the record's second word): the bin is its byte 1, no record is read for it
                if (lane < 8 * sl) {
                    const uint32_t kidx = a_pk >> 16, pos = a_pk & 0xFFFFu, j = lane & 7u;
                    desc[(size_t)kidx * 8 + j] = acc;
                    desc_ys[(size_t)pos * 8 + j] = acc;
                    if (j == 0) reinterpret_cast<uint8_t*>(kps + (size_t)kidx * 2 + 1)[1] = (uint8_t)a_bin;
                }
            }
            if (cb < pb) __syncthreads();   // every wave is done with the list before the next chunk
        }
    } else {
        // no keypoint in the tile's rows (block-uniform): the copies must land before the block
        // ends, or they would land in LDS that the next block already owns
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    // padding slots of the level get zero descriptors (the level's first tile does it, behind its
    // keypoints: no store of the block stands in front of a table load)
    if (first) {
        const int Kl = c.g.Kq[l];
        for (int i = kn * 8 + threadIdx.x; i < Kl * 8; i += TS_DT_THREADS) {
            desc[(size_t)(koff + i / 8) * 8 + (i & 7)] = 0u;
            desc_ys[i] = 0u;
        }
    }
}

void launch_describe(const BatchCtx& c, hipStream_t s) {
    hipLaunchKernelGGL(k_describe, xcd_grid3(c.n * c.ncam, c.g.dt_total), dim3(TS_DT_THREADS), 0, s, c);
}
