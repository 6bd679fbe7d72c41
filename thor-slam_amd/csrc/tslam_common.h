// tslam_common.h — device-side layout shared by the gfx950 kernels and the C-ABI host code.
//
// HBM layout (one handle = one device, P stereo pairs, C = 2P cameras, K keypoints/image,
// batch B frames, ring R = 2B + 1 frames (+ the keyframe interval with BA) so frame t-1 of a
// batch's first frame is still resident while the next batch's front stages run):
//
//   pyramid  u8  [R][C][pyr_bytes]   rectified level 0 + 2x2 box levels, each level dense (pitch W_l)
//   smooth   u8  [B][C][pyr_bytes]   5x5 binomial of every level (BRIEF sampling image)
//   cand     u32 [B][C][cand_total]  per (level, 16-row band) fixed-capacity key segments
//   ccount   u32 [B][C][total_bands] keys written per band
//   hist     u32 [B][C][L][256]      survivor histogram in key order (bin = 255 - score)
//   kps      u32 [R][C][K][2]        {x | y<<16, level | angle<<8 | score<<16}
//   kcount   i32 [R][C][L]
//   desc     u32 [R][C][K][8]        rBRIEF-256
//   ys       u32x4 [R][C][K]  desc_ys u32 [R][C][K][8]  per level, keypoints sorted by (y, rank):
//            {xy, level | score<<16, kp index, valid} and their descriptors (contiguous match staging)
//   rowstart u16 [R][C][sum(H_l+1)]  per level: first y-sorted position of row y
//   qbest/qsecond/tbest u32 [B][P][2][K]   matching scratch (mode 0 stereo, 1 temporal): qbest, qsecond by
//            the query's y-sorted position, tbest by the train's; qtpos u16 [B][P][2][K] that train position
//   ypos     u16 [R][C][K]           keypoint index -> y-sorted position (the inverse of ys' index word)
//   stereo   i32 [R][P][K]  disp f64 [R][P][K]        stereo match + refined disparity of left kps
//            (RGB-D: disp = fx / Z from the aligned depth, a virtual 1 m baseline; stereo = k or -1)
//   temporal i32 [R][P][K]  tuv  f64 [B][P][K][2]     temporal match + refined (u, v) at t
//   corr     f64 [B][P][K][8]        X Y Z du dv bx by bz (ordered by t keypoint index)
//   pose     f64 [B][P][68]          T_rel, T_abs, cov;  stats i32 [B][P][8];  state f64 [P][16]
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define TS_MAX_LEVELS 6
// tslam_detect_counters: per level, three stages (phase B bright, phase B dark, NMS) x (rounds of 64
// inside the loop, tail rounds, lanes filled in the tail rounds), then the blocks that ran.  Phase
// B's tails are pooled over the block's waves; an NMS tail round is a wave's own.
#define TS_DCNT 12
#define TS_DCNT_BLOCKS 9
// detect band height: 32 rows while the band's LDS (2 * rows + 10 rows of W bytes) stays <= 48 KiB
// (3 blocks per CU; fewer halo rows and barriers per pixel), else 24 or 16 (LevelGeom::band_rows)
#define TS_BAND_ROWS_MAX 32
#define TS_DET_HALO 4
#define TS_RECT_BAND 32
#define TS_MATCH_CHUNK 512
#define TS_MTB 896         // k_match: entries of a block's train-side merge array (k_match.hip)
#define TS_SAD_HALF 5
#define TS_SAD_RANGE 2
#define TS_POSE_DOUBLES 68
#define TS_STATS_INTS 8
#define TS_CORR_DOUBLES 8
#define TS_MAX_HYP 1024
// one P3P candidate pose: [R 9 | t 3] f64, then f32 R 9, t 3, max |R_ij|, max |t_i| and 2 pad
// (the scoring pass reads the f32 record through scalar loads as operands of its inlier test)
#define TS_HYP_DOUBLES 20
#define TS_MAX_SPLITS 32   // RANSAC blocks per frame
#define TS_RANSAC_WORDS 26 // per split: key + pad + 12 doubles
#define TS_PRIOR_DOUBLES 16 // per (frame, pair): IMU prior R (row-major 3x3), W_r, t[3], W_t, 0, 0
#define TS_BA_CU_RESERVE 96   // CUs the front / back streams leave to the BA stream (tslam_submit_host;
                              // bench.py --front-cu-reserve sweep)
// Wave issue priority of the back kernels (match .. chain, rig pose): latency-bound waves that share
// the SIMDs with the next batch's front-end waves (detect, describe: throughput-bound) get served
// first (C2 234.7-235.3k -> 235.6-235.9k frames/s, C3 59.75k -> 60.05k; the front kernels at
// priority 1 or 2 instead were 1 % slower).  The local BA's kernels use 3 (k_ba.hip).
#define TS_BACK_PRIO __builtin_amdgcn_s_setprio(2)
#define TS_BA_MAXW 10      // keyframes per BA window (6 camera rows each in the 64-wide system)

struct LevelGeom {
    int n_levels;
    int W[TS_MAX_LEVELS], H[TS_MAX_LEVELS];
    int pyr_off[TS_MAX_LEVELS];
    int pyr_bytes;
    int K;
    int Kq[TS_MAX_LEVELS], koff[TS_MAX_LEVELS];
    int band_rows[TS_MAX_LEVELS];  // detect band height per level (LevelGeom rule in build_geometry)
    int smooth_groups[TS_MAX_LEVELS];   // detect smoothing: row groups per band (items = groups x quads)
    int det_lds;                   // detect dynamic LDS bytes: max over levels of (2 rows + 10) x W
    int nbands[TS_MAX_LEVELS], band_start[TS_MAX_LEVELS];
    int total_bands;
    int cand_cap[TS_MAX_LEVELS];   // keys per band at level l
    int cand_off[TS_MAX_LEVELS];   // u32 offset of level l's first band segment (per image)
    int cand_total;                // u32 per image
    int qtiles[TS_MAX_LEVELS], qtile_start[TS_MAX_LEVELS];  // 128-query k_match tiles per level
    int total_qtiles;
    int rs_off[TS_MAX_LEVELS];     // u16 offset of level l's row-start table (H_l + 1 entries)
    int rs_total;                  // u16 per image
    int dt_nx[TS_MAX_LEVELS], dt_start[TS_MAX_LEVELS];   // describe tiles: per row of level l, first tile
    int dt_total;                  // describe tiles per image
};

// k_describe's block decode as a table: for block i of an image (0 <= i < dt_total) the word
// level | tile column << 8 | tile row << 16 (tiles of level l are dt_start[l] .. in row-major order,
// dt_nx[l] per row), so the block finds its tile with one load instead of a level search and a division
static inline void describe_tile_table(const LevelGeom& g, uint32_t* out) {
    for (int l = 0; l < g.n_levels; ++l) {
        const int end = l + 1 < g.n_levels ? g.dt_start[l + 1] : g.dt_total;
        for (int i = g.dt_start[l]; i < end; ++i) {
            const int local = i - g.dt_start[l], ty = local / g.dt_nx[l], tx = local - ty * g.dt_nx[l];
            out[i] = (uint32_t)l | ((uint32_t)tx << 8) | ((uint32_t)ty << 16);
        }
    }
}

struct PairCalib {
    double fx, fy, cx, cy, fxb;     // fxb = fx * baseline
};

struct MatchParams {
    int max_hamming, ratio_pct, row_tol, max_disp, window;
    int refine_split;   // stereo + temporal refinement: 0 one fused kernel (k_refine_pair), 1 the two kernels
    int merge_cap;      // k_match: train positions per block merged in LDS before tbest (0: none; tslam_match_mode)
    int split;          // k_match: 0 a block matches both sides of its tile, 1 one side per block (tslam_match_layout)
};

struct PoseParams {
    int n_hyp, iters, min_inliers, splits;
    int mode;   // RANSAC scoring: 0 auto, 1 exhaustive (k_ransac_all), 2 bounded (k_ransac)
    int refine_block;   // k_refine threads per frame: 0 auto, 128, 256
    double thr2;
    uint64_t seed;
};

// Everything a batch launch needs; built by the host per stage call.
struct BatchCtx {
    LevelGeom g;
    int C, P, B, R;
    int cpp;               // cameras per pair: 2 (stereo), 1 (RGB-D: colour camera + aligned depth)
    int rgbd;
    int n;                 // frames in this batch
    // camera view of the front-end kernels (rectify .. describe): cameras cam0 .. cam0+ncam-1 of
    // every frame, images [n][ncam][H][W] (the whole rig: 0, C; a sharded rig: the rank's streams)
    int cam0, ncam;
    // pair view of the back-end kernels (match .. pose): pairs pair0 .. pair0+npair-1 of every
    // frame (the whole rig: 0, P; a camera-sharded RGB-D rig: the rank's cameras); batch buffers
    // keep their [n][P] layout
    int pair0, npair;
    int match_modes;       // k_match: 3 = temporal + stereo, 1 = stereo only (sharded pre-pass)
    int reloc;             // k_rig_pose solves a relocalisation (frame 0 is not a first frame)
    // peer layout of a sharded import (tslam_import_peers): images [world][nbuf][S][H][W] as the
    // all-to-all delivers them; the launch covers the world-1 peers' slots (not peer_me's), frames
    // peer_skip .. nbuf-1 of each (peer_S = 0: the plain [n][ncam] view above)
    int peer_S, peer_me, peer_nbuf, peer_skip;
    int64_t g0;            // global index of the batch's first frame (set with ctx_set_first_frame)
    int slot0;             // g0 % R: ring slot of the batch's first frame (batch_slot)
    uint32_t ncam_rcp, npair_rcp;   // floor(2^32 / ncam) + 1, the same of npair (0 for 1): div_small
    const uint32_t* dt_tile;        // [dt_total] describe tile of an image's block: level | column << 8 | row << 16
    int W, H;              // level-0 size
    // inputs
    const uint8_t* images; // [n][C][H][W] gray (RGB-D: the converted staging buffer)
    const uint8_t* rgbd_in; // RGB-D only: [n][P][BGR u8 H*W*3 | depth u16 mm H*W]
    const int32_t* maps;   // [C][H][W][2] or nullptr
    uint32_t map_mask;     // bit c set -> camera c has a map (else identity)
    // buffers
    uint8_t* pyr;
    uint8_t* smo;
    uint32_t* cand;
    uint32_t* ccount;
    uint32_t* hist;
    uint32_t* kps;
    int32_t* kcount;
    uint32_t* desc;
    uint4* ys;             // [R][C][K] y-sorted keypoint records
    uint32_t* desc_ys;     // [R][C][K][8] y-sorted descriptors
    uint16_t* rowstart;    // [R][C][rs_total]
    uint32_t* qbest;
    uint32_t* qsecond;
    uint32_t* tbest;       // [B][P][2][K] by the train's y-sorted position
    uint16_t* ypos;        // [R][C][K] keypoint index -> y-sorted position (select, the sharded import)
    uint16_t* qtpos;       // [B][P][2][K] by query position: ypos of its best train
    int32_t* stereo;
    double* disp;
    int32_t* temporal;
    double* tuv;
    double* corr;
    double* pose;
    double* ransac;        // [B][P][TS_MAX_SPLITS][13] split winners (key word + pose)
    double* hyp;           // [B][P][4 * n_hyp][TS_HYP_DOUBLES] P3P candidate poses (k_p3p -> k_ransac)
    int32_t* stats;
    double* state;
    const double* prior;   // [B][P][16] IMU prior of the batch (tslam_set_motion_prior) or null
    // rig: base_T_rect-left of each pair and its inverse, body-frame results
    const double* rig_E;   // [P][16]
    const double* rig_Einv;
    double* rig_pose;      // [B][68]  body T_rel, T_abs, cov
    int32_t* rig_stats;    // [B][8]
    double* rig_state;     // [32]: the rig chain's (A, Q), two row-major 4x4 (k_pose.hip blocked chain)
    double* rig_prior;     // [B][16] body-frame IMU prior (k_rig_prior, from the pairs' priors) or null
    // A4 speculative FAST threshold (DESIGN.md §5 "detect"): te[cam][l] in use, its running
    // minimum for the next batch, per (frame, cam, level) fallback flags, launch mode
    // (0: te = max(t + 1, det_thr), flags set by select; 1: te = t + 1 for flagged images only)
    const uint32_t* det_thr;      // [C][L]
    uint32_t* det_thr_acc;        // [C][L]
    uint32_t* det_fail;           // [B][C][L]
    uint32_t* match_cnt;          // [16] k_match path counters (tslam_match_counters) or null
    uint32_t* det_cnt;            // [TS_MAX_LEVELS][TS_DCNT] k_detect round counters (tslam_detect_counters) or null

    const uint32_t* brief_table;  // [30][256] LDS patch byte offsets of the two points (lo | hi << 16)
    const int64_t* wedges;        // [31][2]
    PairCalib calib[8];
    MatchParams mp;
    PoseParams pp;
    int fast_threshold, margin;
    int dt_list_cap;       // k_describe: y-sorted positions listed at a time, 1 .. TS_DT_LIST (tslam_describe_mode)
};

static inline __host__ __device__ int ring_slot(const BatchCtx& c, int64_t g) { return (int)(g % c.R); }
// The host side of batch_slot and div_small below: the batch's first frame with its ring slot, the
// view's camera and pair counts with their reciprocals.
static inline uint32_t small_rcp(int d) { return d > 1 ? (uint32_t)((1ull << 32) / (uint32_t)d) + 1u : 0u; }
static inline void ctx_set_first_frame(BatchCtx& c, int64_t g0) {
    c.g0 = g0;
    c.slot0 = ring_slot(c, g0);
}
static inline void ctx_set_views(BatchCtx& c, int cam0, int ncam, int pair0, int npair) {
    c.cam0 = cam0, c.ncam = ncam, c.pair0 = pair0, c.npair = npair;
    c.ncam_rcp = small_rcp(ncam), c.npair_rcp = small_rcp(npair);
}
#ifdef __HIPCC__
// Ring slot of frame f of the batch (0 <= f < n <= R) without the 64-bit modulo, and of the frame
// before the frame in `slot`.
__device__ __forceinline__ int batch_slot(const BatchCtx& c, int f) {
    const int s = c.slot0 + f;
    return s >= c.R ? s - c.R : s;
}
__device__ __forceinline__ int prev_slot(const BatchCtx& c, int slot) { return slot > 0 ? slot - 1 : c.R - 1; }
// a / d for a, d >= 1 with a * d < 2^32, `rcp` = small_rcp(d) = (2^32 + e) / d with 1 <= e <= d: the
// multiply-high is floor(a / d + a e / (2^32 d)), whose second term stays below 1 / d
__device__ __forceinline__ int div_small(int a, uint32_t rcp) { return rcp ? (int)__umulhi((uint32_t)a, rcp) : a; }
#endif

// sharded rig: frame ranges of the ranks (tslam_ranges.h)
#include "tslam_ranges.h"
// front-end image index (f * ncam + view camera) -> frame, rig camera; in the peer layout the
// index runs over (peer, frame, camera) of the world-1 peers
__device__ __forceinline__ void view_image(const BatchCtx& c, int img, int* f, int* cam) {
    if (c.peer_S) {
        const int per = c.n * c.peer_S, qq = img / per, q = qq < c.peer_me ? qq : qq + 1;
        const int r = img - qq * per;
        *f = r / c.peer_S;
        *cam = q * c.peer_S + (r - *f * c.peer_S);
        return;
    }
    *f = div_small(img, c.ncam_rcp);
    *cam = c.cam0 + (img - *f * c.ncam);
}
// the input image of view index img (its offset in c.images, in images)
__device__ __forceinline__ size_t view_src(const BatchCtx& c, int img) {
    if (c.peer_S) {
        const int per = c.n * c.peer_S, qq = img / per, q = qq < c.peer_me ? qq : qq + 1;
        const int r = img - qq * per, f = r / c.peer_S;
        return ((size_t)q * c.peer_nbuf + c.peer_skip + f) * c.peer_S + (r - f * c.peer_S);
    }
    return (size_t)img;
}

// host launchers (one per stage kernel set)
void launch_rectify_pyramid(const BatchCtx& c, hipStream_t s);
void launch_detect(const BatchCtx& c, hipStream_t s);
void launch_select(const BatchCtx& c, hipStream_t s, int mode, int rcap);   // tslam_select_mode
void launch_describe(const BatchCtx& c, hipStream_t s);
void launch_match(const BatchCtx& c, hipStream_t s);
int match_blocks_per_cu();   // k_match blocks the runtime places on a CU (tslam_match_counters)
void launch_match_refine(const BatchCtx& c, hipStream_t s);
void launch_match_stereo(const BatchCtx& c, hipStream_t s);
void launch_pose(const BatchCtx& c, hipStream_t s);
void launch_chains(const BatchCtx& c, bool rig, hipStream_t s);   // every pair's chain (+ the rig's)
void launch_rig_pose(const BatchCtx& c, hipStream_t s);
// sharded rig exchange (k_exchange.hip): stream blocks (per frame x camera) and pose records (per frame)
int64_t stream_block_bytes(const LevelGeom& g);
int64_t pose_record_bytes(int P);
void launch_stream_blocks(const BatchCtx& c, bool pack, int64_t first, int n_frames, int cam_lo, int ncam, uint8_t* blk,
                          hipStream_t s);
// all peers at once (alltoall layout [world][cap][S][block], cap = peer_cap): pack this rank's
// cameras of every peer q's frames lo_q - 1 .. hi_q - 1 (slot q), or unpack every peer's cameras
// of frames lo_me - 1 .. hi_me - 1 (slot q <- cameras q*S ..); slot `me` untouched
void launch_stream_blocks_peers(const BatchCtx& c, bool pack, int64_t g0, int n, int world, int cap, int me, int S,
                                uint8_t* blk, hipStream_t s);
void launch_stage_raw_peers(const uint8_t* images, const uint8_t* prev, uint8_t* dst, int n, int world, int cap, int me,
                            int S, int64_t img_bytes, hipStream_t s);
void launch_pose_records(const BatchCtx& c, bool pack, int f0, int n, uint8_t* rec, hipStream_t s);
// every frame of the batch from the all-gather's padded layout [world][peer_records][record]
// (`pairs`: rank q's slot holds rig range rig_slot(q), tslam_ranges.h)
void launch_pose_records_gathered(const BatchCtx& c, int world, bool pairs, const uint8_t* rec, hipStream_t s);
// state blocks a sharded rank sends to rank 0 so that rank 0's ring holds what local BA, loop
// closure and relocalisation read (k_exchange.hip): per (frame of the sender's range, pair) the
// temporal matches + refined disparities, per (batch frame, left camera of the sender's streams)
// keypoints + level counts + descriptors; pack on the sender, unpack on rank 0 (per sender)
int64_t state_range_block_bytes(const LevelGeom& g);
int64_t state_camera_block_bytes(const LevelGeom& g);
void launch_state_blocks(const BatchCtx& c, bool pack, int n, int world, int rank, int cam_lo, int cam_hi, uint8_t* blk,
                         hipStream_t s);
// camera-sharded RGB-D rig: pair blocks (per batch frame x pair: pose, stats, correspondences)
int64_t pair_block_bytes(const LevelGeom& g);
void launch_pair_blocks(const BatchCtx& c, bool pack, int f0, int n_frames, int p0, int np, uint8_t* blk, hipStream_t s);
void launch_pose_solve(const BatchCtx& c, hipStream_t s);
void launch_perturb_uv(const BatchCtx& c, int percent, uint64_t seed, hipStream_t s);   // benchmark hook
void launch_reloc(const BatchCtx& c, int pair, int64_t frame, const double* map_xyz, const uint32_t* map_desc, int M,
                  int32_t* match, double* corr, int32_t* stats, double* pose, double* ransac, double* hyp, hipStream_t s);
void launch_reloc_rig(const BatchCtx& c, int64_t frame, const double* map_xyz, const uint32_t* map_desc, int M,
                      int32_t* match, double* corr, int32_t* stats, double* pose, double* ransac, double* hyp,
                      double* rig_pose, int32_t* rig_stats, hipStream_t s);
// relocalisation query image: keypoint records [K][2], level counts [L], descriptors [K][8] of one
// camera image (a ring slot's, or a keyframe database entry's snapshot)
struct RelocQuery {
    const uint32_t* kps;
    const int32_t* kcount;
    const uint32_t* desc;
};
static inline RelocQuery reloc_query_ring(const BatchCtx& c, int cam, int64_t frame) {
    const size_t ib = (size_t)ring_slot(c, frame) * c.C + cam;
    return {c.kps + ib * c.g.K * 2, c.kcount + ib * c.g.n_levels, c.desc + ib * c.g.K * 8};
}
// `dM` (device, may be null): the map size read on the device instead of M
void launch_reloc_query(const BatchCtx& c, int pair, int64_t frame, RelocQuery q, const double* map_xyz,
                        const uint32_t* map_desc, int M, const int32_t* dM, int32_t* match, double* corr, int32_t* stats,
                        double* pose, double* ransac, double* hyp, hipStream_t s);
// keyframe database (tslam_loop_*): entry e holds landmarks xyz [K][3] + desc [K][8] + count, and
// the snapshot of its image (kps [K][2], kcount [TS_MAX_LEVELS], desc [K][8])
struct LoopDb {
    double* xyz;
    uint32_t* desc;
    int32_t* n;
    uint32_t* snap_kps;
    int32_t* snap_kcount;
    uint32_t* snap_desc;
};
void launch_loop_store(const BatchCtx& c, int pair, int64_t frame, double* xyz, uint32_t* desc, int32_t* n_out,
                       hipStream_t s);
void launch_loop_store_auto(const BatchCtx& c, int interval, const LoopDb& db, int capk, bool rig, int64_t* count,
                            hipStream_t s);
void launch_loop_vote(const uint32_t* db_desc, const int32_t* db_n, int K, int S, int q_slot, int64_t k0, int capk, int P,
                      int n_cand, int max_hamming, int ratio_pct, int32_t* votes, hipStream_t s);
void launch_pose_graph_iteration(double* T, const int32_t* edges, const double* Z, const double* info, int N, int E,
                                 const int32_t* adj_off, const int32_t* adj, const int32_t* ftile, double* terms,
                                 double* H, double* g, double* delta, double* Ld, hipStream_t s);
// test hook: blocks >= 1 of every k_pg_potrf launch sleep `spins` x 127 x 64 cycles first
void pose_graph_test_delay(int spins);
void launch_pose_graph_cost(const double* T, const int32_t* edges, const double* Z, const double* info, int E,
                            double* terms, double* cost, hipStream_t s);
// TSDF volume + one integration launch (k_tsdf.hip)
#define TSDF_MAX_FRAMES 256
#define TSDF_POSE 13   // R (9), t (3), use flag: cam_T_world for integration, world_T_cam (t = the centre) for rendering
struct TsdfArgs {
    float* tsdf;
    float* weight;
    int nx, ny, nz;
    double ox, oy, oz, s;
    double trunc, max_dist, max_weight;
    const uint8_t* depth;      // frame 0's depth (u16 mm), frames `stride` bytes apart
    int64_t stride;
    int n;                     // frames
    int W, H;
    double fx, fy, cx, cy;
    const int32_t* map;        // [H][W][2] undistortion table (fixed point, 5 bits) or null
    const double* poses;       // [n][TSDF_POSE]
    // colour layer (null when off): frame 0's BGR image (frames `color_stride` bytes apart, below),
    // the running colour [nv][3] (R, G, B) f32 and its weight f32
    const uint8_t* color;
    float* col;
    float* col_w;
    // colour with a stride of its own and a visibility mask (tslam_tsdf_integrate_rect_color: colour
    // registered to the depth, thor_slam_amd/depth_register.py): color_stride 0 = `stride`; mask u8
    // [H][W] per frame, mask_stride bytes apart: a voxel's colour is updated only where the sampled
    // pixel's mask is non-zero; null = every pixel
    int64_t color_stride;
    const uint8_t* mask;
    int64_t mask_stride;
    // the rolling window's record (null: the volume's corner is ox, oy, oz as they stand; else the
    // corner is o + s * (double)win->shift[a], thor_slam_amd/dense_follow.py)
    const struct TsdfWindow* win;
};
// The rolling window (thor_slam_amd/dense_follow.py): the cumulative shift of the volume in whole
// voxels, and the move the current call makes (delta; all zero: none).  Written on the device
// (k_tsdf_follow, k_tsdf_shift), read by the move and by k_tsdf_integrate.
struct TsdfWindow {
    int32_t shift[3];
    int32_t delta[3];
};
#define TSDF_SHIFT_LIMIT (1 << 30)   // |shift|, |delta| and the camera's voxel index stay below it
struct TsdfFollow {
    int32_t anchor[3];
    int32_t margin, step;
};
// the layers of a volume as the move sees them: rows of nx * comp floats, ny * nz rows per layer
struct TsdfLayers {
    float* vol[5];       // tsdf, weight, colour weight and colour, the free-space words (moved as bits)
    float* scratch[5];
    int comp[5];
    int n;
    int nx, ny, nz;
};
// follow: the decision of an integrate call from the pose table of its first chunk (n entries);
// shift: the same two fields from a caller's delta
void launch_tsdf_follow(const double* poses, int n, const TsdfArgs& a, const TsdfFollow& f, TsdfWindow* win, hipStream_t s);
void launch_tsdf_shift(TsdfWindow* win, int dx, int dy, int dz, hipStream_t s);
// The brick store (thor_slam_amd/dense_store.py; k_tsdf_store.hip): what leaves the window goes
// into a pool of 8 x 8 x 8 bricks behind a hash table of absolute brick coordinates, what enters
// comes back from it.  All of it lives on the device; the host only keeps the pointers.
struct TsdfStoreCounters {
    unsigned long long dropped;   // leaving non-zero voxels that found no brick
    unsigned long long moves;     // moves (delta != 0) the store has seen
    int32_t bricks;               // slots handed out (never above capacity once a kernel has ended)
    int32_t pad;
};
struct TsdfStore {
    unsigned long long* keys;     // [cells] tslam_tsdf_store.h's keys, 0 = empty
    int32_t* vals;                // [cells] the key's slot
    int32_t* occ;                 // [capacity] voxels the slot's brick holds
    uint32_t* pool;               // [capacity] bricks: per layer [8][8][8][comp] words
    TsdfStoreCounters* ctr;
    int32_t capacity;
    uint32_t mask;                // cells - 1
    int32_t wpv;                  // words per voxel the pool's bricks were sized for
};
// move: the volume through the scratch and back; with a store, k_tsdf_store_out before and
// k_tsdf_store_in after the two launches
void launch_tsdf_move(const TsdfLayers& l, const TsdfWindow* win, hipStream_t s, const TsdfStore* store = nullptr);
void launch_tsdf_store_out(const TsdfLayers& l, const TsdfWindow* win, const TsdfStore& st, hipStream_t s);
void launch_tsdf_store_in(const TsdfLayers& l, const TsdfWindow* win, const TsdfStore& st, hipStream_t s);
// The mesh of the whole map (thor_slam_amd/dense_store.py; k_tsdf_store_mesh.hip): marching cubes over
// the window and the store together, one block per listed store brick.  o is the configured,
// unshifted origin; the kernels read the window's shift from the record.
struct WmeshArgs {
    const float* tsdf;         // the window's layers [nz][ny][nx]
    const float* weight;
    const float* color;        // [nz][ny][nx][3] or null (no vertex colours)
    int nx, ny, nz;
    double ox, oy, oz, s;
    float sf, min_weight;
    const TsdfWindow* win;
    TsdfStore st;
};
// list: the keys of the bricks to visit, unsorted, *count of them (beyond `cap` nothing is written)
void launch_wmesh_list(const WmeshArgs& a, int64_t cells, int64_t max_window, uint64_t* list, int64_t cap, uint32_t* count, hipStream_t s);
void launch_wmesh_count(const WmeshArgs& a, const uint64_t* list, int64_t n_bricks, uint32_t* block_sums, hipStream_t s);
void launch_wmesh_emit(const WmeshArgs& a, const uint64_t* list, int64_t n_bricks, const uint64_t* block_off, float* tris, float* cols,
                       int64_t cap, hipStream_t s);
// what a call's first chunk does between its poses and its integration when the window follows
struct TsdfFollowCall {
    TsdfFollow f;
    TsdfLayers l;
    TsdfWindow* win;
    const TsdfStore* store = nullptr;   // the brick store, when it is on
};
void launch_tsdf(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfArgs& a, double* poses,
                 hipStream_t s, const TsdfFollowCall* follow = nullptr);
// The rig's launch: every selected camera of every frame in one read-modify-write of the volume.
// View v = f * n_cams + ci (frame-major, camera-minor) is integrated in ascending v, on the rig's
// body pose: world_T_cam = (E_0^-1 T_abs(f)) E_pair.  TsdfArgs' n counts VIEWS here, and its depth /
// color / stride / map / intrinsics are unused: they come from the view's camera record.
#define TS_RIG_MAXP 8   // pairs of a rig (tslam_create: n_pairs <= 8)
struct TsdfRigCam {
    const uint8_t* depth;      // this camera's frame 0 (u16 mm), frames `stride` bytes apart
    const uint8_t* color;      // BGR u8, frames `color_stride` apart (null: TsdfArgs::col is null too)
    const int32_t* map;        // the raw camera's undistortion table, or null (rectified depth)
    int64_t stride;
    double fx, fy, cx, cy;
    int64_t color_stride;      // 0 = `stride`
    const uint8_t* mask;       // as TsdfArgs::mask, or null
    int64_t mask_stride;
};
struct TsdfRigArgs : TsdfArgs {
    int n_cams;
    TsdfRigCam cams[TS_RIG_MAXP];
};
// pairs: 8 bits per camera, camera ci's pair in bits 8 ci .. 8 ci + 7; f0: first frame within the batch
// (device poses); host_wTb_dev: staged world_T_base [n_frames][16] or null
void launch_tsdf_rig(const BatchCtx& c, uint64_t pairs, int f0, const double* host_wTb_dev, const TsdfRigArgs& a,
                     double* poses, hipStream_t s, const TsdfFollowCall* follow = nullptr);
// The volume seen from a pose (k_tsdf_render.hip; thor_slam_amd/dense_render.py): n_views images of
// one pinhole camera.  Outputs [views][H][W] (normal and color x 3); a null output is not written.
struct TsdfRenderArgs {
    const float* tsdf;
    const float* weight;
    const float* col;          // the colour layer [nv][3] (R, G, B) and its weight, or null
    const float* col_w;
    int nx, ny, nz;
    double ox, oy, oz, s;
    const TsdfWindow* win;     // as TsdfArgs::win
    int W, H;
    double fx, fy, cx, cy;
    double min_weight, min_depth, max_depth, step_scale;
    const double* L;           // [H][W] metres per unit of depth along the pixel's ray (host table)
    const double* poses;       // [views][TSDF_POSE]: world_T_cam R rows (9), centre (3), use flag
    float* depth_m;
    uint16_t* depth_mm;
    float* normal;
    uint8_t* color;
};
// pair, f0, host_wTc_dev as launch_tsdf; poses: the call's table, written by its pose kernel
void launch_tsdf_render(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfRenderArgs& a, int n_views,
                        double* poses, hipStream_t s);
// Dense frame-to-model alignment (k_tsdf_align.hip; thor_slam_amd/dense_align.py): n frames of one
// camera against the model images rendered at their initial poses.
#define ALIGN_TERMS 29   // J J^T upper (21), -J r (6), sum r^2, inliers
#define ALIGN_PART 32    // doubles per block partial
#define ALIGN_STATE 32   // doubles per frame: T = R rows (9), C (3); T0 alike (12); the active flag [24]
#define ALIGN_STATS 4    // status, iterations run, inliers of the first and of the last iteration
struct TsdfAlignArgs {
    const uint8_t* depth;      // frame 0's depth (u16 mm), frames `stride` bytes apart
    int64_t stride;
    int n;                     // frames
    int W, H;
    double fx, fy, cx, cy;
    const int32_t* map;        // as TsdfArgs::map
    double max_dist;           // the volume's
    const float* depth_m;      // the model images at T0: [n][H][W] and [n][H][W][3]
    const float* normal;
    const double* poses;       // the render's table at T0 [n][TSDF_POSE]
    double max_distance2, eps_t2, eps_r2, max_t2, rot_lim, min_pivot;   // squares; rot_lim = 1 + 2 cos(max_rotation)
    int min_inliers, iterations;
    int pblocks;               // blocks of a view padded to a power of two >= 256
    double* state;             // [n][ALIGN_STATE]
    double* partial;           // [n][pblocks][ALIGN_PART]; blocks past the view's stay zero
    double* wTc;               // out: world_T_cam [n][16]
    int32_t* stats;            // out: [n][ALIGN_STATS]
    double* resid;             // out: rms of the first and of the last iteration [n][2]
    double* neq;               // out: the 28 sums of the last executed iteration [n][28]
};
// the render at T0 (r: the align state's own images and ray-length table; pair, f0, host_wTc_dev
// and poses as launch_tsdf_render), then a.iterations x (accumulate, solve)
void launch_tsdf_align(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfRenderArgs& r,
                       const TsdfAlignArgs& a, double* poses, hipStream_t s);
// the aligned poses as the integrator's table
void launch_align_poses(const double* wTc, const int32_t* stats, int n, double* out, hipStream_t s);
// The free-space depth mask (k_tsdf_dynamic.hip; thor_slam_amd/dense_dynamic.py): n frames of one
// camera against the volume as the stream finds it; depth that lands in voxels seen free is masked.
#define DYNAMIC_STATS 4      // status (0 OK, 1 UNUSED), valid pixels, candidates, valid pixels under the mask
#define DYNAMIC_MAX_OPEN 4   // open_radius and dilate_radius at most: the clean-up reaches 2 * 4 + 8 = 16 < 64 bits
#define DYNAMIC_MAX_DILATE 8
struct TsdfDynamicArgs {
    const float* tsdf;
    const float* weight;
    int nx, ny, nz;
    double ox, oy, oz, s;
    const TsdfWindow* win;     // as TsdfArgs::win
    const uint8_t* depth;      // frame 0's depth (u16 mm), frames `stride` bytes apart
    int64_t stride;
    int n;                     // frames
    int W, H;
    double fx, fy, cx, cy;
    const int32_t* map;        // as TsdfArgs::map
    double max_dist;           // the volume's
    double min_free_weight, thr;   // thr = free_fraction * trunc, rounded once on the host
    const uint32_t* layer;     // the free-space words [nz][ny][nx] (a settled voxel is no candidate), or null
    int open_radius, dilate_radius;
    const double* poses;       // [n][TSDF_POSE]: world_T_cam R rows (9), centre (3), use flag
    uint64_t* bits;            // scratch: per (frame, row, 64 columns) the candidates' word and the valid pixels' word
    uint16_t* out_depth;       // out: [n][H][W]
    uint8_t* out_mask;         // out: [n][H][W]
    int32_t* stats;            // out: [n][DYNAMIC_STATS]
};
// pair, f0, host_wTc_dev and poses as launch_tsdf_render
void launch_tsdf_dynamic(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfDynamicArgs& a,
                         double* poses, hipStream_t s);
// The free-space layer's update (k_tsdf_freespace.hip; thor_slam_amd/dense_freespace.py): the used
// frames of a (depth, camera, n, stride and volume as for launch_tsdf; its tsdf / weight / colour are
// not touched) observe every voxel in frame order: occupied within `band` of the surface, free in
// front of it.  pair, f0, host_wTc_dev and poses (cam_T_world, written here by launch_tsdf_poses) as
// launch_tsdf.
#define FREESPACE_RUN_MASK 0xffffu
#define FREESPACE_SETTLED 0x10000u
void launch_tsdf_freespace(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfArgs& a, uint32_t* words,
                           double band, int settle_frames, double* poses, hipStream_t s);
// launch_tsdf's pose kernel alone (k_tsdf_poses): n entries of the integrator's table
void launch_tsdf_poses(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, int n, double* poses, hipStream_t s);
// launch_tsdf without its pose kernel: the table `poses` [a.n][TSDF_POSE] is already on the stream
void launch_tsdf_posed(const TsdfArgs& a, double* poses, hipStream_t s, const TsdfFollowCall* follow = nullptr);
// The depth archive (k_tsdf_move_frames.hip; thor_slam_amd/dense_loop.py): a ring of the depth frames
// the volume was built from, each with the very pose-table entry it was integrated on, so that a
// frame whose pose changes is taken out of the volume at its old pose and put back at the new one.
#define TSDF_MOVE_CHUNK 128   // selected frames whose two pose tables sit in LDS at a time (26 KB)
struct TsdfArchiveRec {       // written on the device only
    int64_t count;            // frames archived so far; frame number a lives in slot a % cap
    int64_t moved_total;      // frames moved since the ring was emptied
    int32_t n_sel;            // frames the last selection chose
    int32_t moved_last;       // frames the last move moved
};
struct TsdfArchive {
    uint8_t* depth;           // [cap] u16 [H][W] images, slot_stride bytes apart (a multiple of 16)
    int64_t slot_stride;
    double* pose;             // [cap][TSDF_POSE]: the entry the slot's frame is in the volume with
    double* wTc;              // [cap][16]: the same pose as world_T_cam
    int64_t* frame;           // [cap] frame ids
    int cap;
    TsdfArchiveRec* rec;
    // the last selection, in ascending archive order
    int32_t* sel_slot;        // [cap]
    double* sel_old;          // [cap][TSDF_POSE]
    double* sel_new;          // [cap][TSDF_POSE]
    double* sel_wTc;          // [cap][16]
};
struct Mat4 {
    double m[16];
};
// n frames (<= TSDF_MAX_FRAMES) of a call: entry i is frame `first_frame + i`, used only when that
// is a multiple of `interval` (>= 1) and its pose is (call_pose's flag); on device poses the entry
// is corr * T_abs (mul4_fixed's order) when has_corr.  Writes the integrator's table `poses`
// [n][TSDF_POSE] and the same poses as world_T_cam `wTc` [n][16].
void launch_tsdf_archive_poses(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, int n, int64_t first_frame,
                               int interval, bool has_corr, const Mat4& corr, double* poses, double* wTc, hipStream_t s);
// the used entries of that table into the ring, in order, with their depth images (`depth`: entry
// 0's, entries `stride` bytes apart; W * H pixels); slot_of [TSDF_MAX_FRAMES] is scratch
void launch_tsdf_archive_put(const TsdfArchive& ar, const double* poses, const double* wTc, int n, int64_t first_frame,
                             const uint8_t* depth, int64_t stride, int pixels, int32_t* slot_of, hipStream_t s);
// The move.  req_frame [n] / req_wTc [n][16] on the device: the frames asked for and their new
// world_T_cam; min_t2 = min_translation^2, rot_lim = 1 + 2 cos(min_rotation).  a: the volume and the
// archive's camera (integrate_args; depth, stride, n and poses unused).  Three launches: selection,
// k_tsdf_reintegrate over every brick (the count stays on the device), the ring's poses updated.
void launch_tsdf_archive_move(const TsdfArchive& ar, const TsdfArgs& a, const int64_t* req_frame, const double* req_wTc, int n,
                              double min_t2, double rot_lim, hipStream_t s);
// dense stereo depth (k_stereo_depth.hip): n frames of one rectified pair -> disp32 (1/32 px) and
// depth (mm), u16 [n][H][W]; win_left / win_right: u8 [n][H][W] winner maps between its two kernels
struct StereoDepthArgs {
    const uint8_t* left;       // frame 0's level-0 images (dense rows of W bytes)
    const uint8_t* right;
    int64_t stride;            // bytes between frames (ring != 0: between ring slots)
    int ring;                  // 0: frame f at f * stride; else at ((first + f) % ring) * stride
    int64_t first;
    int W, H, n;
    int n_disp, uniqueness, lr_tol;
    double fxb;
    uint16_t* depth;
    uint16_t* disp32;
    uint8_t* win_left;
    uint8_t* win_right;
};
hipError_t launch_stereo_depth(const StereoDepthArgs& a, hipStream_t s);
// semi-global aggregation (k_sd_sgm.hip; rule 3a of thor_slam_amd/stereo_depth.py): the same n
// frames through volume -> path sums -> winners -> k_sd_finish.  vol and sum are scratch, u16
// [n][H][W][sd_sgm_pitch(n_disp)] each (d contiguous); paths is the bit mask of rule 3a.
struct StereoSgmArgs {
    int p1, p2, paths;
    uint16_t* vol;
    uint16_t* sum;
};
static inline int sd_sgm_pitch(int n_disp) { return (n_disp + 3) & ~3; }
hipError_t launch_stereo_depth_sgm(const StereoDepthArgs& a, const StereoSgmArgs& g, hipStream_t s);
// the box matcher's kernels as stages of the semi-global one (k_stereo_depth.hip)
hipError_t launch_sd_volume(const StereoDepthArgs& a, uint16_t* vol, int pitch, hipStream_t s);
hipError_t launch_sd_finish(const StereoDepthArgs& a, hipStream_t s);
// post-filters (k_sd_filter.hip; rules 9 and 10 of thor_slam_amd/stereo_depth.py) on n dense frames
// of disp32, in place, then rule 8's depth.  median 0 / 3 / 5 / 7, speckle_size 0 = off.  tmp: u16
// [n][H][W], the median's output (unused without it); label, count: u32 [n][H][W] each (unused
// without the speckle filter).
struct StereoFilterArgs {
    int W, H, n;
    double fxb;
    int median, speckle_size, speckle_range;
    uint16_t* disp32;
    uint16_t* depth;
    uint16_t* tmp;
    uint32_t* label;
    uint32_t* count;
};
hipError_t launch_sd_filter(const StereoFilterArgs& a, hipStream_t s);
// n values of a caller's disp32 plane into dst, clamped to 8191
hipError_t launch_sd_filter_load(const uint16_t* src, uint16_t* dst, size_t n, hipStream_t s);
// depth registration (k_depth_register.hip; thor_slam_amd/depth_register.py): n frames of depth of a
// W x H pinhole camera forward-warped into a Wc x Hc colour camera through a z-buffer
struct DepthRegArgs {
    int W, H, Wc, Hc, n;
    double fx, fy, cx, cy;     // the depth camera
    double fc, cxc, cyc;       // the undistorted colour camera
    double T[12];              // color_T_rect, 3 x 4 row-major
    int max_depth_mm, tol_mm, max_splat;
    const int32_t* map;        // [Hc][Wc][2] undistorted -> raw colour pixel (fixed point, 5 bits) or null
    const uint8_t* depth;      // frame 0's depth (u16 mm, dense rows), frames depth_stride bytes apart
    int64_t depth_stride;
    const uint8_t* color;      // frame 0's raw BGR image [Hc][Wc][3], frames color_stride bytes apart
    int64_t color_stride;
    uint32_t* zbuf;            // [n][Hc][Wc] scratch
    uint16_t* reg;             // [n][Hc][Wc] registered depth (mm)
    uint8_t* bgr;              // [n][H][W][3] colour registered to the depth
    uint8_t* mask;             // [n][H][W] 1 = seen by the colour camera
};
// clear, splat, gather on the stream; ev (4 events) non-null: recorded before, between and after them
hipError_t launch_depth_register(const DepthRegArgs& a, hipStream_t s, hipEvent_t* ev = nullptr);
// dense-map outputs of the TSDF volume (k_dense.hip): marching-cubes mesh, capped exact ESDF
struct DenseArgs {
    const float* tsdf;
    const float* weight;
    int nx, ny, nz;
    uint32_t n_cubes;          // (nx - 1)(ny - 1)(nz - 1)
    int64_t n_voxels;
    double ox, oy, oz, s;      // volume corner and voxel size (voxel centres in f64, rounded to f32)
    float sf;                  // (float)s
    float min_weight;          // observed: weight >= min_weight
    float site_dist;           // ESDF site: |tsdf| <= site_dist
    float max_dist;            // ESDF value beyond R voxels
    int32_t cap;               // R^2 + 1
    const float* color;        // mesh: the colour layer [nv][3] or null (no vertex colours)
};
void launch_mesh_count(const DenseArgs& a, uint8_t* cfg, uint32_t* block_sums, uint64_t* block_off, uint64_t* total,
                       hipStream_t s);
// k_mesh_scan alone: block_off[b] = sum of block_sums[0..b), *total = the sum of all
void launch_mesh_scan(const uint32_t* block_sums, int nb, uint64_t* block_off, uint64_t* total, hipStream_t s);
void launch_mesh_emit(const DenseArgs& a, const uint8_t* cfg, const uint64_t* block_off, float* tris, float* cols,
                      int64_t cap, hipStream_t s);
void launch_esdf(const DenseArgs& a, int R, const float* tab, int32_t* g0, int32_t* g1, float* out, hipStream_t s);
void launch_esdf_slice(const DenseArgs& a, int y0, int y1, int R, const float* tab, int32_t* g0, int32_t* g1,
                       uint8_t* obs, float* out, hipStream_t s);
void launch_rgbd_gray(const BatchCtx& c, uint8_t* gray, hipStream_t s);
void launch_rgbd_depth(const BatchCtx& c, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_lane() { return threadIdx.x & 63; }

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// Wave-uniform minimum via DPP row reductions (quad perms, half-row and row mirrors: VALU
// latency, no LDS crossbar) and four readlanes.  Requires all 64 lanes active.
__device__ __forceinline__ uint32_t wave_min_dpp(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, false));  // row_mirror
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// Wave-uniform sum via the same DPP row reduction (result in an SGPR).
__device__ __forceinline__ int wave_sum_dpp(int v) {
    // old = 0 (the identity) lets each step fuse into one v_add_u32_dpp; after the 4 row steps
    // every lane holds its row's sum, row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3) fold
    // the rows into lane 63 — 6 VALU + 1 readlane instead of 4 DPP moves, 4 adds and 4 readlanes
    // (exact: integer sums, every lane of the wave active)
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
    return __builtin_amdgcn_readlane(v, 63);
}

// f64 DPP move (both halves) for the row reductions below.
__device__ __forceinline__ double dpp_f64(double v, int ctrl_sel) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    int lo = (int)(uint32_t)b, hi = (int)(uint32_t)(b >> 32);
    switch (ctrl_sel) {   // constant after inlining
        case 0: lo = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, false); break;
        case 1: lo = __builtin_amdgcn_mov_dpp(lo, 0x4E, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0x4E, 0xF, 0xF, false); break;
        case 2: lo = __builtin_amdgcn_mov_dpp(lo, 0x141, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0x141, 0xF, 0xF, false); break;
        default: lo = __builtin_amdgcn_mov_dpp(lo, 0x140, 0xF, 0xF, false); hi = __builtin_amdgcn_mov_dpp(hi, 0x140, 0xF, 0xF, false); break;
    }
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
// f64 DPP move with a compile-time control (e.g. quad_perm broadcasts 0x00/0x55/0xAA/0xFF).
template <int CTRL>
__device__ __forceinline__ double dpp_f64c(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)b, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// Wave-uniform f64 sum: DPP row reductions (no LDS crossbar) + four readlanes.  Requires all 64
// lanes active.  The summation order is fixed (deterministic run to run).
__device__ __forceinline__ double wave_sum_f64(double v) {
    v = v + dpp_f64(v, 0);
    v = v + dpp_f64(v, 1);
    v = v + dpp_f64(v, 2);
    v = v + dpp_f64(v, 3);
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// Wave sums of N <= 32 f64 values at once (a transposing butterfly): at the exchange with lane
// distance d = 32, 16, .., 2 every lane keeps half of its values (the upper half when lane & d)
// and adds its partner's copy of that half, so value k ends in lanes 2k and 2k + 1 after a last
// exchange at distance 1.  31 shuffles for 32 values instead of 32 separate reductions; a fixed
// order, so deterministic.  Returns the sum of value lane >> 1 (lanes past 2N hold zeros).
template <int N>
__device__ __forceinline__ double wave_multi_sum(const double (&in)[N]) {
    static_assert(N <= 32, "at most 32 values");
    double v[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) v[k] = k < N ? in[k] : 0.0;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int h = 16; h >= 1; h >>= 1) {   // values per lane after this exchange
        const int d = 2 * h;              // lane distance 32, 16, 8, 4, 2
        const bool upper = (lane & d) != 0;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const double keep = upper ? v[h + j] : v[j];
            const double send = upper ? v[j] : v[h + j];
            v[j] = keep + __shfl_xor(send, d, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

// XCD-aware 1-D block mapping: blocks are dealt round-robin over the 8 XCDs, so block b runs on the
// XCD labelled b % 8.  Give all `bpi` blocks of one image the same label, so that image's pyramid
// lines are fetched into one L2 only.  Speed only: correctness never depends on placement.
// Launch with xcd_grid(n_img, bpi) blocks (xcd_grid3 below: the same order without the divisions); returns
// false for the padding blocks.
static inline __host__ int xcd_grid(int n_img, int bpi) { return ((n_img + 7) / 8) * 8 * bpi; }
__device__ __forceinline__ bool xcd_image_block(int b, int n_img, int bpi, int* img, int* local) {
    const int k = b >> 3;
    *img = (k / bpi) * 8 + (b & 7);
    *local = k % bpi;
    return *img < n_img;
}
// The same mapping as a 3-D grid (8, bpi, image groups): the linear workgroup order, hence the XCD
// of every block, is xcd_grid's, and the block reads its image and local index from its
// coordinates with no division.  Grids whose y or z extent would pass 65,535 stay 1-D (x only).
static inline __host__ dim3 xcd_grid3(int n_img, int bpi) {
    const int groups = (n_img + 7) / 8;
    return bpi <= 65535 && groups <= 65535 ? dim3(8, bpi, groups) : dim3(xcd_grid(n_img, bpi));
}
__device__ __forceinline__ bool xcd_image_block3(int n_img, int bpi, int* img, int* local) {
    // a 1-D grid has gridDim.y = 1 != bpi; with bpi = 1 the two decodes agree (blockIdx.z = 0, img = blockIdx.x)
    if ((int)gridDim.y != bpi) return xcd_image_block(blockIdx.x, n_img, bpi, img, local);
    *img = blockIdx.z * 8 + blockIdx.x;
    *local = blockIdx.y;
    return *img < n_img;
}

// The use flag of the pose record of frame f0 + i of the batch from its status: tracked, or the
// global first frame
__device__ __forceinline__ double pose_used(const BatchCtx& c, int st, int f0, int i) {
    return (st == 0 || (st == 2 && c.g0 + f0 + i == 0)) ? 1.0 : 0.0;
}

// The pose of entry i of a call and its use flag: the host's world_T_cam [n][16] (a NaN pose is
// not used), or T_abs of `pair` at frame f0 + i of the batch with its status' flag.
__device__ __forceinline__ const double* call_pose(const BatchCtx& c, int pair, int f0, const double* host_wTc, int i,
                                                   double* use) {
    if (host_wTc) {
        const double* T = host_wTc + 16 * (size_t)i;
        *use = __builtin_isfinite(T[0]) ? 1.0 : 0.0;
        return T;
    }
    const size_t o = (size_t)(f0 + i) * c.P + pair;
    const double* T = c.pose + o * TS_POSE_DOUBLES + 16;
    const int st = c.stats[o * TS_STATS_INTS];
    *use = pose_used(c, st, f0, i);
    return T;
}

// world_T_cam T (4 x 4, row-major) inverted into a TSDF_POSE entry: R^T (9) and -R^T t (3), the
// integrator's cam_T_world; the use flag q[12] is the caller's
__device__ __forceinline__ void store_cam_T_world(const double* T, double* q) {
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) q[3 * r + k] = T[4 * k + r];   // R^T
        q[9 + r] = -((T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]);
    }
}

// Level of y-sorted position `pos` (levels are laid out back to back, koff[l] .. koff[l+1]).
__device__ __forceinline__ int pos_level(const LevelGeom& g, int pos) {
    int l = 0;
    while (l + 1 < g.n_levels && pos >= g.koff[l + 1]) ++l;
    return l;
}
