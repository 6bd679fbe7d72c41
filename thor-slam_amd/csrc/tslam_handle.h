// tslam_handle.h — the handle behind the C-ABI and what the host files of the library share to
// work on it.  Host only: no .hip file includes it.
//
// The fields of tslam_handle are ordered by the file that owns them ("host sources"):
// a field is written by its owner and by tslam_create; other files go through the helpers
// declared at the end.  Every helper is TSLAM_INTERNAL: none reaches the dynamic symbol table.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tslam.h"
#include "tslam_ba.h"
#include "tslam_common.h"
#include "tslam_internal.h"

struct Buffer {
    void* ptr = nullptr;
    int64_t bytes = 0;
    int64_t per_frame = 0;
};

struct tslam_handle {
    // ---- tslam_api.cpp: geometry, workspace, the current batch, rig, motion prior, host boundary ----
    int device = 0;
    tslam_params prm{};
    int W = 0, H = 0, P = 0, C = 0, B = 0, R = 0;
    LevelGeom g{};
    PairCalib calib[8]{};
    uint32_t map_mask = 0;
    int32_t* d_maps = nullptr;
    uint32_t* d_brief = nullptr;
    int64_t* d_wedges = nullptr;
    uint32_t* d_dt_tile = nullptr;   // describe tile table (describe_tile_table)
    uint8_t* d_gray = nullptr;   // RGB-D: converted colour images [B][P][H][W]
    Buffer buf[TSLAM_BUF_COUNT];
    uint32_t* d_cand = nullptr;
    uint32_t* d_ccount = nullptr;
    uint32_t* d_det_thr_acc = nullptr;   // [C][L] running minimum of the next te
    uint32_t* d_hist = nullptr;
    double* d_state = nullptr;
    double* d_ransac = nullptr;
    double* d_hyp = nullptr;
    int64_t frames_done = 0;
    // current batch
    const uint8_t* cur_images = nullptr;
    int cur_n = 0;
    int64_t cur_g0 = 0;
    bool in_batch = false;
    int64_t batch_idx = 0;   // batches ended; its parity picks the slot of everything kept per two batches
    bool batch_started = false;
    hipStream_t last_stream = nullptr;
    std::vector<void*> allocs;
    std::vector<void*> host_allocs;
    // front (rectify .. describe) and back (match .. chain) stages on two streams: batch s's back
    // waits for its front; batch s's front waits for the back of batch s - 2 (shared ring slots)
    hipStream_t front_stream = nullptr, back_stream = nullptr;
    bool front_started = false, back_started = false;
    hipEvent_t ev_front = nullptr, ev_back[2] = {nullptr, nullptr};
    bool back_pending[2] = {false, false};
    // rig pose (tslam_set_rig): E = base_T_rect-left per pair, its inverse, body-frame results
    bool rig = false;
    int rig_q = 0, rig_cap = 0;   // E entries set; allocated
    double* d_rig_E = nullptr;
    double* d_rig_pose = nullptr;
    int32_t* d_rig_stats = nullptr;
    double* d_rig_state = nullptr;
    // IMU rotation prior for the next batch (tslam_set_motion_prior); the rig's body-frame
    // version of it (k_rig_prior), per batch parity
    double* d_prior = nullptr;
    double* d_rig_prior = nullptr;
    hipEvent_t ev_prior[2] = {nullptr, nullptr};   // the last reader of each prior slot is done
    bool prior_read_armed[2] = {false, false};
    bool prior_armed = false;
    double* h_prior_pin[2] = {nullptr, nullptr};   // pinned staging of each parity's prior slot
    bool prior_copy_pending = false;               // copied on the batch's back stream at its first back stage
    // asynchronous host boundary (tslam_submit_host / tslam_poll_*): the handle's own front/back
    // streams, pinned staging + device input per batch parity, pinned result slots per parity
    hipStream_t as_front = nullptr, as_back = nullptr;
    hipStream_t as_ba = nullptr;      // local BA (ba_window > 0): its own stream on every CU
    uint8_t* as_stage[2] = {nullptr, nullptr};   // pinned host
    uint8_t* as_input[2] = {nullptr, nullptr};   // device
    hipEvent_t as_staged[2] = {nullptr, nullptr};   // DMA out of as_stage[k] done
    bool as_staged_armed[2] = {false, false};
    struct ResultSlot {
        double* pose = nullptr;       // pinned [B][P][68]
        int32_t* stats = nullptr;     // pinned [B][P][8]
        double* rig_pose = nullptr;   // pinned [B][68]
        int32_t* rig_stats = nullptr; // pinned [B][8]
        std::vector<double> ts;
        hipEvent_t ev = nullptr;
        int64_t batch = -1, g0 = 0;
        int n = 0;
        bool pending = false;         // completed or in flight, not yet returned by tslam_poll_batch
    } as_res[2];
    int64_t as_batches = 0;           // batches submitted through tslam_submit_host
    int64_t as_last_pose_batch = -1;  // newest batch tslam_poll_pose returned
    // ---- tslam_api_ba.cpp ----
    // A8 keyframe window (slots shared by all pairs: keyframes are whole frames)
    BaStore ba{};
    int64_t ba_frame[TS_BA_MAXW]{};
    int64_t ba_nkf = 0;
    int64_t ba_last = -1;    // newest frame inserted
    BaTiming ba_timing{};    // k_ba_schur events while profiling is on
    bool ba_split = false;   // tslam_ba_split_solve: k_ba_reduce + k_ba_solve instead of k_ba_reduce_solve
    // tslam_ba_defer: a BA stage on its own stream is enqueued later (the next batch's first back
    // stage, or any call that reads or changes BA state), so the caller's next front stages are on
    // the GPU before this batch's ~160 BA launches are issued from the host
    bool ba_defer = false;
    // tslam_select_mode: the path of k_select (0 auto, 1 global sweeps, 2 resident wherever it fits)
    // and a cap on the candidates kept resident (0: each block shape's own capacity)
    int sel_mode = 0, sel_rcap = 0;
    // tslam_match_mode: k_match's train-side flush (0 auto, 1 direct, 2 merged per block), a cap on
    // the merge array's entries (0: TS_MTB), and the path counters tslam_match_counters switches on
    int match_mode = 0, match_cap = 0;
    int match_split = 0;   // tslam_match_layout: 1 = one side per k_match block (the tests' reference)
    // tslam_describe_mode: a cap on the positions k_describe lists at a time (0: TS_DT_LIST)
    int dt_list_cap = 0;
    uint32_t* d_match_cnt = nullptr;
    uint32_t* d_det_cnt = nullptr;   // tslam_detect_counters switches the counted k_detect build on
    struct {
        bool pending = false;
        BatchCtx c{};
        hipStream_t s = nullptr;
        double* snap = nullptr;
        double* snap_body = nullptr;
        int32_t* assoc = nullptr;
        int par = 0;
    } ba_job;
    std::map<std::pair<int, int64_t>, std::array<double, 10>> ba_imu;   // (pair, keyframe) -> IMU factor
    // (pair, keyframe) -> inertial factor record + initial velocity (tslam_ba_inertial_factor)
    std::map<std::pair<int, int64_t>, std::array<double, TS_BA_INE + 3>> ba_ine;
    std::vector<std::array<double, 12>> ba_icfg;            // per pair: gravity, bias priors and weights (BaArgs.icfg)
    std::vector<std::array<uint8_t, TS_BA_MAXW>> ba_ine_slot;   // per pair and slot: carries a factor
    std::vector<BaArgs> ba_solved;   // per pair: the arguments of its last window solve (replays)
    // A pair window's keyframe chain (eviction, gate, tiles, iters x (Schur, reduce-and-solve),
    // back substitution: ~16 launches) replayed from a captured hipGraph per chain shape: the
    // kernels read a device record (BaRec) written by the graph's first node, so a replay costs one
    // node update and one graph launch instead of ~16 launches with 2 KB of by-value arguments.
    // Each shape keeps a ring of instances (own record, event of its last replay), so an instance
    // is updated only once its previous replay has run.
    struct BaGraphInst {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        hipGraphNode_t setrec = nullptr;
        hipEvent_t done = nullptr;
        bool armed = false;
        BaRec* d_rec = nullptr;
    };
    struct BaGraphSet {
        std::array<int, 6> key{};   // evict, eviction n_order, n_order, inertial, split, iters
        std::vector<BaGraphInst> inst;
        int next = 0;
    };
    // tslam_ba_graph: off by default — measured on MI355X (tools/ba_probe.py), a
    // replay (one node update + the graph launch) costs the host 162 us per keyframe against 80 us
    // for the 16 direct launches, and the chain's GPU time 0.240 against 0.222 ms
    bool ba_graph = false;
    std::vector<BaGraphSet> ba_graphs;
    hipStream_t ba_cap_stream = nullptr;
    // BA on its own stream (overlapping the next batch): events per batch parity (batch_idx)
    hipStream_t ba_stream = nullptr;
    hipEvent_t ev_fe = nullptr, ev_ba[2] = {nullptr, nullptr};
    bool ba_pending[2] = {false, false};
    std::vector<hipEvent_t> ba_events;
    // ---- tslam_api_exchange.cpp ----
    // sharded rig (tslam_set_shard): front-end cameras [sh_cam_lo, sh_cam_hi) and back-end frames
    // [rank * n / world, (rank + 1) * n / world) of every batch
    int sh_cam_lo = 0, sh_cam_hi = 0, sh_rank = 0, sh_world = 1;
    // pair split (TSLAM_SHARD_PAIRS, one camera per rank): the back end solves this camera's pair
    // over half of the batch and the rig pose covers range rig_slot (tslam_ranges.h)
    bool sh_pairs = false;
    // library-driven sharding (tslam_comm_init / tslam_group_create, tslam_shard.cpp): the driver
    // that owns this rank's communicators, streams and exchange buffers (owned here after
    // tslam_comm_init; a group owns it otherwise)
    bool sh_comm = false;
    tslam_shard_driver* drv = nullptr;
    bool drv_owned = false;
    // ---- tslam_api_loop.cpp ----
    // relocalisation map (tslam_map_upload) and scratch
    double* d_map_xyz = nullptr;
    uint32_t* d_map_desc = nullptr;
    int64_t map_n = 0, map_cap = 0;
    int32_t* d_rl_match = nullptr;
    double* d_rl_corr = nullptr;
    int32_t* d_rl_stats = nullptr;
    double* d_rl_pose = nullptr;
    double* d_rl_ransac = nullptr;
    double* d_rl_hyp = nullptr;
    double* d_rl_rig_pose = nullptr;    // tslam_relocalize_rig: the body record
    int32_t* d_rl_rig_stats = nullptr;
    // loop closure (tslam_loop_*): keyframe database, one entry per keyframe, slot = count mod cap
    int lp_cap = 0, lp_S = 0;
    int64_t lp_count = 0;
    double* d_lp_xyz = nullptr;      // [cap][K][3] camera-frame landmarks (compacted)
    uint32_t* d_lp_desc = nullptr;   // [cap][K][8]
    int32_t* d_lp_n = nullptr;       // [cap]
    int32_t* d_lp_votes = nullptr;   // [cap]
    // asynchronous loop closure (tslam_loop_auto / tslam_loop_job_*): keyframes stored by the
    // submit path into entry (k mod cap_k) * P + p with a snapshot of their image; jobs (vote,
    // verify, pose graph) in order on the loop stream, results in pinned memory
    int lp_auto = 0;                       // keyframe interval (0: off)
    int64_t* d_lp_pos = nullptr;           // database positions taken so far (device counter)
    uint32_t* d_lp_snap_kps = nullptr;     // [cap][K][2]
    int32_t* d_lp_snap_kcount = nullptr;   // [cap][TS_MAX_LEVELS]
    uint32_t* d_lp_snap_desc = nullptr;    // [cap][K][8]
    hipStream_t lp_stream = nullptr;
    hipEvent_t lp_ev_store = nullptr;      // the newest batch's keyframe stores (back stream)
    bool lp_store_armed = false;
    struct LoopJob {
        int kind = 0;                      // 0 free, 1 vote, 2 verify, 3 pose graph
        int64_t id = 0;
        hipEvent_t ev = nullptr;
        int n_out = 0, n_edges = 0;        // votes / nodes; pose-graph edges
        void* out = nullptr;               // pinned results
        size_t out_cap = 0;
        void* in = nullptr;                // pinned pose-graph inputs
        size_t in_cap = 0;
        int posted = 0;                    // (worker mutex) 0 queued, 1 on the loop stream, -1 failed
        std::string err;
    } lp_jobs[64];
    int64_t lp_job_next = 1;
    // the loop worker: a host thread that issues the jobs' copies and launches on the loop stream,
    // so a job call returns once its inputs are staged (the caller's frame loop does not pay the
    // ~10-200 launches of a verification or a span solve)
    struct LoopWorker {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::deque<std::function<void()>> q;
        int pending = 0;
        bool stop = false;
    }* lp_worker = nullptr;
    // pose graph (tslam_pose_graph) scratch, grown on demand
    int pg_nodes = 0, pg_edges = 0, pg_np = 0;
    double *d_pg_T = nullptr, *d_pg_Z = nullptr, *d_pg_info = nullptr, *d_pg_terms = nullptr;
    double *d_pg_H = nullptr, *d_pg_g = nullptr, *d_pg_delta = nullptr, *d_pg_Ld = nullptr;
    int32_t *d_pg_edges = nullptr, *d_pg_adj_off = nullptr, *d_pg_adj = nullptr, *d_pg_ftile = nullptr;
    double* d_pg_cost = nullptr;   // the solve's cost (k_pg_cost_sum), one double
    // ---- tslam_api_tsdf.cpp ----
    // RGB-D dense mapping (tslam_tsdf_*): dense TSDF volume + per-launch pose scratch
    bool tsdf_on = false;
    bool tsdf_color = false;          // colour layer (tslam_tsdf_color)
    TsdfArgs tsdf{};
    double tsdf_trunc_vox = 0.0;      // as tslam_tsdf_init was given it (tsdf.trunc = trunc_vox * s)
    double* d_tsdf_poses = nullptr;   // [TSDF_MAX_FRAMES][TSDF_POSE]
    double* d_tsdf_wTc = nullptr;     // [TSDF_MAX_FRAMES][16] host poses staged
    // the rolling window (tslam_tsdf_follow / _shift): allocated on first use; once the record
    // exists the volume's corner is the effective origin everywhere (TsdfArgs::win of every launch)
    bool tsdf_follow_on = false;
    TsdfFollow tsdf_follow{};
    TsdfWindow* d_tsdf_win = nullptr; // {shift, delta}, written on the device
    float* d_tsdf_scratch = nullptr;  // the move's copy of every layer (each layer's base a multiple of 4 floats)
    size_t tsdf_scratch_cap = 0;
    // ---- tslam_api_store.cpp ----
    // the brick store behind the window (tslam_tsdf_store_*): table, pool and counters on the device
    bool store_on = false;
    TsdfStore store{};
    int64_t store_cells = 0;
    size_t store_pool_bytes = 0;      // as allocated (for the layers tslam_tsdf_store_init found)
    // ---- tslam_api_store_mesh.cpp ----
    // the mesh of the whole map (tslam_mesh_extract_whole): the brick list, its pinned host copy for
    // the sort, the per-brick triangle totals and first triangles; all sized on first use and grown
    // on demand.  The triangles go to d_mesh_tris / d_mesh_cols, which the two extracts share.
    uint64_t* d_wmesh_list = nullptr;   // [wmesh_list_cap] keys
    int64_t wmesh_list_cap = 0;
    uint32_t* d_wmesh_count = nullptr;  // the list's length
    uint64_t* wmesh_host = nullptr;     // pinned
    size_t wmesh_host_cap = 0;
    uint32_t* d_wmesh_bsum = nullptr;   // [wmesh_bricks_cap]
    uint64_t* d_wmesh_boff = nullptr;   // [wmesh_bricks_cap + 1]; the last one = the mesh's total
    int64_t wmesh_bricks_cap = 0;
    // ---- tslam_api_render.cpp ----
    // the volume seen from a pose (tslam_tsdf_render_*): parameters, the camera's ray-length table,
    // the call's pose table and staged host poses, and the images [rnd_views][H][W] of every
    // output the init asked for (the others stay null)
    bool rnd_on = false;
    tslam_tsdf_render_params rnd_prm{};
    int rnd_views = 0;
    double* d_rnd_L = nullptr;        // [H][W]
    double* d_rnd_poses = nullptr;    // [TSDF_MAX_FRAMES][TSDF_POSE]
    double* d_rnd_wTc = nullptr;      // [TSDF_MAX_FRAMES][16]
    float* d_rnd_depth_m = nullptr;
    uint16_t* d_rnd_depth_mm = nullptr;
    float* d_rnd_normal = nullptr;
    uint8_t* d_rnd_color = nullptr;
    // dense frame-to-model alignment (tslam_tsdf_align_*): parameters, the pair's ray-length table,
    // the model images [aln_frames][H][W] of its own render, the per-frame state and block partials,
    // and the outputs; aln_n: the frames of the last tslam_tsdf_align call
    bool aln_on = false;
    tslam_tsdf_align_params aln_prm{};
    int aln_pair = 0, aln_rect = 0, aln_frames = 0, aln_n = 0, aln_pblocks = 0;
    double* d_aln_L = nullptr;        // [H][W]
    double* d_aln_poses = nullptr;    // [TSDF_MAX_FRAMES][TSDF_POSE]: the render's table at T0
    double* d_aln_wTc_in = nullptr;   // [TSDF_MAX_FRAMES][16] host poses staged
    float* d_aln_depth_m = nullptr;
    float* d_aln_normal = nullptr;
    double* d_aln_state = nullptr;    // [aln_frames][ALIGN_STATE]
    double* d_aln_part = nullptr;     // [aln_frames][aln_pblocks][ALIGN_PART]
    double* d_aln_wTc = nullptr;      // [aln_frames][16]
    int32_t* d_aln_stats = nullptr;   // [aln_frames][ALIGN_STATS]
    double* d_aln_resid = nullptr;    // [aln_frames][2]
    double* d_aln_neq = nullptr;      // [aln_frames][28]
    // ---- tslam_api_dynamic.cpp ----
    // the free-space depth mask (tslam_tsdf_dynamic_*): parameters, the camera of its frames, the
    // call's pose table and staged host poses, the candidate words and the outputs [dyn_frames][H][W]
    bool dyn_on = false;
    tslam_tsdf_dynamic_params dyn_prm{};
    int dyn_pair = 0, dyn_rect = 0, dyn_frames = 0;
    double* d_dyn_poses = nullptr;    // [TSDF_MAX_FRAMES][TSDF_POSE]
    double* d_dyn_wTc = nullptr;      // [TSDF_MAX_FRAMES][16] host poses staged
    uint64_t* d_dyn_bits = nullptr;   // [dyn_frames][H][(W + 63) / 64][2]: candidates, valid pixels
    uint16_t* d_dyn_depth = nullptr;
    uint8_t* d_dyn_mask = nullptr;
    int32_t* d_dyn_stats = nullptr;   // [dyn_frames][DYNAMIC_STATS]
    // ---- tslam_api_freespace.cpp ----
    // the free-space layer (tslam_tsdf_freespace_*): one word per voxel, its parameters (band =
    // occupied_band_vox * s, formed once at the init) and the update's pose table
    bool fs_on = false;
    double fs_band = 0.0;
    int fs_settle = 0;
    uint32_t* d_fs_words = nullptr;   // [nz][ny][nx]: run (bits 0..15), settled (bit 16)
    double* d_fs_poses = nullptr;     // [TSDF_MAX_FRAMES][TSDF_POSE]: cam_T_world of the call's frames
    // ---- tslam_api_stereo.cpp ----
    // dense stereo depth (tslam_stereo_depth_*): parameters, output slots and winner-map scratch
    bool sd_on = false;
    tslam_stereo_depth_params sd_prm{};
    int sd_frames = 0;                // slots
    int sd_w = 0, sd_h = 0;           // image size of the last call (layout of the slots)
    uint16_t* d_sd_depth = nullptr;   // [sd_frames][H][W]
    uint16_t* d_sd_disp = nullptr;
    uint8_t* d_sd_win = nullptr;      // [2][sd_frames][H][W] left / right winners
    // semi-global aggregation (tslam_stereo_depth_sgm): off unless asked for
    bool sd_sgm_on = false;
    tslam_stereo_depth_sgm_params sd_sgm_prm{};
    int sd_sgm_chunk = 0;             // frames per pass (resolved from chunk_frames)
    uint16_t* d_sd_vol = nullptr;     // A [sd_sgm_chunk][H][W][pitch]
    uint16_t* d_sd_sum = nullptr;     // S, the same layout
    // median and speckle filters (tslam_stereo_depth_filter): off unless asked for.  The median
    // writes into d_sd_win, whose winner maps are dead by then and which is one u16 plane per slot
    bool sd_flt_on = false;
    tslam_stereo_depth_filter_params sd_flt_prm{};
    uint32_t* d_sd_label = nullptr;   // [sd_frames][H][W], with a speckle size only
    uint32_t* d_sd_count = nullptr;
    // ---- tslam_api_register.cpp ----
    // depth registration (tslam_depth_register_*), one state per pair: parameters (prm.map: the
    // device copy of the table, or null), the z-buffer planes of one call and the output slots
    struct DepthReg {
        bool on = false;
        tslam_depth_register_params prm{};
        int frames = 0;                   // slots
        int32_t* d_map = nullptr;         // [Hc][Wc][2]
        uint32_t* d_z = nullptr;          // [frames][Hc][Wc]
        uint16_t* d_reg = nullptr;        // [frames][Hc][Wc]
        uint8_t* d_bgr = nullptr;         // [frames][H][W][3]
        uint8_t* d_mask = nullptr;        // [frames][H][W]
    } dr[8];
    // tslam_depth_register_profile: events around the three passes of the newest call
    bool dr_prof = false, dr_timed = false;
    hipEvent_t dr_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // ---- tslam_api_dense.cpp ----
    // dense-map outputs (tslam_mesh_* / tslam_esdf_*): scratch sized on first use
    uint8_t* d_mesh_cfg = nullptr;    // [cubes] configuration bytes
    uint32_t* d_mesh_bsum = nullptr;  // [blocks] triangle totals
    uint64_t* d_mesh_boff = nullptr;  // [blocks] first triangle; [blocks] = mesh total
    size_t mesh_cubes_cap = 0;
    float* d_mesh_tris = nullptr;     // [tri cap][9]
    float* d_mesh_cols = nullptr;     // [tri cap][9] vertex colours (colour layer)
    int64_t mesh_tris_cap = 0, mesh_n = 0;
    int32_t* d_edt[2] = {nullptr, nullptr};
    size_t edt_cap = 0;
    float* d_esdf = nullptr;          // [nz][ny][nx]
    size_t esdf_cap = 0;
    bool esdf_valid = false;
    float* d_dist_tab = nullptr;      // [R^2 + 1]
    int dist_tab_R = -1;
    double dist_tab_s = 0.0;
    uint8_t* d_slice_obs = nullptr;
    float* d_slice = nullptr;
    size_t slice_cap = 0;
    // ---- tslam_api_archive.cpp ----
    // the depth archive (tslam_tsdf_archive_*; thor_slam_amd/dense_loop.py): the ring and its last
    // selection on the device, the camera and interval of its frames, the table of one integrate
    // chunk as world_T_cam with the slots its entries took, and a move's requests (pinned staging,
    // reused once the event of the copy out of it has passed, and their device copies)
    bool arc_on = false;
    int arc_pair = 0, arc_rect = 0, arc_interval = 1;
    TsdfArchive arc{};
    double* d_arc_wTc = nullptr;        // [TSDF_MAX_FRAMES][16]
    int32_t* d_arc_slot_of = nullptr;   // [TSDF_MAX_FRAMES]
    void* arc_pin = nullptr;            // [n] frame ids, then [n][16] poses
    size_t arc_pin_cap = 0;
    hipEvent_t arc_ev = nullptr;
    bool arc_ev_armed = false;
    void* d_arc_req = nullptr;          // the same layout on the device
    size_t arc_req_cap = 0;
};

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return fail(TSLAM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

#define BA_FLUSH(h)                                    \
    do {                                               \
        if ((h) && (h)->ba_job.pending) {              \
            const int rc_flush__ = ba_flush(h);        \
            if (rc_flush__ != TSLAM_OK) return rc_flush__; \
        }                                              \
    } while (0)

// -- tslam_api.cpp ---------------------------------------------------------------------------------
TSLAM_INTERNAL int fail(int code, const std::string& msg);   // sets tslam_last_error(), returns `code`
TSLAM_INTERNAL int dev_alloc(tslam_handle* h, void** p, size_t bytes);
TSLAM_INTERNAL int dev_grow(tslam_handle* h, void** p, size_t need, size_t* cap = nullptr);
TSLAM_INTERNAL void dev_release(tslam_handle* h, void** p);   // hipFree, out of h->allocs, *p = nullptr
TSLAM_INTERNAL int pinned_reserve(tslam_handle* h, void** p, size_t* cap, size_t bytes);
TSLAM_INTERNAL BatchCtx make_ctx(tslam_handle* h);

// What differs between the paths in the back stages of a batch: the contexts they run on (null:
// nothing to run, as on a rank whose frame range is empty) and what TSLAM_STAGE_POSE includes.
struct BackView {
    const BatchCtx* b;     // match, refinement and pose
    const BatchCtx* pre;   // stereo pre-pass of the frame before a sharded range
    const BatchCtx* rig;   // rig pose
    bool pose_rig;         // STAGE_POSE runs the rig pose
    bool pose_chain;       // ... and the chains and the loop database's keyframe store
};
// The stage table.  Both return 1 when `stage` was theirs, 0 when it is not one of their codes,
// < 0 on an error; the caller checks hipGetLastError().
TSLAM_INTERNAL int run_front_stage(tslam_handle* h, const BatchCtx& c, int stage, hipStream_t s);
TSLAM_INTERNAL int run_back_stage(tslam_handle* h, const BatchCtx& c, const BackView& v, int stage, hipStream_t s);

// -- tslam_api_ba.cpp ------------------------------------------------------------------------------
TSLAM_INTERNAL int alloc_ba(tslam_handle* h);
TSLAM_INTERNAL int ba_flush(tslam_handle* h);
TSLAM_INTERNAL int ba_stage(tslam_handle* h, const BatchCtx& c, hipStream_t s);    // TSLAM_STAGE_BA
TSLAM_INTERNAL int ba_inline(tslam_handle* h, const BatchCtx& c, hipStream_t s);   // A8 inside TSLAM_STAGE_ALL
TSLAM_INTERNAL int ba_reset(tslam_handle* h);
TSLAM_INTERNAL void ba_destroy(tslam_handle* h);

// -- tslam_api_exchange.cpp ------------------------------------------------------------------------
TSLAM_INTERNAL int run_sharded_stage(tslam_handle* h, const BatchCtx& c, int stage, hipStream_t s);

// -- tslam_api_loop.cpp ----------------------------------------------------------------------------
TSLAM_INTERNAL void loop_worker_drain(tslam_handle* h);
TSLAM_INTERNAL void loop_worker_stop(tslam_handle* h);
TSLAM_INTERNAL void loop_auto_store(tslam_handle* h, const BatchCtx& c, hipStream_t s);
TSLAM_INTERNAL int loop_reset(tslam_handle* h);
TSLAM_INTERNAL void loop_destroy(tslam_handle* h);

// the stream of a call: the caller's, or the one the handle worked on last
static inline hipStream_t call_stream(const tslam_handle* h, void* stream) { return stream ? (hipStream_t)stream : h->last_stream; }

// -- tslam_api_tsdf.cpp ----------------------------------------------------------------------------
TSLAM_INTERNAL int dense_reset(tslam_handle* h);
TSLAM_INTERNAL size_t tsdf_voxels(const tslam_handle* h);
TSLAM_INTERNAL int dense_quiesce(tslam_handle* h);   // every stream's work on the map is done
TSLAM_INTERNAL int no_volume();                      // TSLAM_ESTATE, "no TSDF volume (tslam_tsdf_init)"
// The checks that open an entry point that works on the volume outside a batch, in the order all of
// them report: a deferred BA flushed, no volume, `ready` false (`need`: the render or the align state
// the call works with), "`name` inside a batch".  `h` is not null.
TSLAM_INTERNAL int dense_open(tslam_handle* h, const char* name, bool ready = true, const char* need = nullptr);
// device poses (host_poses null): frames first_frame .. first_frame + n - 1 must belong to the last
// batch, *f0 is the first one's index in it; with host poses nothing is asked and *f0 = 0
TSLAM_INTERNAL int batch_frames(const tslam_handle* h, const double* host_poses, int64_t first_frame, int n, int* f0);
// host poses [n][16] copied onto the stream into `staging`, *staged = staging; device poses
// (host null): nothing is copied and *staged = null
TSLAM_INTERNAL int stage_poses(const double* host, int n, double* staging, hipStream_t s, const double** staged);
// the window's record and the move's scratch for every layer the volume has now: on first use, after
// a larger tslam_tsdf_init, and when a layer is added while the record exists
TSLAM_INTERNAL int window_alloc(tslam_handle* h);
// the window as the device has it once `s` has drained
TSLAM_INTERNAL int window_read(tslam_handle* h, hipStream_t s, int32_t shift[3], double origin[3]);
// a pair's rectified left camera; map: the raw camera's undistortion table, null for depth that is
// rectified already (`rect`) and for a pair without a table
struct PairCamera {
    double fx, fy, cx, cy;
    const int32_t* map;
};
TSLAM_INTERNAL PairCamera pair_camera(tslam_handle* h, int pair, bool rect);
// what every integrate call hands k_tsdf_integrate but its frames: the volume, the window's record,
// the camera (its table in `map`; the rig's cameras go into their own records), and the colour layer
// only with colour input; and what the call's first chunk does while the window follows
TSLAM_INTERNAL TsdfArgs integrate_args(const tslam_handle* h, const PairCamera& k, bool color_given);
TSLAM_INTERNAL TsdfFollowCall follow_call(const tslam_handle* h);
// the fields of a that describe the volume: tsdf, weight, dims, origin, s, win (the colour layer is the caller's)
TSLAM_INTERNAL void volume_view(const tslam_handle* h, TsdfRenderArgs& a);

// the layers of the volume as the move and the brick store see them (the scratch must exist)
TSLAM_INTERNAL TsdfLayers window_layers(const tslam_handle* h);

// -- tslam_api_store.cpp ---------------------------------------------------------------------------
TSLAM_INTERNAL int store_clear(tslam_handle* h);   // tslam_tsdf_init, tslam_reset: the store is empty, sized for the layers of now
static inline const TsdfStore* store_of(const tslam_handle* h) { return h->store_on ? &h->store : nullptr; }

// -- tslam_api_archive.cpp ------------------------------------------------------------------------
TSLAM_INTERNAL int archive_reset(tslam_handle* h);     // tslam_reset: the ring is empty, the state stays
TSLAM_INTERNAL void archive_off(tslam_handle* h);      // the archive belongs to the volume it was filled with
TSLAM_INTERNAL void archive_destroy(tslam_handle* h);  // its event (the buffers go with the handle's)

// -- tslam_api_register.cpp ------------------------------------------------------------------------
TSLAM_INTERNAL void register_destroy(tslam_handle* h);   // its events (the buffers go with the handle's)

// -- tslam_api_render.cpp --------------------------------------------------------------------------
TSLAM_INTERNAL void align_off(tslam_handle* h);   // the align state belongs to the volume it was made for

// -- tslam_api_dynamic.cpp -------------------------------------------------------------------------
TSLAM_INTERNAL void dynamic_off(tslam_handle* h);    // the mask state belongs to the volume it was made for
TSLAM_INTERNAL int dynamic_reset(tslam_handle* h);   // tslam_reset: the state stays, its images do not

// -- tslam_api_freespace.cpp -----------------------------------------------------------------------
TSLAM_INTERNAL void freespace_off(tslam_handle* h);    // the layer belongs to the volume it was made for
TSLAM_INTERNAL int freespace_reset(tslam_handle* h);   // tslam_reset: the layer is zeroed, as the volume is
// the layer's update with the frames of a tslam_tsdf_dynamic call, on its stream after its outputs
// (nothing unless the layer exists); host_wTc_dev: that call's staged host poses, or null
TSLAM_INTERNAL void freespace_update(tslam_handle* h, const void* depth, int64_t stride_bytes, int n_frames, int f0,
                                     const double* host_wTc_dev, hipStream_t s);
