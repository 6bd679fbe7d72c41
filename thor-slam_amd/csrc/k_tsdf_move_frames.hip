// k_tsdf_move_frames.hip — the dense map kept consistent with corrected poses (loop closure,
// relocalisation): archived depth frames taken out of the TSDF volume at the pose they went in with
// and put back at their new pose (BundleFusion's re-integration).  Rule and limits:
// thor_slam_amd/dense_loop.py; its restatement for the tests: tests/ref_tsdf_move.py.
//
//   k_tsdf_archive_poses   k_tsdf_poses for an archiving call: only every `interval`-th frame is
//                          used, device poses are premultiplied by the loop correction
//                          (corr * T_abs, mul4_fixed's order), and the poses are also kept as
//                          world_T_cam;
//   k_tsdf_archive_put     one block: the used entries of that table take the next ring slots in
//                          order (ballot + prefix; the count lives on the device), their pose
//                          entries and frame ids written with them;
//   k_tsdf_archive_copy    their depth images into those slots;
//   k_tsdf_archive_select  one block: every archived frame, oldest first, against the poses asked
//                          for; the frames that moved by more than the thresholds are compacted in
//                          that order with their old and new pose entries, and counted;
//   k_tsdf_reintegrate     one block per 16x4x4 brick, as k_tsdf_integrate: the selected frames in
//                          chunks of TSDF_MOVE_CHUNK whose two pose tables sit in LDS, the frames
//                          that can see the brick at the old OR at the new pose (one test per
//                          thread, ballot), and per voxel, loaded once and stored once, for each of
//                          them in order the removal at the old pose and the insertion at the new;
//                          the count is read on the device, zero returns at once;
//   k_tsdf_archive_commit  the ring's poses of the moved frames become the new ones.
//
// The per-voxel test and arithmetic are k_tsdf_integrate's, operation for operation (f64, f32 after
// every update), so a removal meets exactly the voxels its insertion met.
#include <algorithm>

#include "tslam_common.h"
#include "tslam_mul4.h"
#include "tslam_tsdf_brick.h"

__global__ void k_tsdf_archive_poses(BatchCtx c, int pair, int f0, const double* host_wTc, int n, int64_t first_frame,
                                     int interval, int has_corr, Mat4 corr, double* out, double* wTc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double use = 1.0;
    const double* T = call_pose(c, pair, f0, host_wTc, i, &use);
    double M[16];
    if (!host_wTc && has_corr) {
        mul4_fixed(corr.m, T, M);
    } else {
        for (int k = 0; k < 16; ++k) M[k] = T[k];
    }
    if ((first_frame + i) % interval != 0) use = 0.0;
    double* q = out + (size_t)i * TSDF_POSE;
    store_cam_T_world(M, q);
    q[12] = use;
    for (int k = 0; k < 16; ++k) wTc[(size_t)i * 16 + k] = M[k];
}

// the block's exclusive prefix of a flag over its 256 threads (4 waves) and the total
__device__ __forceinline__ int block_rank(bool flag, int* s_cnt, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    __syncthreads();   // s_cnt's readers of the round before
    if (lane == 0) s_cnt[wv] = __popcll(m);
    __syncthreads();
    int before = 0, tot = 0;
    for (int k = 0; k < 4; ++k) {
        if (k < wv) before += s_cnt[k];
        tot += s_cnt[k];
    }
    *total = tot;
    return before + __popcll(m & (((uint64_t)1 << lane) - 1));
}

// Entry t of the table (frame first_frame + t) when it is used: rank r among the used ones, slot
// (count + r) % cap; the first U - cap of U > cap used entries would be overwritten at once and
// take no slot.  Every thread reads the count before thread 0 adds U to it.
__global__ __launch_bounds__(256) void k_tsdf_archive_put(TsdfArchive ar, const double* __restrict__ poses,
                                                          const double* __restrict__ wTc, int n, int64_t first_frame,
                                                          int32_t* __restrict__ slot_of) {
    __shared__ int s_cnt[4];
    const int t = threadIdx.x;
    const bool used = t < n && poses[(size_t)t * TSDF_POSE + 12] != 0.0;
    const int64_t count = ar.rec->count;
    int total;
    const int rank = block_rank(used, s_cnt, &total);
    int slot = -1;
    if (used && rank >= total - ar.cap) {
        slot = (int)((count + rank) % ar.cap);
        for (int k = 0; k < TSDF_POSE; ++k) ar.pose[(size_t)slot * TSDF_POSE + k] = poses[(size_t)t * TSDF_POSE + k];
        for (int k = 0; k < 16; ++k) ar.wTc[(size_t)slot * 16 + k] = wTc[(size_t)t * 16 + k];
        ar.frame[slot] = first_frame + t;
    }
    if (t < n) slot_of[t] = slot;
    if (t == 0) ar.rec->count = count + total;   // after block_rank's barriers: every thread has read it
}

// blockIdx.y: the table's entry; its image (`pixels` u16) into its slot, 16 bytes per thread where
// both ends are aligned
__global__ __launch_bounds__(256) void k_tsdf_archive_copy(uint8_t* __restrict__ ring, int64_t slot_stride,
                                                           const int32_t* __restrict__ slot_of, const uint8_t* __restrict__ depth,
                                                           int64_t stride, int pixels) {
    const int slot = slot_of[blockIdx.y];
    if (slot < 0) return;
    const uint8_t* src = depth + (size_t)blockIdx.y * stride;
    uint8_t* dst = ring + (size_t)slot * slot_stride;
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
    int done = 0;   // pixels copied by the wide loop
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        const int n16 = pixels / 8;
        for (int i = t0; i < n16; i += nt) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        done = n16 * 8;
    }
    for (int i = done + t0; i < pixels; i += nt)
        reinterpret_cast<uint16_t*>(dst)[i] = reinterpret_cast<const uint16_t*>(src)[i];
}

// the camera centre of a cam_T_world entry, component a: -(R^T t)[a]
__device__ __forceinline__ double entry_centre(const double* q, int a) {
    return -((q[a] * q[9] + q[3 + a] * q[10]) + q[6 + a] * q[11]);
}

// The selection (dense_loop.py, "Selection"): archive number a0 + t per thread, oldest first; the
// last request that names the frame counts.  The compaction keeps that order (block_rank).
__global__ __launch_bounds__(256) void k_tsdf_archive_select(TsdfArchive ar, const int64_t* __restrict__ req_frame,
                                                             const double* __restrict__ req_wTc, int n, double min_t2,
                                                             double rot_lim) {
    __shared__ int s_cnt[4];
    const int t = threadIdx.x;
    const int64_t count = ar.rec->count;
    const int m = count < ar.cap ? (int)count : ar.cap;
    const int64_t start = count - m;
    int base = 0;
    for (int a0 = 0; a0 < m; a0 += 256) {
        const int a = a0 + t;
        bool sel = false;
        int slot = 0, j = -1;
        double qn[TSDF_POSE];
        for (int k = 0; k < TSDF_POSE; ++k) qn[k] = 0.0;
        if (a < m) {
            slot = (int)((start + a) % ar.cap);
            const int64_t fid = ar.frame[slot];
            for (int r = 0; r < n; ++r)
                if (req_frame[r] == fid) j = r;
            if (fid < 0) j = -1;
        }
        if (j >= 0) {
            const double* T = req_wTc + (size_t)16 * j;
            if (__builtin_isfinite(T[0])) {
                store_cam_T_world(T, qn);
                qn[12] = 1.0;
                const double* qo = ar.pose + (size_t)slot * TSDF_POSE;
                const double d0 = entry_centre(qn, 0) - entry_centre(qo, 0), d1 = entry_centre(qn, 1) - entry_centre(qo, 1),
                             d2 = entry_centre(qn, 2) - entry_centre(qo, 2);
                const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                double tr = 0.0;
                for (int k = 0; k < 9; ++k) tr = tr + qo[k] * qn[k];
                sel = dd > min_t2 || tr < rot_lim;
            }
        }
        int total;
        const int k = base + block_rank(sel, s_cnt, &total);
        if (sel) {
            ar.sel_slot[k] = slot;
            for (int i = 0; i < TSDF_POSE; ++i) {
                ar.sel_old[(size_t)k * TSDF_POSE + i] = ar.pose[(size_t)slot * TSDF_POSE + i];
                ar.sel_new[(size_t)k * TSDF_POSE + i] = qn[i];
            }
            for (int i = 0; i < 16; ++i) ar.sel_wTc[(size_t)k * 16 + i] = req_wTc[(size_t)16 * j + i];
        }
        base += total;
    }
    if (t == 0) ar.rec->n_sel = base;
}

// k_tsdf_integrate's per-voxel test of one frame: the voxel centre (X, Y, Z) through the entry q
// into the frame's depth image; true with the observation when the frame updates the voxel
__device__ __forceinline__ bool tsdf_observe(const TsdfArgs& a, const double* q, double X, double Y, double Z,
                                             const uint8_t* depth, double* obs) {
    const double pz = ((q[6] * X + q[7] * Y) + q[8] * Z) + q[11];
    if (!(pz > 0.0)) return false;
    const double px = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[9];
    const double py = ((q[3] * X + q[4] * Y) + q[5] * Z) + q[10];
    const double u = a.fx * px / pz + a.cx, vv = a.fy * py / pz + a.cy;
    const double fu = floor(u + 0.5), fv = floor(vv + 0.5);
    if (!(fu >= 0.0 && fu < a.W && fv >= 0.0 && fv < a.H)) return false;
    int ix = (int)fu, iy = (int)fv;
    if (a.map) {
        const int32_t* mp = a.map + ((size_t)iy * a.W + ix) * 2;
        ix = min(max((mp[0] + 16) >> 5, 0), a.W - 1);
        iy = min(max((mp[1] + 16) >> 5, 0), a.H - 1);
    }
    const uint16_t mm = reinterpret_cast<const uint16_t*>(depth)[(size_t)iy * a.W + ix];
    const double d = (double)mm * 0.001;
    if (!(d > 0.0 && d <= a.max_dist)) return false;
    const double sdf = d - pz;
    if (sdf < -a.trunc) return false;
    *obs = fmin(sdf, a.trunc);
    return true;
}

__global__ __launch_bounds__(256) void k_tsdf_reintegrate(TsdfArgs a, TsdfArchive ar, int nbx, int nby) {
    __shared__ double s_old[TSDF_MOVE_CHUNK * TSDF_POSE];
    __shared__ double s_new[TSDF_MOVE_CHUNK * TSDF_POSE];
    __shared__ int s_slot[TSDF_MOVE_CHUNK];
    __shared__ uint64_t s_vis[2 * TSDF_MOVE_CHUNK / 64];   // [old, new][word]
    static_assert(2 * TSDF_MOVE_CHUNK == 256, "one view test per thread: old poses, then new poses");
    const int n_sel = ar.rec->n_sel;   // uniform
    if (n_sel == 0) return;
    double ox = a.ox, oy = a.oy, oz = a.oz;
    if (a.win) {
        ox = a.ox + a.s * (double)a.win->shift[0];
        oy = a.oy + a.s * (double)a.win->shift[1];
        oz = a.oz + a.s * (double)a.win->shift[2];
    }
    const int b = blockIdx.x, t = threadIdx.x;
    const int i0 = (b % nbx) * TSDF_BX, j0 = ((b / nbx) % nby) * TSDF_BY, k0 = (b / (nbx * nby)) * TSDF_BZ;
    const int ex = min(TSDF_BX, a.nx - i0), ey = min(TSDF_BY, a.ny - j0), ez = min(TSDF_BZ, a.nz - k0);
    const double BX = ox + a.s * (i0 + 0.5 * ex), BY = oy + a.s * (j0 + 0.5 * ey), BZ = oz + a.s * (k0 + 0.5 * ez);
    const double R = 0.5 * a.s * sqrt((double)(ex * ex + ey * ey + ez * ez)) * 1.01 + 1e-6;
    const int ti = t % TSDF_BX, tj = (t / TSDF_BX) % TSDF_BY, tk = t / (TSDF_BX * TSDF_BY);
    const bool active = ti < ex && tj < ey && tk < ez;   // the others only help with the tables
    const int i = i0 + ti, j = j0 + tj, k = k0 + tk;
    const int64_t v = ((int64_t)k * a.ny + j) * a.nx + i;
    const double X = ox + a.s * (i + 0.5), Y = oy + a.s * (j + 0.5), Z = oz + a.s * (k + 0.5);
    bool loaded = false;
    double ts = 0.0, w = 0.0;
    for (int c0 = 0; c0 < n_sel; c0 += TSDF_MOVE_CHUNK) {
        const int nc = min(TSDF_MOVE_CHUNK, n_sel - c0);
        __syncthreads();   // the chunk before is done with the tables
        for (int e = t; e < nc * TSDF_POSE; e += 256) {
            s_old[e] = ar.sel_old[(size_t)c0 * TSDF_POSE + e];
            s_new[e] = ar.sel_new[(size_t)c0 * TSDF_POSE + e];
        }
        if (t < nc) s_slot[t] = ar.sel_slot[c0 + t];
        __syncthreads();
        {   // thread t: frame t's old pose (t < CHUNK), frame t - CHUNK's new pose
            const int f = t & (TSDF_MOVE_CHUNK - 1);
            const double* q = (t < TSDF_MOVE_CHUNK ? s_old : s_new) + f * TSDF_POSE;
            const bool vis = f < nc && tsdf_brick_visible(a, a.fx, a.fy, a.cx, a.cy, q, BX, BY, BZ, R);
            const uint64_t m = __ballot(vis);
            if ((t & 63) == 0) s_vis[t >> 6] = m;
        }
        __syncthreads();
        if (!active) continue;
        for (int wd = 0; wd < TSDF_MOVE_CHUNK / 64; ++wd) {
            uint64_t m = s_vis[wd] | s_vis[wd + TSDF_MOVE_CHUNK / 64];   // wave-uniform: frames in order
            while (m) {
                const int f = wd * 64 + __builtin_ctzll(m);
                m &= m - 1;
                const uint8_t* depth = ar.depth + (size_t)s_slot[f] * ar.slot_stride;
                double obs;
                if (tsdf_observe(a, s_old + f * TSDF_POSE, X, Y, Z, depth, &obs)) {   // out at the old pose
                    if (!loaded) {
                        ts = (double)a.tsdf[v];
                        w = (double)a.weight[v];
                        loaded = true;
                    }
                    const double w1 = w - 1.0;
                    if (w1 > 0.0) {
                        ts = (double)(float)((ts * w - obs) / w1);
                        w = (double)(float)w1;
                    } else {   // unobserved again
                        ts = 0.0;
                        w = 0.0;
                    }
                }
                if (tsdf_observe(a, s_new + f * TSDF_POSE, X, Y, Z, depth, &obs)) {   // in at the new pose
                    if (!loaded) {
                        ts = (double)a.tsdf[v];
                        w = (double)a.weight[v];
                        loaded = true;
                    }
                    const double w1 = w + 1.0;
                    ts = (double)(float)((ts * w + obs) / w1);
                    w = (double)(float)fmin(w1, a.max_weight);
                }
            }
        }
    }
    if (loaded) {
        a.tsdf[v] = (float)ts;
        a.weight[v] = (float)w;
    }
}

// after the move: the moved frames are in the volume with their new entries
__global__ __launch_bounds__(256) void k_tsdf_archive_commit(TsdfArchive ar) {
    const int n_sel = ar.rec->n_sel;
    const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = t0; k < n_sel; k += gridDim.x * blockDim.x) {
        const int slot = ar.sel_slot[k];
        for (int i = 0; i < TSDF_POSE; ++i) ar.pose[(size_t)slot * TSDF_POSE + i] = ar.sel_new[(size_t)k * TSDF_POSE + i];
        for (int i = 0; i < 16; ++i) ar.wTc[(size_t)slot * 16 + i] = ar.sel_wTc[(size_t)k * 16 + i];
    }
    if (t0 == 0) {
        ar.rec->moved_last = n_sel;
        ar.rec->moved_total += n_sel;
    }
}

void launch_tsdf_archive_poses(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, int n, int64_t first_frame,
                               int interval, bool has_corr, const Mat4& corr, double* poses, double* wTc, hipStream_t s) {
    hipLaunchKernelGGL(k_tsdf_archive_poses, dim3((n + 63) / 64), dim3(64), 0, s, c, pair, f0, host_wTc_dev, n, first_frame,
                       interval, has_corr ? 1 : 0, corr, poses, wTc);
}

void launch_tsdf_archive_put(const TsdfArchive& ar, const double* poses, const double* wTc, int n, int64_t first_frame,
                             const uint8_t* depth, int64_t stride, int pixels, int32_t* slot_of, hipStream_t s) {
    if (n < 1) return;
    hipLaunchKernelGGL(k_tsdf_archive_put, dim3(1), dim3(256), 0, s, ar, poses, wTc, n, first_frame, slot_of);
    const unsigned bx = (unsigned)std::min((pixels / 8 + 255) / 256 + 1, 64);
    hipLaunchKernelGGL(k_tsdf_archive_copy, dim3(bx, (unsigned)n), dim3(256), 0, s, ar.depth, ar.slot_stride, slot_of, depth,
                       stride, pixels);
}

void launch_tsdf_archive_move(const TsdfArchive& ar, const TsdfArgs& a, const int64_t* req_frame, const double* req_wTc, int n,
                              double min_t2, double rot_lim, hipStream_t s) {
    hipLaunchKernelGGL(k_tsdf_archive_select, dim3(1), dim3(256), 0, s, ar, req_frame, req_wTc, n, min_t2, rot_lim);
    const int nbx = (a.nx + TSDF_BX - 1) / TSDF_BX, nby = (a.ny + TSDF_BY - 1) / TSDF_BY, nbz = (a.nz + TSDF_BZ - 1) / TSDF_BZ;
    hipLaunchKernelGGL(k_tsdf_reintegrate, dim3((unsigned)((int64_t)nbx * nby * nbz)), dim3(256), 0, s, a, ar, nbx, nby);
    hipLaunchKernelGGL(k_tsdf_archive_commit, dim3((unsigned)std::min((ar.cap + 255) / 256, 64)), dim3(256), 0, s, ar);
}
