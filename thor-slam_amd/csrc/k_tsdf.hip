// k_tsdf.hip — RGB-D dense mapping: projective TSDF integration (nvblox
// parameters of launch/thor_nvblox.launch.py:26-36).  CPU restatement and spec:
// oracle/numpy_tsdf.py.
//
// The volume is a dense voxel grid resident in HBM (tsdf f32 + weight f32, [nz][ny][nx]) in the
// tracking world frame.  One launch integrates a whole batch of depth frames: thread per voxel of a 16x4x4 brick,
// the batch's camera poses in LDS, and the voxel's (tsdf, weight) loaded on its first update and
// stored once after the last frame — the per-voxel update order is the frame order, so a batch
// equals one call per frame, while the voxel read-modify-write traffic is paid once per batch.
//
//   k_tsdf_poses      per frame: cam_T_world (3x4) + a use flag, from the host's world_T_cam or
//                     from the batch's device-resident chained poses (tracked frames only);
//   k_tsdf_integrate  per 16x4x4 brick: the frames whose view can reach the brick (bounding
//                     sphere vs the frustum, one frame per thread, ballot), then per voxel for
//                     each of those frames project the centre (f64), nearest depth pixel through
//                     the undistortion table, truncated signed distance, weighted average;
//                     with the colour layer, the same pixel's colour averaged into the voxels
//                     inside the truncation band (nvblox's colour integration), where the
//                     pixel's visibility mask, if the call has one, is non-zero (colour registered
//                     to the depth, k_depth_register.hip).
//
// A rig (tslam_tsdf_integrate_rig) integrates several cameras in the same launch:
//   k_tsdf_rig_poses         per view v = f * n_cams + ci: world_T_cam = (E_0^-1 T_abs(f)) E_pair from
//                            the rig's body pose (device record or staged host poses), inverted;
//   k_tsdf_integrate<true>   the same kernel walking views instead of frames, the view's camera
//                            (intrinsics, table, depth / colour base and stride) from a per-camera
//                            record in the kernel argument, read with scalar loads.
//
// The rolling window (thor_slam_amd/dense_follow.py; opt-in, tslam_tsdf_follow / tslam_tsdf_shift):
//   k_tsdf_follow     one wave: the first used entry of the call's first pose table, the camera
//                     centre's voxel against the anchor, and from that the call's move (delta) and
//                     the new cumulative shift, into the handle's TsdfWindow record;
//   k_tsdf_shift      the same two fields from a caller's delta;
//   k_tsdf_move       every layer of the volume moved by delta into the scratch, and (a second
//                     launch) copied back; both return at once when delta is zero; with the brick
//                     store on, k_tsdf_store.hip's two kernels run before and after them;
//   k_tsdf_integrate  with TsdfArgs::win set, the volume's corner is o + s * (double)shift.
#include <algorithm>
#include <type_traits>

#include "tslam_common.h"
#include "tslam_mul4.h"
#include "tslam_tsdf_brick.h"

// host poses: world_T_cam [n][16] -> cam_T_world; device poses: T_abs of batch frames (f0 + i)
__global__ void k_tsdf_poses(BatchCtx c, int pair, int f0, const double* host_wTc, int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double use = 1.0;   // 0: the frame is skipped
    const double* T = call_pose(c, pair, f0, host_wTc, i, &use);
    double* q = out + (size_t)i * TSDF_POSE;
    store_cam_T_world(T, q);
    q[12] = use;
}

// rig: view v = f * n_cams + ci on the body pose T = world_T_base(f) (base at frame 0), in the
// volume's frame (pair 0's rectified left camera at frame 0): world_T_cam = (E_0^-1 T) E_pair, the
// products in mul4_fixed's order, then k_tsdf_poses' inverse.  A frame's views are all used or all
// skipped: the rig's status (k_rig_pose: 0 tracked, 2 at the global first frame), or a NaN host pose.
__global__ void k_tsdf_rig_poses(BatchCtx c, uint64_t pairs, int n_cams, int f0, const double* host_wTb, int n, double* out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int f = v / n_cams, pair = (int)((pairs >> (8 * (v % n_cams))) & 0xff);
    const double* Tb;
    double use = 1.0;
    if (host_wTb) {
        Tb = host_wTb + 16 * (size_t)f;
        use = __builtin_isfinite(Tb[0]) ? 1.0 : 0.0;
    } else {
        Tb = c.rig_pose + (size_t)(f0 + f) * TS_POSE_DOUBLES + 16;
        use = pose_used(c, c.rig_stats[(size_t)(f0 + f) * TS_STATS_INTS], f0, f);
    }
    double A[16], T[16];
    mul4_fixed(c.rig_Einv, Tb, A);
    mul4_fixed(A, c.rig_E + 16 * pair, T);
    double* q = out + (size_t)v * TSDF_POSE;
    store_cam_T_world(T, q);
    q[12] = use;
}

// RIG: a.n views (frame-major, camera-minor) instead of a.n frames of one camera.  The view index
// in the update loop is wave-uniform (it comes from the block's mask words), so the view's camera
// record is read from the kernel argument with scalar loads, once per (brick, view).
template <bool RIG>
__global__ __launch_bounds__(256) void k_tsdf_integrate(std::conditional_t<RIG, TsdfRigArgs, TsdfArgs> a, int nbx, int nby) {
    __shared__ double s_p[TSDF_MAX_FRAMES * TSDF_POSE];
    __shared__ uint64_t s_mask[TSDF_MAX_FRAMES / 64];
    for (int i = threadIdx.x; i < a.n * TSDF_POSE; i += blockDim.x) s_p[i] = a.poses[i];
    double ox = a.ox, oy = a.oy, oz = a.oz;
    if (a.win) {   // the rolling window: the corner from the cumulative shift (three uniform loads)
        ox = a.ox + a.s * (double)a.win->shift[0];
        oy = a.oy + a.s * (double)a.win->shift[1];
        oz = a.oz + a.s * (double)a.win->shift[2];
    }
    const int b = blockIdx.x;
    const int i0 = (b % nbx) * TSDF_BX, j0 = ((b / nbx) % nby) * TSDF_BY, k0 = (b / (nbx * nby)) * TSDF_BZ;
    const int ex = min(TSDF_BX, a.nx - i0), ey = min(TSDF_BY, a.ny - j0), ez = min(TSDF_BZ, a.nz - k0);
    __syncthreads();
    {   // frames that may see the brick: thread t tests frame t (t < TSDF_MAX_FRAMES = blockDim)
        const int t = threadIdx.x;
        bool vis = false;
        if (t < a.n) {
            const double BX = ox + a.s * (i0 + 0.5 * ex), BY = oy + a.s * (j0 + 0.5 * ey),
                         BZ = oz + a.s * (k0 + 0.5 * ez);
            const double R = 0.5 * a.s * sqrt((double)(ex * ex + ey * ey + ez * ez)) * 1.01 + 1e-6;
            if constexpr (RIG) {
                const TsdfRigCam& cm = a.cams[t % a.n_cams];
                vis = tsdf_brick_visible(a, cm.fx, cm.fy, cm.cx, cm.cy, s_p + t * TSDF_POSE, BX, BY, BZ, R);
            } else {
                vis = tsdf_brick_visible(a, a.fx, a.fy, a.cx, a.cy, s_p + t * TSDF_POSE, BX, BY, BZ, R);
            }
        }
        const uint64_t m = __ballot(vis);
        if ((t & 63) == 0) s_mask[t >> 6] = m;
    }
    __syncthreads();
    const int ti = threadIdx.x % TSDF_BX, tj = (threadIdx.x / TSDF_BX) % TSDF_BY, tk = threadIdx.x / (TSDF_BX * TSDF_BY);
    if (ti >= ex || tj >= ey || tk >= ez) return;
    const int i = i0 + ti, j = j0 + tj, k = k0 + tk;
    const int64_t v = ((int64_t)k * a.ny + j) * a.nx + i;
    const double X = ox + a.s * (i + 0.5), Y = oy + a.s * (j + 0.5), Z = oz + a.s * (k + 0.5);
    bool loaded = false;
    double ts = 0.0, w = 0.0;
    double cr = 0.0, cg = 0.0, cb = 0.0, cw = 0.0;   // colour layer (loaded with the voxel)
    for (int wd = 0; wd < (a.n + 63) / 64; ++wd) {
        uint64_t m = s_mask[wd];   // wave-uniform: frames in order
        while (m) {
            int f = wd * 64 + __builtin_ctzll(m);
            m &= m - 1;
            double fx, fy, cx, cy;
            const int32_t* map;
            const uint8_t *depth, *color, *mask;
            if constexpr (RIG) {   // f is a view: its frame's image of its camera
                f = __builtin_amdgcn_readfirstlane(f);
                const TsdfRigCam& cm = a.cams[f % a.n_cams];
                const size_t fo = (size_t)(f / a.n_cams) * cm.stride;
                fx = cm.fx, fy = cm.fy, cx = cm.cx, cy = cm.cy;
                map = cm.map;
                depth = cm.depth + fo;
                color = cm.color + (size_t)(f / a.n_cams) * cm.color_stride;
                mask = cm.mask ? cm.mask + (size_t)(f / a.n_cams) * cm.mask_stride : nullptr;
            } else {
                fx = a.fx, fy = a.fy, cx = a.cx, cy = a.cy;
                map = a.map;
                depth = a.depth + (size_t)f * a.stride;
                color = a.color + (size_t)f * a.color_stride;
                mask = a.mask ? a.mask + (size_t)f * a.mask_stride : nullptr;
            }
            const double* q = s_p + f * TSDF_POSE;   // LDS broadcast
            const double pz = ((q[6] * X + q[7] * Y) + q[8] * Z) + q[11];
            if (!(pz > 0.0)) continue;
            const double px = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[9];
            const double py = ((q[3] * X + q[4] * Y) + q[5] * Z) + q[10];
            const double u = fx * px / pz + cx, vv = fy * py / pz + cy;
            const double fu = floor(u + 0.5), fv = floor(vv + 0.5);
            if (!(fu >= 0.0 && fu < a.W && fv >= 0.0 && fv < a.H)) continue;
            int ix = (int)fu, iy = (int)fv;
            if (map) {
                const int32_t* mp = map + ((size_t)iy * a.W + ix) * 2;
                ix = min(max((mp[0] + 16) >> 5, 0), a.W - 1);
                iy = min(max((mp[1] + 16) >> 5, 0), a.H - 1);
            }
            const uint16_t mm = reinterpret_cast<const uint16_t*>(depth)[(size_t)iy * a.W + ix];
            const double d = (double)mm * 0.001;
            if (!(d > 0.0 && d <= a.max_dist)) continue;
            const double sdf = d - pz;
            if (sdf < -a.trunc) continue;
            const double obs = fmin(sdf, a.trunc);
            if (!loaded) {
                ts = (double)a.tsdf[v];
                w = (double)a.weight[v];
                if (a.col) {
                    cr = (double)a.col[3 * v];
                    cg = (double)a.col[3 * v + 1];
                    cb = (double)a.col[3 * v + 2];
                    cw = (double)a.col_w[v];
                }
                loaded = true;
            }
            const double w1 = w + 1.0;
            ts = (double)(float)((ts * w + obs) / w1);   // stored as f32 after every frame (as the oracle)
            w = (double)(float)fmin(w1, a.max_weight);
            // colour inside the truncation band: the same pixel's BGR, where its mask (if any) is set
            if (a.col && sdf <= a.trunc && (!mask || mask[(size_t)iy * a.W + ix])) {
                const uint8_t* px = color + ((size_t)iy * a.W + ix) * 3;
                const double c1 = cw + 1.0;
                cr = (double)(float)((cr * cw + (double)px[2]) / c1);
                cg = (double)(float)((cg * cw + (double)px[1]) / c1);
                cb = (double)(float)((cb * cw + (double)px[0]) / c1);
                cw = (double)(float)fmin(c1, a.max_weight);
            }
        }
    }
    if (loaded) {
        a.tsdf[v] = (float)ts;
        a.weight[v] = (float)w;
        if (a.col) {
            a.col[3 * v] = (float)cr;
            a.col[3 * v + 1] = (float)cg;
            a.col[3 * v + 2] = (float)cb;
            a.col_w[v] = (float)cw;
        }
    }
}

// -- the rolling window --------------------------------------------------------------------------
// The decision of one integrate call (thor_slam_amd/dense_follow.py, "The decision"): one wave.
// Every lane ends up with the same first used entry (ballot + ctz), so all lanes compute the same
// move and lane 0 writes it.  No used entry, a centre that is not finite, or an index / shift that
// would reach 2^30: delta = 0 and the shift stays.
__global__ __launch_bounds__(64) void k_tsdf_follow(const double* __restrict__ poses, int n, double o0x, double o0y, double o0z,
                                                    double s, TsdfFollow f, TsdfWindow* win) {
    const int lane = threadIdx.x;
    int first = -1;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool used = i < n && poses[(size_t)i * TSDF_POSE + 12] != 0.0;
        const uint64_t m = __ballot(used);
        if (m) {
            first = base + __builtin_ctzll(m);
            break;
        }
    }
    int sh[3], d[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a) sh[a] = win->shift[a];
    if (first >= 0) {
        const double* q = poses + (size_t)first * TSDF_POSE;
        const double o0[3] = {o0x, o0y, o0z};
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double C = -((q[a] * q[9] + q[3 + a] * q[10]) + q[6 + a] * q[11]);
            const double c = floor((C - (o0[a] + s * (double)sh[a])) / s);
            if (!__builtin_isfinite(C) || !(fabs(c) < (double)TSDF_SHIFT_LIMIT)) {   // a NaN c too
                ok = false;
                continue;
            }
            const int e = (int)c - f.anchor[a];   // |anchor| < 2^30 (tslam_tsdf_follow): no overflow
            d[a] = (e > f.margin || e < -f.margin) ? f.step * (e / f.step) : 0;
            const int64_t ns = (int64_t)sh[a] + d[a];
            if (ns <= -(int64_t)TSDF_SHIFT_LIMIT || ns >= (int64_t)TSDF_SHIFT_LIMIT) ok = false;
        }
        if (!ok) d[0] = d[1] = d[2] = 0;
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            win->delta[a] = d[a];
            win->shift[a] = sh[a] + d[a];
        }
    }
}

// a caller's move: the same two fields (a shift that would reach 2^30 moves nothing)
__global__ void k_tsdf_shift(TsdfWindow* win, int dx, int dy, int dz) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int d[3] = {dx, dy, dz};
    bool ok = true;
    for (int a = 0; a < 3; ++a) {
        const int64_t ns = (int64_t)win->shift[a] + d[a];
        if (ns <= -(int64_t)TSDF_SHIFT_LIMIT || ns >= (int64_t)TSDF_SHIFT_LIMIT) ok = false;
    }
    for (int a = 0; a < 3; ++a) {
        if (!ok) d[a] = 0;
        win->delta[a] = d[a];
        win->shift[a] += d[a];
    }
}

// One row of L floats: dst[x] = src[x + sx] where the row exists (ok) and 0 <= x + sx < L, else 0.
// src is the source row's first element (dereferenced only where the element exists).  V: float4
// (the caller has checked L % 4 == 0 and sx % 4 == 0, and row bases are multiples of L) or float.
template <typename V>
__device__ __forceinline__ void tsdf_move_row(V* __restrict__ dst, const V* __restrict__ src, int64_t L, int64_t sx, bool ok,
                                              int lane) {
    for (int64_t x = lane; x < L; x += 64) {
        const int64_t xs = x + sx;
        V v{};
        if (ok && xs >= 0 && xs < L) v = src[xs];
        dst[x] = v;
    }
}

// The move, one wave per row (j, k) of every layer, rows grid-strided over a bounded grid.
// BACK = false: scratch(i, j, k) = vol(i + dx, j + dy, k + dz) inside the volume, else 0;
// BACK = true: vol = scratch.  delta comes from the record (uniform loads); zero: nothing to do.
template <bool BACK>
__global__ __launch_bounds__(256) void k_tsdf_move(TsdfLayers l, const TsdfWindow* __restrict__ win) {
    const int dx = win->delta[0], dy = win->delta[1], dz = win->delta[2];
    if ((dx | dy | dz) == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t rows = (int64_t)l.ny * l.nz;
    const int64_t w0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), wn = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t row = w0; row < rows; row += wn) {
        int64_t srow = row, sdx = 0;
        bool ok = true;
        if (!BACK) {
            const int64_t k = row / l.ny, j = row - k * l.ny;
            const int64_t js = j + dy, ks = k + dz;
            ok = js >= 0 && js < l.ny && ks >= 0 && ks < l.nz;
            srow = ks * l.ny + js;
            sdx = dx;
        }
        for (int a = 0; a < l.n; ++a) {
            const int64_t L = (int64_t)l.nx * l.comp[a], sx = sdx * l.comp[a];
            float* dst = (BACK ? l.vol[a] : l.scratch[a]) + row * L;
            const float* src = (BACK ? l.scratch[a] : l.vol[a]) + (ok ? srow : 0) * L;
            if (((L | sx) & 3) == 0)
                tsdf_move_row(reinterpret_cast<float4*>(dst), reinterpret_cast<const float4*>(src), L >> 2, sx >> 2, ok, lane);
            else
                tsdf_move_row(dst, src, L, sx, ok, lane);
        }
    }
}

void launch_tsdf_follow(const double* poses, int n, const TsdfArgs& a, const TsdfFollow& f, TsdfWindow* win, hipStream_t s) {
    hipLaunchKernelGGL(k_tsdf_follow, dim3(1), dim3(64), 0, s, poses, n, a.ox, a.oy, a.oz, a.s, f, win);
}

void launch_tsdf_shift(TsdfWindow* win, int dx, int dy, int dz, hipStream_t s) {
    hipLaunchKernelGGL(k_tsdf_shift, dim3(1), dim3(64), 0, s, win, dx, dy, dz);
}

// a bounded grid: a call that does not move costs two launches of at most TSDF_MOVE_BLOCKS blocks
#define TSDF_MOVE_BLOCKS 2048
// with the brick store (k_tsdf_store.hip): what leaves goes out before the move, what enters comes in after it
void launch_tsdf_move(const TsdfLayers& l, const TsdfWindow* win, hipStream_t s, const TsdfStore* store) {
    const int64_t rows = (int64_t)l.ny * l.nz;
    const unsigned blocks = (unsigned)std::min<int64_t>((rows + 3) / 4, TSDF_MOVE_BLOCKS);
    if (store) launch_tsdf_store_out(l, win, *store, s);
    hipLaunchKernelGGL(k_tsdf_move<false>, dim3(blocks), dim3(256), 0, s, l, win);
    hipLaunchKernelGGL(k_tsdf_move<true>, dim3(blocks), dim3(256), 0, s, l, win);
    if (store) launch_tsdf_store_in(l, win, *store, s);
}

// The table `poses` [a.n][TSDF_POSE] is on the stream: the window's decision and move when the call
// follows, then one block per brick.  Args: TsdfArgs, or TsdfRigArgs for the rig's kernel.
template <typename Args>
static void tsdf_integrate_posed(const Args& a, double* poses, hipStream_t s, const TsdfFollowCall* follow) {
    if (follow) {
        launch_tsdf_follow(poses, a.n, a, follow->f, follow->win, s);
        launch_tsdf_move(follow->l, follow->win, s, follow->store);
    }
    Args b = a;
    b.poses = poses;
    if (!b.color_stride) b.color_stride = b.stride;   // colour in the depth's records
    if constexpr (std::is_same_v<Args, TsdfRigArgs>)
        for (int ci = 0; ci < b.n_cams; ++ci)
            if (!b.cams[ci].color_stride) b.cams[ci].color_stride = b.cams[ci].stride;
    const int nbx = (a.nx + TSDF_BX - 1) / TSDF_BX, nby = (a.ny + TSDF_BY - 1) / TSDF_BY,
              nbz = (a.nz + TSDF_BZ - 1) / TSDF_BZ;
    constexpr bool RIG = std::is_same_v<Args, TsdfRigArgs>;
    hipLaunchKernelGGL(k_tsdf_integrate<RIG>, dim3((unsigned)((int64_t)nbx * nby * nbz)), dim3(256), 0, s, b, nbx, nby);
}

void launch_tsdf_poses(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, int n, double* poses, hipStream_t s) {
    hipLaunchKernelGGL(k_tsdf_poses, dim3((n + 63) / 64), dim3(64), 0, s, c, pair, f0, host_wTc_dev, n, poses);
}

void launch_tsdf(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfArgs& a, double* poses,
                 hipStream_t s, const TsdfFollowCall* follow) {
    launch_tsdf_poses(c, pair, f0, host_wTc_dev, a.n, poses, s);
    tsdf_integrate_posed(a, poses, s, follow);
}

void launch_tsdf_posed(const TsdfArgs& a, double* poses, hipStream_t s, const TsdfFollowCall* follow) {
    tsdf_integrate_posed(a, poses, s, follow);
}

void launch_tsdf_rig(const BatchCtx& c, uint64_t pairs, int f0, const double* host_wTb_dev, const TsdfRigArgs& a,
                     double* poses, hipStream_t s, const TsdfFollowCall* follow) {
    hipLaunchKernelGGL(k_tsdf_rig_poses, dim3((a.n + 63) / 64), dim3(64), 0, s, c, pairs, a.n_cams, f0, host_wTb_dev, a.n, poses);
    tsdf_integrate_posed(a, poses, s, follow);
}
