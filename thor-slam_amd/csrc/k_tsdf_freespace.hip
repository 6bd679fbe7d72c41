// k_tsdf_freespace.hip — masked objects that come to rest enter the map: the free-space layer's
// update (tslam_tsdf_freespace_*; run after the mask outputs of every tslam_tsdf_dynamic call while
// the layer exists).  Spec and CPU restatement: thor_slam_amd/dense_freespace.py; every f64
// operation below is one of k_tsdf_integrate's, in its order (-ffp-contract=off keeps them unfused).
//
// One uint32 word per voxel [nz][ny][nx]: bits 0..15 the run of consecutive occupied observations
// (saturating), bit 16 `settled`.
//
//   k_tsdf_poses        (k_tsdf.hip, through launch_tsdf_poses) per frame: cam_T_world (3x4) + the use flag;
//   k_freespace_update  k_tsdf_integrate's shape: one 256-thread block per 16x4x4 brick, the call's
//                       pose table in LDS, the frames whose view can reach the brick as ballot words
//                       in LDS (tsdf_brick_visible: band <= trunc keeps the cull conservative), and
//                       each thread walks those frames in order for its voxel: the centre projected
//                       (f64), the nearest depth pixel through the undistortion table, sdf = d - p_z;
//                       within the band the run grows and settles, in front of it the word clears,
//                       behind it nothing is seen.  The word is loaded on the first observation and
//                       stored once, only if it changed; a brick nobody sees loads and stores
//                       nothing.  No atomics and no floating-point sums: a voxel belongs to one thread.
#include "tslam_common.h"
#include "tslam_tsdf_brick.h"

__global__ __launch_bounds__(256) void k_freespace_update(TsdfArgs a, uint32_t* __restrict__ words, double band, uint32_t settle,
                                                          int nbx, int nby) {
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
            const double BX = ox + a.s * (i0 + 0.5 * ex), BY = oy + a.s * (j0 + 0.5 * ey), BZ = oz + a.s * (k0 + 0.5 * ez);
            const double R = 0.5 * a.s * sqrt((double)(ex * ex + ey * ey + ez * ez)) * 1.01 + 1e-6;
            vis = tsdf_brick_visible(a, a.fx, a.fy, a.cx, a.cy, s_p + t * TSDF_POSE, BX, BY, BZ, R);
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
    uint32_t word = 0, word0 = 0;
    for (int wd = 0; wd < (a.n + 63) / 64; ++wd) {
        uint64_t m = s_mask[wd];   // wave-uniform: frames in order
        while (m) {
            const int f = wd * 64 + __builtin_ctzll(m);
            m &= m - 1;
            const double* q = s_p + f * TSDF_POSE;   // LDS broadcast
            const double pz = ((q[6] * X + q[7] * Y) + q[8] * Z) + q[11];
            if (!(pz > 0.0)) continue;
            const double px = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[9];
            const double py = ((q[3] * X + q[4] * Y) + q[5] * Z) + q[10];
            const double u = a.fx * px / pz + a.cx, vv = a.fy * py / pz + a.cy;
            const double fu = floor(u + 0.5), fv = floor(vv + 0.5);
            if (!(fu >= 0.0 && fu < a.W && fv >= 0.0 && fv < a.H)) continue;
            int ix = (int)fu, iy = (int)fv;
            if (a.map) {
                const int32_t* mp = a.map + ((size_t)iy * a.W + ix) * 2;
                ix = min(max((mp[0] + 16) >> 5, 0), a.W - 1);
                iy = min(max((mp[1] + 16) >> 5, 0), a.H - 1);
            }
            const uint16_t mm = reinterpret_cast<const uint16_t*>(a.depth + (size_t)f * a.stride)[(size_t)iy * a.W + ix];
            const double d = (double)mm * 0.001;
            if (!(d > 0.0 && d <= a.max_dist)) continue;
            const double sdf = d - pz;
            if (sdf < -band) continue;   // behind the surface: not observed
            if (!loaded) {
                word = word0 = words[v];
                loaded = true;
            }
            if (sdf <= band) {           // occupied: the run grows, and settles
                const uint32_t run = min((word & FREESPACE_RUN_MASK) + 1u, FREESPACE_RUN_MASK);
                word = (word & FREESPACE_SETTLED) | run;
                if (run >= settle) word |= FREESPACE_SETTLED;
            } else {                     // free: the run ends and a release is withdrawn
                word = 0;
            }
        }
    }
    if (loaded && word != word0) words[v] = word;
}

void launch_tsdf_freespace(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfArgs& a, uint32_t* words,
                           double band, int settle_frames, double* poses, hipStream_t s) {
    if (a.n <= 0) return;
    launch_tsdf_poses(c, pair, f0, host_wTc_dev, a.n, poses, s);   // the integrator's own table
    TsdfArgs b = a;
    b.poses = poses;
    const int nbx = (a.nx + TSDF_BX - 1) / TSDF_BX, nby = (a.ny + TSDF_BY - 1) / TSDF_BY, nbz = (a.nz + TSDF_BZ - 1) / TSDF_BZ;
    hipLaunchKernelGGL(k_freespace_update, dim3((unsigned)((int64_t)nbx * nby * nbz)), dim3(256), 0, s, b, words, band,
                       (uint32_t)settle_frames, nbx, nby);
}
