// k_tsdf_align.hip — dense frame-to-model alignment: projective point-to-plane ICP of a depth frame
// against the ray-cast map (tslam_tsdf_align).  Spec and CPU restatement:
// thor_slam_amd/dense_align.py (rules 1-7; every f64 operation below is one of its written
// operations, in its order; -ffp-contract=off keeps them unfused).
//
// The model images (depth_m, normal at T0) come from k_tsdf_render through launch_tsdf_render, into
// the align state's own images.  Then, per iteration, on the one stream:
//
//   k_align_accumulate  grid = 16 x 16 pixel blocks x frames, a wave per 8 x 8 tile as in
//                       k_tsdf_render (the model gathers of a wave stay local).  The frame's state
//                       (T, T0, active flag) is read with uniform loads; a frame that is done exits
//                       at the top.  Each pixel's 29 terms are summed by rule 3's trees: the wave's
//                       butterfly (xor 1, 2, .. 32: neighbours first, every lane ends with the
//                       tile's sum), then (w0 + w1) + (w2 + w3) through LDS.  One partial per block,
//                       zeros included, so the partials are never cleared.  No atomics.
//   k_align_solve       one block per frame.  The padded block partials are folded by the same tree,
//                       level by level in place with coalesced loads, until 256 values are left;
//                       those go through the butterfly and LDS again, and thread 0 does the 6 x 6
//                       LDL^T, the update, the stop and accept tests, and writes the pose, the state
//                       and the stats.
//   k_align_begin       per frame: T = T0 from the render's pose table, the stats cleared.
//   k_align_poses       the aligned world_T_cam as the integrator's table: cam_T_world and the use
//                       flag (k_tsdf_poses' operations on a host pose).
//
// The host enqueues iterations x (accumulate, solve); nothing waits, and no loop on the device has a
// length that depends on data.
#include "tslam_common.h"

#define ALIGN_TILE 16

__global__ void k_align_begin(TsdfAlignArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double* q = a.poses + (size_t)i * TSDF_POSE;
    double* st = a.state + (size_t)i * ALIGN_STATE;
    double* T = a.wTc + (size_t)i * 16;
    for (int k = 0; k < 12; ++k) st[k] = st[12 + k] = q[k];
    st[24] = q[12];
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) T[4 * r + k] = q[3 * r + k];
        T[4 * r + 3] = q[9 + r];
    }
    T[12] = T[13] = T[14] = 0.0;
    T[15] = 1.0;
    int32_t* s = a.stats + (size_t)i * ALIGN_STATS;
    s[0] = q[12] != 0.0 ? 0 : 1;   // OK until a solve says otherwise; UNUSED
    s[1] = s[2] = s[3] = 0;
    a.resid[2 * (size_t)i] = a.resid[2 * (size_t)i + 1] = 0.0;
    for (int k = 0; k < 28; ++k) a.neq[28 * (size_t)i + k] = 0.0;
}

// Rule 3 over the 256 threads of a block: the wave's pairwise tree over the lane index, then the four
// waves as (w0 + w1) + (w2 + w3).  Thread q < 29 returns term q's sum; s is [4][ALIGN_PART].
__device__ __forceinline__ double align_block_sum(double (&v)[ALIGN_TERMS], double* s) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < ALIGN_TERMS; ++k) v[k] = v[k] + __shfl_xor(v[k], m);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < ALIGN_TERMS; ++k) s[wave * ALIGN_PART + k] = v[k];
    }
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x < ALIGN_TERMS) {
        const int k = threadIdx.x;
        r = (s[k] + s[ALIGN_PART + k]) + (s[2 * ALIGN_PART + k] + s[3 * ALIGN_PART + k]);
    }
    return r;
}

__global__ __launch_bounds__(256) void k_align_accumulate(TsdfAlignArgs a, int tiles_x) {
    __shared__ double s_w[4 * ALIGN_PART];
    const int f = blockIdx.y;
    const double* __restrict__ st = a.state + (size_t)f * ALIGN_STATE;   // uniform: scalar loads
    if (st[24] == 0.0) return;   // unused or done: the whole block
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = (blockIdx.x % tiles_x) * ALIGN_TILE + (wave & 1) * 8 + (lane & 7);
    const int y = (blockIdx.x / tiles_x) * ALIGN_TILE + (wave >> 1) * 8 + (lane >> 3);
    double v[ALIGN_TERMS];
#pragma unroll
    for (int k = 0; k < ALIGN_TERMS; ++k) v[k] = 0.0;
    if (x < a.W && y < a.H) {   // partial tiles: lanes outside the image carry zeros through the tree
        int ix = x, iy = y;
        if (a.map) {
            const int32_t* mp = a.map + ((size_t)y * a.W + x) * 2;
            ix = min(max((mp[0] + 16) >> 5, 0), a.W - 1);
            iy = min(max((mp[1] + 16) >> 5, 0), a.H - 1);
        }
        const uint16_t mm = reinterpret_cast<const uint16_t*>(a.depth + (size_t)f * a.stride)[(size_t)iy * a.W + ix];
        const double D = (double)mm * 0.001;
        bool ok = D > 0.0 && D <= a.max_dist;
        // 2: the frame's point in the volume's frame, and in the model view
        const double dc0 = ((double)x - a.cx) / a.fx, dc1 = ((double)y - a.cy) / a.fy;
        const double pc0 = D * dc0, pc1 = D * dc1;
        const double p0 = ((st[0] * pc0 + st[1] * pc1) + st[2] * D) + st[9];
        const double p1 = ((st[3] * pc0 + st[4] * pc1) + st[5] * D) + st[10];
        const double p2 = ((st[6] * pc0 + st[7] * pc1) + st[8] * D) + st[11];
        const double* __restrict__ s0 = st + 12;   // T0: R0 rows, C0
        const double h0 = p0 - s0[9], h1 = p1 - s0[10], h2 = p2 - s0[11];
        const double q0 = (s0[0] * h0 + s0[3] * h1) + s0[6] * h2;
        const double q1 = (s0[1] * h0 + s0[4] * h1) + s0[7] * h2;
        const double q2 = (s0[2] * h0 + s0[5] * h1) + s0[8] * h2;
        ok = ok && q2 > 0.0;
        const double fu = floor((a.fx * q0 / q2 + a.cx) + 0.5), fv = floor((a.fy * q1 / q2 + a.cy) + 0.5);
        ok = ok && fu >= 0.0 && fu < (double)a.W && fv >= 0.0 && fv < (double)a.H;   // in floating point: a NaN is outside
        if (ok) {
            const int mx = (int)fu, my = (int)fv;
            const size_t o = ((size_t)f * a.H + my) * a.W + mx;
            const double dm = (double)a.depth_m[o];
            const double n0 = (double)a.normal[3 * o], n1 = (double)a.normal[3 * o + 1], n2 = (double)a.normal[3 * o + 2];
            ok = dm > 0.0 && (n0 != 0.0 || n1 != 0.0 || n2 != 0.0);
            // 1: the model pixel's vertex
            const double mc0 = ((double)mx - a.cx) / a.fx, mc1 = ((double)my - a.cy) / a.fy;
            const double e0 = p0 - (s0[9] + dm * ((s0[0] * mc0 + s0[1] * mc1) + s0[2]));
            const double e1 = p1 - (s0[10] + dm * ((s0[3] * mc0 + s0[4] * mc1) + s0[5]));
            const double e2 = p2 - (s0[11] + dm * ((s0[6] * mc0 + s0[7] * mc1) + s0[8]));
            ok = ok && (e0 * e0 + e1 * e1) + e2 * e2 <= a.max_distance2;
            if (ok) {
                const double r = (n0 * e0 + n1 * e1) + n2 * e2;
                const double J[6] = {n0, n1, n2, p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0};
                int k = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i) {
#pragma unroll
                    for (int j = i; j < 6; ++j) v[k++] = J[i] * J[j];
                }
#pragma unroll
                for (int i = 0; i < 6; ++i) v[21 + i] = -(J[i] * r);
                v[27] = r * r;
                v[28] = 1.0;
            }
        }
    }
    const double r = align_block_sum(v, s_w);
    if (threadIdx.x < ALIGN_TERMS)
        a.partial[((size_t)f * a.pblocks + blockIdx.x) * ALIGN_PART + threadIdx.x] = r;
}

__global__ __launch_bounds__(256) void k_align_solve(TsdfAlignArgs a, int it) {
    __shared__ double s_w[4 * ALIGN_PART];
    __shared__ double s_sum[ALIGN_PART];
    const int f = blockIdx.x;
    double* st = a.state + (size_t)f * ALIGN_STATE;
    if (st[24] == 0.0) return;
    // 3: the tree over the blocks.  While more than 256 values are left, the block folds a level in
    // place: the pair (2j, 2j + 1) of the level's values lies 2^l partials apart and its sum replaces
    // its first member, which nothing else reads, so a level needs no second buffer; consecutive
    // threads take consecutive terms of a partial (its three spare slots are zeros and stay zeros).
    double* part = a.partial + (size_t)f * a.pblocks * ALIGN_PART;
    int step = 1;   // partials between neighbouring values of the level
    for (; a.pblocks / step > 256; step <<= 1) {
        // at least 256 pairs of ALIGN_PART slots: a multiple of 8 items per thread.  Eight pairs are
        // loaded before the first sum is stored, so a level costs items / 2048 round trips, not
        // items / 256 (the compiler keeps a store and the loads behind it in order)
        const int items = (a.pblocks / (2 * step)) * ALIGN_PART;
        for (int i0 = threadIdx.x; i0 < items; i0 += 256 * 8) {
            double* p[8];
            double x[8], y[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 256 * u;
                p[u] = part + ((size_t)(i / ALIGN_PART) * (2 * step)) * ALIGN_PART + (i % ALIGN_PART);
                x[u] = p[u][0];
                y[u] = p[u][(size_t)step * ALIGN_PART];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) p[u][0] = x[u] + y[u];
        }
        __syncthreads();
    }
    const double* base = part + (size_t)threadIdx.x * step * ALIGN_PART;   // thread t: value t of the 256 left
    double v[ALIGN_TERMS];
#pragma unroll
    for (int k = 0; k < ALIGN_TERMS; ++k) v[k] = base[k];
    const double tot = align_block_sum(v, s_w);
    if (threadIdx.x < ALIGN_TERMS) s_sum[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x != 0) return;

    double S[ALIGN_TERMS];
#pragma unroll
    for (int k = 0; k < ALIGN_TERMS; ++k) S[k] = s_sum[k];
    const int inl = (int)S[28];
    const double rms = S[28] > 0.0 ? sqrt(S[27] / S[28]) : 0.0;
    int32_t* stats = a.stats + (size_t)f * ALIGN_STATS;
    if (it == 1) {
        stats[2] = inl;
        a.resid[2 * (size_t)f] = rms;
    }
    stats[1] = it;
    stats[3] = inl;
    a.resid[2 * (size_t)f + 1] = rms;
#pragma unroll
    for (int k = 0; k < 28; ++k) a.neq[28 * (size_t)f + k] = S[k];

    int status = 0;
    bool done = false;
    if (inl < a.min_inliers) {
        status = 2;   // NO_MODEL
        done = true;
    } else {
        // 4: LDL^T without pivoting
        double A[6][6], L[6][6], d[6], g[6], X[6];
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    A[i][j] = S[k];
                    A[j][i] = S[k];
                    ++k;
                }
            }
        }
        double top = A[0][0];
#pragma unroll
        for (int i = 1; i < 6; ++i) top = fmax(top, A[i][i]);
        const double floor_d = a.min_pivot * top;
        bool deg = false;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double dj = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                g[k] = L[j][k] * d[k];
                dj = dj - L[j][k] * g[k];
            }
            d[j] = dj;
            deg = deg || !(dj > floor_d);
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double s = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s = s - L[i][k] * g[k];
                L[i][j] = s / dj;
            }
        }
        if (deg) {
            status = 3;   // DEGENERATE
            done = true;
        } else {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double s = S[21 + i];
#pragma unroll
                for (int k = 0; k < i; ++k) s = s - L[i][k] * g[k];
                g[i] = s;   // y
            }
#pragma unroll
            for (int i = 5; i >= 0; --i) {
                double s = g[i] / d[i];
#pragma unroll
                for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * X[k];
                X[i] = s;
            }
            // 5: the update, T <- (Rod(w), t) T
            const double w[3] = {X[3], X[4], X[5]};
            const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
            double ca = 1.0, cb = 0.5;
            if (th2 != 0.0) {
                const double th = sqrt(th2);
                ca = sin(th) / th;
                cb = (1.0 - cos(th)) / th2;
            }
            const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
            double Q[3][3], N[12];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    Q[i][j] = ((i == j ? 1.0 : 0.0) + ca * K[i][j]) + cb * (w[i] * w[j] - (i == j ? th2 : 0.0));
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) N[3 * i + j] = (Q[i][0] * st[j] + Q[i][1] * st[3 + j]) + Q[i][2] * st[6 + j];
                N[9 + i] = ((Q[i][0] * st[9] + Q[i][1] * st[10]) + Q[i][2] * st[11]) + X[i];
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) st[k] = N[k];
            // 6, 7: stop, accept
            const double tt = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
            if ((tt < a.eps_t2 && th2 < a.eps_r2) || it == a.iterations) {
                done = true;
                const double c0 = N[9] - st[21], c1 = N[10] - st[22], c2 = N[11] - st[23];
                const double cc = (c0 * c0 + c1 * c1) + c2 * c2;
                double tr = 0.0;
#pragma unroll
                for (int k = 0; k < 9; ++k) tr = tr + N[k] * st[12 + k];
                if (cc <= a.max_t2 && tr >= a.rot_lim) {
                    double* T = a.wTc + (size_t)f * 16;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) T[4 * r + k] = N[3 * r + k];
                        T[4 * r + 3] = N[9 + r];
                    }
                } else {
                    status = 4;   // REJECTED: the pose stays T0, as k_align_begin wrote it
                }
            }
        }
    }
    if (done) {
        stats[0] = status;
        st[24] = 0.0;
    }
}

// the aligned poses as k_tsdf_integrate's table (k_tsdf_poses' operations on a host pose)
__global__ void k_align_poses(const double* wTc, const int32_t* stats, int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* T = wTc + 16 * (size_t)i;
    double* q = out + (size_t)i * TSDF_POSE;
    store_cam_T_world(T, q);
    q[12] = stats[(size_t)i * ALIGN_STATS] != 1 ? 1.0 : 0.0;   // every frame but an UNUSED one
}

void launch_tsdf_align(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfRenderArgs& r,
                       const TsdfAlignArgs& a, double* poses, hipStream_t s) {
    if (a.n <= 0) return;
    launch_tsdf_render(c, pair, f0, host_wTc_dev, r, a.n, poses, s);
    TsdfAlignArgs b = a;
    b.poses = poses;
    hipLaunchKernelGGL(k_align_begin, dim3((b.n + 63) / 64), dim3(64), 0, s, b);
    const int tx = (b.W + ALIGN_TILE - 1) / ALIGN_TILE, ty = (b.H + ALIGN_TILE - 1) / ALIGN_TILE;
    for (int it = 1; it <= b.iterations; ++it) {
        hipLaunchKernelGGL(k_align_accumulate, dim3((unsigned)(tx * ty), (unsigned)b.n), dim3(256), 0, s, b, tx);
        hipLaunchKernelGGL(k_align_solve, dim3((unsigned)b.n), dim3(256), 0, s, b, it);
    }
}

void launch_align_poses(const double* wTc, const int32_t* stats, int n, double* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_align_poses, dim3((n + 63) / 64), dim3(64), 0, s, wTc, stats, n, out);
}
