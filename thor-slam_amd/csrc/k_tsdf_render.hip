// k_tsdf_render.hip — the dense map seen from a pose: TSDF ray casting (tslam_tsdf_render).
// Spec and CPU restatement: thor_slam_amd/dense_render.py (rules 1-6; every f64 operation below is
// one of its written operations, in its order; -ffp-contract=off keeps them unfused).
//
//   k_render_poses   per view: world_T_cam's rotation rows (9), the camera centre (3) and a use
//                    flag, from the host's world_T_cam or from the batch's device-resident chained
//                    poses (k_tsdf_poses' frame selection and tracked-status rule; the ray caster
//                    wants world_T_cam as it stands, so nothing is inverted);
//   k_tsdf_render    one thread per pixel, a wave per 8 x 8 pixel tile (coherent rays: the
//                    gathers of neighbouring lanes land in neighbouring lines), a 256-thread block
//                    per 16 x 16 pixels, grid = tiles x views.  The view's pose entry and the
//                    window record are read with uniform loads.  Every pixel of the call's views is
//                    written (zeros at a miss and in an unused view), so the images need no clear.
//                    No atomics, no acceleration structure: the samples of a ray are rule 5's.
#include "tslam_common.h"

__global__ void k_render_poses(BatchCtx c, int pair, int f0, const double* host_wTc, int n, double* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double use = 1.0;   // 0: a zero image
    const double* T = call_pose(c, pair, f0, host_wTc, i, &use);
    double* q = out + (size_t)i * TSDF_POSE;
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) q[3 * r + k] = T[4 * r + k];
        q[9 + r] = T[4 * r + 3];
    }
    q[12] = use;
}

__device__ __forceinline__ double render_lerp(double p, double q, double u) { return p + u * (q - p); }

// Rule 4 at grid coordinates g: false when the cell is not valid or a corner is unobserved.  The
// sixteen loads are issued together, before the first use.
__device__ __forceinline__ bool render_sample(const TsdfRenderArgs& a, double gx, double gy, double gz, double& f) {
    const double bx = floor(gx), by = floor(gy), bz = floor(gz);
    // in floating point before any conversion: a NaN or a huge coordinate is "not valid"
    if (!(bx >= 0.0 && bx <= (double)(a.nx - 2) && by >= 0.0 && by <= (double)(a.ny - 2) && bz >= 0.0 && bz <= (double)(a.nz - 2)))
        return false;
    const size_t sy = (size_t)a.nx, sz = (size_t)a.nx * a.ny;
    const size_t v = ((size_t)(int)bz * a.ny + (size_t)(int)by) * a.nx + (size_t)(int)bx;
    const float* __restrict__ tp = a.tsdf + v;
    const float* __restrict__ wp = a.weight + v;
    const float w0 = wp[0], w1 = wp[1], w2 = wp[sy], w3 = wp[sy + 1];
    const float w4 = wp[sz], w5 = wp[sz + 1], w6 = wp[sz + sy], w7 = wp[sz + sy + 1];
    const float t0 = tp[0], t1 = tp[1], t2 = tp[sy], t3 = tp[sy + 1];
    const float t4 = tp[sz], t5 = tp[sz + 1], t6 = tp[sz + sy], t7 = tp[sz + sy + 1];
    const double mw = a.min_weight;
    // `&`, not `&&`: a short-circuit chain lets the compiler sink seven weight loads behind the first
    // comparison, a second dependent round trip per sample
    const bool known = ((double)w0 >= mw) & ((double)w1 >= mw) & ((double)w2 >= mw) & ((double)w3 >= mw) & ((double)w4 >= mw) &
                       ((double)w5 >= mw) & ((double)w6 >= mw) & ((double)w7 >= mw);
    const double ux = gx - bx, uy = gy - by, uz = gz - bz;
    const double c00 = render_lerp((double)t0, (double)t1, ux), c10 = render_lerp((double)t2, (double)t3, ux);
    const double c01 = render_lerp((double)t4, (double)t5, ux), c11 = render_lerp((double)t6, (double)t7, ux);
    f = render_lerp(render_lerp(c00, c10, uy), render_lerp(c01, c11, uy), uz);
    return known;
}

#define RENDER_TILE 16   // pixels per block side; a wave owns an 8 x 8 quarter

__global__ __launch_bounds__(256) void k_tsdf_render(TsdfRenderArgs a, int tiles_x) {
    const int view = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = (blockIdx.x % tiles_x) * RENDER_TILE + (wave & 1) * 8 + (lane & 7);
    const int y = (blockIdx.x / tiles_x) * RENDER_TILE + (wave >> 1) * 8 + (lane >> 3);
    if (x >= a.W || y >= a.H) return;   // partial tiles: masked lanes (no barrier below)
    const size_t px = (size_t)y * a.W + x, o = (size_t)view * a.W * a.H + px;
    const double* __restrict__ q = a.poses + (size_t)view * TSDF_POSE;   // uniform: scalar loads

    double tstar = 0.0, gsx = 0.0, gsy = 0.0, gsz = 0.0;
    bool hit = false;
    if (q[12] != 0.0) {
        double ox = a.ox, oy = a.oy, oz = a.oz;
        if (a.win) {   // the rolling window: the corner from the cumulative shift (three uniform loads)
            ox = a.ox + a.s * (double)a.win->shift[0];
            oy = a.oy + a.s * (double)a.win->shift[1];
            oz = a.oz + a.s * (double)a.win->shift[2];
        }
        // 1, 2: the ray in grid coordinates
        const double dc0 = ((double)x - a.cx) / a.fx, dc1 = ((double)y - a.cy) / a.fy;
        const double L = a.L[px];
        const double g0x = (q[9] - ox) / a.s - 0.5, g0y = (q[10] - oy) / a.s - 0.5, g0z = (q[11] - oz) / a.s - 0.5;
        const double gdx = ((q[0] * dc0 + q[1] * dc1) + q[2]) / a.s;
        const double gdy = ((q[3] * dc0 + q[4] * dc1) + q[5]) / a.s;
        const double gdz = ((q[6] * dc0 + q[7] * dc1) + q[8]) / a.s;
        // 3: clip against [min_depth, max_depth] and the three slabs
        double t = a.min_depth, t1 = a.max_depth;
        bool active = true;
        {
            const double g0[3] = {g0x, g0y, g0z}, gd[3] = {gdx, gdy, gdz};
            const double top[3] = {(double)(a.nx - 1), (double)(a.ny - 1), (double)(a.nz - 1)};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (gd[k] == 0.0) {
                    if (g0[k] < 0.0 || g0[k] > top[k]) active = false;
                } else {
                    const double qa = (0.0 - g0[k]) / gd[k], qb = (top[k] - g0[k]) / gd[k];
                    t = fmax(t, fmin(qa, qb));
                    t1 = fmin(t1, fmax(qa, qb));
                }
            }
            if (!(t <= t1)) active = false;
        }
        // 5: march; the wave leaves the loop when its last ray has ended
        bool has = false;
        double fp = 0.0, tp = 0.0;
        int left = a.nx + a.ny + a.nz + 2;
        while (__ballot(active)) {
            if (active) {
                double f = 0.0;
                const bool known = render_sample(a, g0x + t * gdx, g0y + t * gdy, g0z + t * gdz, f);
                if (known && has && f <= 0.0) {
                    tstar = tp + (t - tp) * (fp / (fp - f));
                    hit = true;
                    active = false;
                } else {
                    has = known && f > 0.0;
                    fp = f;
                    tp = t;
                    t = t + (has ? fmax(a.step_scale * f, a.s) : a.s) / L;
                    if (t > t1 || --left == 0) active = false;
                }
            }
        }
        gsx = g0x + tstar * gdx;
        gsy = g0y + tstar * gdy;
        gsz = g0z + tstar * gdz;
    }

    // 6: outputs (zeros at a miss and in an unused view)
    if (a.depth_m) a.depth_m[o] = hit ? (float)tstar : 0.0f;
    if (a.depth_mm) {
        const double mm = floor(1000.0 * tstar + 0.5);
        a.depth_mm[o] = (hit && mm >= 1.0 && mm <= 65535.0) ? (uint16_t)(int)mm : (uint16_t)0;
    }
    if (a.normal) {
        float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
        if (hit) {
            double fa = 0.0, fb = 0.0;
            bool ok = render_sample(a, gsx + 0.5, gsy, gsz, fa);
            ok = render_sample(a, gsx - 0.5, gsy, gsz, fb) && ok;
            const double gx = fa - fb;
            ok = render_sample(a, gsx, gsy + 0.5, gsz, fa) && ok;
            ok = render_sample(a, gsx, gsy - 0.5, gsz, fb) && ok;
            const double gy = fa - fb;
            ok = render_sample(a, gsx, gsy, gsz + 0.5, fa) && ok;
            ok = render_sample(a, gsx, gsy, gsz - 0.5, fb) && ok;
            const double gz = fa - fb;
            if (ok) {
                const double nn = sqrt((gx * gx + gy * gy) + gz * gz);
                if (nn > 0.0) {
                    n0 = (float)(gx / nn);
                    n1 = (float)(gy / nn);
                    n2 = (float)(gz / nn);
                }
            }
        }
        float* np = a.normal + 3 * o;
        np[0] = n0;
        np[1] = n1;
        np[2] = n2;
    }
    if (a.color) {
        uint8_t b = 0, g = 0, r = 0;
        if (hit && a.col) {
            const double vx = fmin(fmax(floor(gsx + 0.5), 0.0), (double)(a.nx - 1));
            const double vy = fmin(fmax(floor(gsy + 0.5), 0.0), (double)(a.ny - 1));
            const double vz = fmin(fmax(floor(gsz + 0.5), 0.0), (double)(a.nz - 1));
            const size_t v = ((size_t)(int)vz * a.ny + (size_t)(int)vy) * a.nx + (size_t)(int)vx;
            if (a.col_w[v] > 0.0f) {
                r = (uint8_t)(int)fmin(fmax(floor((double)a.col[3 * v] + 0.5), 0.0), 255.0);
                g = (uint8_t)(int)fmin(fmax(floor((double)a.col[3 * v + 1] + 0.5), 0.0), 255.0);
                b = (uint8_t)(int)fmin(fmax(floor((double)a.col[3 * v + 2] + 0.5), 0.0), 255.0);
            }
        }
        uint8_t* cp = a.color + 3 * o;
        cp[0] = b;
        cp[1] = g;
        cp[2] = r;
    }
}

void launch_tsdf_render(const BatchCtx& c, int pair, int f0, const double* host_wTc_dev, const TsdfRenderArgs& a, int n_views,
                        double* poses, hipStream_t s) {
    if (n_views <= 0) return;
    hipLaunchKernelGGL(k_render_poses, dim3((n_views + 63) / 64), dim3(64), 0, s, c, pair, f0, host_wTc_dev, n_views, poses);
    TsdfRenderArgs b = a;
    b.poses = poses;
    const int tx = (a.W + RENDER_TILE - 1) / RENDER_TILE, ty = (a.H + RENDER_TILE - 1) / RENDER_TILE;
    hipLaunchKernelGGL(k_tsdf_render, dim3((unsigned)(tx * ty), (unsigned)n_views), dim3(256), 0, s, b, tx);
}
