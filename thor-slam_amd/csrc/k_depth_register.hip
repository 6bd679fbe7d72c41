// k_depth_register.hip — depth registration: the depth of a pair's rectified left camera
// forward-warped into a colour camera with a z-buffer (tslam_depth_register).  Spec:
// thor_slam_amd/depth_register.py; restated for the tests in tests/ref_depth_register.py.
//
// Three launches per call, every frame of the call in each of them (the frame on grid axis y):
//
//   k_dr_clear    the call's z-buffer planes (u32 [n][Hc][Wc], row-major, dense) set to empty
//                 (0xffffffff), 16 B per lane;
//   k_dr_splat    one thread per depth pixel: rules 1 and 2, then a 32-bit atomicMin without a
//                 return value on every covered pixel of its frame's plane.  A wave holds 64
//                 neighbouring depth pixels of a row; at footprint offset (dx, dy) its lanes hit
//                 neighbouring words of one colour row, so a wave's atomics of one offset fall into
//                 a few contiguous segments (the shape the memory-side atomics take best);
//   k_dr_gather   one thread per index of the larger of the two images: as a depth pixel it
//                 recomputes rule 1 with the same operations, compares against the finished plane
//                 and writes bgr and mask (rule 4); as a colour pixel it converts the plane to the
//                 registered depth u16 (rule 5).  The plane is only read here.
//
// The minimum makes the result independent of the order the atomics arrive in.  All arithmetic is
// f64 in the spec's written order (the build has -ffp-contract=off).
#include <algorithm>

#include "tslam_common.h"

#define DR_EMPTY 0xffffffffu
#define DR_REACH 8.0   // the footprint reaches at most 8 pixels from the nearest one (rule 2)

struct DrProj {
    double u, v, s;      // projection and z / Qz
    int nu, nv;          // nearest colour pixel (may lie up to 8 pixels outside the image)
    uint32_t zc;         // mm in the colour camera
};

// rule 1; false: invalid depth, behind the colour camera, zc out of range, or farther than the
// footprint's reach outside the image (also what a NaN gives)
__device__ __forceinline__ bool dr_project(const DepthRegArgs& a, int x, int y, uint32_t D, DrProj& p) {
    if (D == 0u || D > (uint32_t)a.max_depth_mm) return false;
    const double z = (double)D * 0.001;
    const double P0 = (((double)x - a.cx) / a.fx) * z, P1 = (((double)y - a.cy) / a.fy) * z;
    const double qx = ((a.T[0] * P0 + a.T[1] * P1) + a.T[2] * z) + a.T[3];
    const double qy = ((a.T[4] * P0 + a.T[5] * P1) + a.T[6] * z) + a.T[7];
    const double qz = ((a.T[8] * P0 + a.T[9] * P1) + a.T[10] * z) + a.T[11];
    if (!(qz > 0.0)) return false;
    const double zc = floor(qz * 1000.0 + 0.5);
    if (!(zc >= 1.0 && zc <= 65535.0)) return false;
    p.u = a.fc * qx / qz + a.cxc;
    p.v = a.fc * qy / qz + a.cyc;
    const double fu = floor(p.u + 0.5), fv = floor(p.v + 0.5);
    if (!(fu >= -DR_REACH && fu < (double)a.Wc + DR_REACH && fv >= -DR_REACH && fv < (double)a.Hc + DR_REACH)) return false;
    p.nu = (int)fu;
    p.nv = (int)fv;
    p.zc = (uint32_t)zc;
    p.s = z / qz;
    return true;
}

// rule 2 on one axis: the covered pixels lo .. hi around the nearest pixel n
__device__ __forceinline__ void dr_footprint(double c, double h, int n, int max_splat, int& lo, int& hi) {
    const double dn = (double)n;
    lo = (int)fmax(ceil(c - h), dn - DR_REACH);
    hi = (int)fmin(ceil(c + h) - 1.0, dn + DR_REACH);
    lo = min(lo, n);
    hi = max(hi, n);
    if (hi - lo + 1 > max_splat) {
        lo = n - ((max_splat - 1) >> 1);
        hi = n + (max_splat >> 1);
    }
}

__global__ __launch_bounds__(256) void k_dr_clear(uint32_t* __restrict__ z, size_t count) {
    const size_t quads = count >> 2;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, tn = (size_t)gridDim.x * blockDim.x;
    uint4* z4 = reinterpret_cast<uint4*>(z);
    for (size_t i = t0; i < quads; i += tn) z4[i] = make_uint4(DR_EMPTY, DR_EMPTY, DR_EMPTY, DR_EMPTY);
    if (t0 < (count & 3)) z[(quads << 2) + t0] = DR_EMPTY;
}

__global__ __launch_bounds__(256) void k_dr_splat(DepthRegArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= a.W * a.H) return;
    const int x = i % a.W, y = i / a.W;
    const uint16_t* depth = reinterpret_cast<const uint16_t*>(a.depth + (size_t)f * a.depth_stride);
    DrProj p;
    if (!dr_project(a, x, y, depth[i], p)) return;
    int lx, hx, ly, hy;
    dr_footprint(p.u, (0.5 * (a.fc / a.fx)) * p.s, p.nu, a.max_splat, lx, hx);
    dr_footprint(p.v, (0.5 * (a.fc / a.fy)) * p.s, p.nv, a.max_splat, ly, hy);
    lx = max(lx, 0);
    ly = max(ly, 0);
    hx = min(hx, a.Wc - 1);
    hy = min(hy, a.Hc - 1);
    uint32_t* Z = a.zbuf + (size_t)f * a.Wc * a.Hc;
    for (int iv = ly; iv <= hy; ++iv)
        for (int iu = lx; iu <= hx; ++iu) atomicMin(&Z[(size_t)iv * a.Wc + iu], p.zc);
}

__global__ __launch_bounds__(256) void k_dr_gather(DepthRegArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    const size_t cpx = (size_t)a.Wc * a.Hc, dpx = (size_t)a.W * a.H;
    const uint32_t* Z = a.zbuf + (size_t)f * cpx;
    if ((size_t)i < dpx) {
        const int x = i % a.W, y = i / a.W;
        const uint16_t* depth = reinterpret_cast<const uint16_t*>(a.depth + (size_t)f * a.depth_stride);
        uint8_t b = 0, g = 0, r = 0, m = 0;
        DrProj p;
        if (dr_project(a, x, y, depth[i], p) && p.nu >= 0 && p.nu < a.Wc && p.nv >= 0 && p.nv < a.Hc) {
            const size_t c = (size_t)p.nv * a.Wc + p.nu;
            // the pixel's own splat landed here, so Z <= zc; a nearer surface by more than tol hides it
            if (p.zc - Z[c] <= (uint32_t)a.tol_mm) {
                int rx = p.nu, ry = p.nv;
                if (a.map) {
                    rx = min(max((a.map[2 * c] + 16) >> 5, 0), a.Wc - 1);
                    ry = min(max((a.map[2 * c + 1] + 16) >> 5, 0), a.Hc - 1);
                }
                const uint8_t* px = a.color + (size_t)f * a.color_stride + ((size_t)ry * a.Wc + rx) * 3;
                b = px[0], g = px[1], r = px[2], m = 1;
            }
        }
        uint8_t* o = a.bgr + ((size_t)f * dpx + i) * 3;
        o[0] = b, o[1] = g, o[2] = r;
        a.mask[(size_t)f * dpx + i] = m;
    }
    if ((size_t)i < cpx) {
        const uint32_t z = Z[i];
        a.reg[(size_t)f * cpx + i] = z == DR_EMPTY ? (uint16_t)0 : (uint16_t)z;
    }
}

#define DR_CLEAR_BLOCKS 2048
hipError_t launch_depth_register(const DepthRegArgs& a, hipStream_t s, hipEvent_t* ev) {
    if (a.n <= 0) return hipSuccess;
    const size_t cpx = (size_t)a.Wc * a.Hc, dpx = (size_t)a.W * a.H, count = cpx * a.n;
    const unsigned cb = (unsigned)std::min<size_t>(((count >> 2) + 255) / 256 + 1, DR_CLEAR_BLOCKS);
    if (ev) (void)hipEventRecord(ev[0], s);
    hipLaunchKernelGGL(k_dr_clear, dim3(cb), dim3(256), 0, s, a.zbuf, count);
    if (ev) (void)hipEventRecord(ev[1], s);
    hipLaunchKernelGGL(k_dr_splat, dim3((unsigned)((dpx + 255) / 256), (unsigned)a.n), dim3(256), 0, s, a);
    if (ev) (void)hipEventRecord(ev[2], s);
    hipLaunchKernelGGL(k_dr_gather, dim3((unsigned)((std::max(dpx, cpx) + 255) / 256), (unsigned)a.n), dim3(256), 0, s, a);
    if (ev) (void)hipEventRecord(ev[3], s);
    return hipGetLastError();
}
