// tslam_tsdf_brick.h — what the kernels that walk the volume brick by brick share: the brick's
// shape and its view test (k_tsdf.hip: integration; k_tsdf_move_frames.hip: archived frames taken
// out of the volume and put back at a new pose; k_tsdf_freespace.hip: the free-space layer's update).
#pragma once

#include "tslam_common.h"

// Bricks of 16 x 4 x 4 voxels, one per 256-thread block (x rows of 64 B stay coalesced).  Before
// touching a voxel the block decides, one frame per thread, which frames can see ANY voxel of its
// brick: the brick's bounding sphere against the conditions the per-voxel test applies
// (p_z > 0, p_z <= max_dist + trunc, 0 <= floor(u + 1/2) < W, same for v — the four image
// borders are planes through the camera centre).  The cull is conservative (radius inflated by 1 %
// + 1 um against rounding), so every update the exact per-voxel test would make still happens,
// in frame order: results are unchanged, while (brick, frame) pairs outside the view cost one
// sphere test per block instead of a projection per voxel (nvblox's "blocks in view" step).
#define TSDF_BX 16
#define TSDF_BY 4
#define TSDF_BZ 4

__device__ __forceinline__ bool tsdf_brick_visible(const TsdfArgs& a, double fx, double fy, double cx, double cy,
                                                   const double* q, double X, double Y, double Z, double R) {
    if (q[12] == 0.0) return false;
    const double pz = ((q[6] * X + q[7] * Y) + q[8] * Z) + q[11];
    if (pz + R <= 0.0) return false;                      // every voxel has p_z <= 0
    if (pz - R > a.max_dist + a.trunc) return false;      // p_z > d + trunc for every valid depth
    const double px = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[9];
    const double py = ((q[3] * X + q[4] * Y) + q[5] * Z) + q[10];
    // u + 1/2 >= 0  <=>  fx p_x + (cx + 1/2) p_z >= 0;  u + 1/2 < W  <=>  fx p_x + (cx + 1/2 - W) p_z < 0
    const double cl = cx + 0.5, cr = cx + 0.5 - a.W, ct = cy + 0.5, cb = cy + 0.5 - a.H;
    if (fx * px + cl * pz + R * sqrt(fx * fx + cl * cl) < 0.0) return false;
    if (fx * px + cr * pz - R * sqrt(fx * fx + cr * cr) >= 0.0) return false;
    if (fy * py + ct * pz + R * sqrt(fy * fy + ct * ct) < 0.0) return false;
    if (fy * py + cb * pz - R * sqrt(fy * fy + cb * cb) >= 0.0) return false;
    return true;
}
