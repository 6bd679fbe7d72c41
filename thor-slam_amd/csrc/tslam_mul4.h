// tslam_mul4.h — the 4x4 product with a fixed summation order, shared by the kernels whose results
// the NumPy oracle restates bit for bit (oracle/numpy_rig.py mul4): k_pose.hip (the rig's body
// motion) and k_tsdf.hip (the rig's camera poses for the dense map).
#pragma once

__device__ __forceinline__ void mul4_fixed(const double* A, const double* B, double* out) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            out[4 * i + j] = ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
}
