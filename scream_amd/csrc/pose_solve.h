// The pose from a 3x3 covariance and the workgroup sum in a fixed order, shared by kabsch.hip (the A9 solve, the point loss) and
// icp_p2p.hip (the ICP update and its chunk partials).  Everything lives in an anonymous namespace: each file that includes this
// gets its own copy.  Compile with -ffp-contract=off.
#pragma once
#include "common.h"
#include "svd3.h"  // dot3, jacobi_svd3, det3: shared with icp_raw.hip

namespace {

// R = V diag(1,1,det(V U^T)) U^T; t = cB - R cA (utils.py:169-175).  Writes a row-major 4x4.
__device__ void solve_pose(const double H[3][3], const float cA[3], const float cB[3], float* T) {
    double U[3][3], V[3][3], sig[3];
    jacobi_svd3(H, U, V, sig);
    const double delta = det3(V) * det3(U);  // det(V U^T)
    float R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            R[i][j] = (float)(V[i][0] * U[j][0] + V[i][1] * U[j][1] + delta * V[i][2] * U[j][2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double rc = (double)R[i][0] * cA[0] + (double)R[i][1] * cA[1] + (double)R[i][2] * cA[2];
        T[i * 4 + 0] = R[i][0];
        T[i * 4 + 1] = R[i][1];
        T[i * 4 + 2] = R[i][2];
        T[i * 4 + 3] = (float)((double)cB[i] - rc);
    }
    T[12] = 0.f;
    T[13] = 0.f;
    T[14] = 0.f;
    T[15] = 1.f;
}

// Workgroup-wide sum of NV doubles per thread; result broadcast to every thread.  NT threads (256: the A9 solve; 1024:
// the ICP update), combined in a fixed order -- waves pairwise, then groups of four -- so the sum depends on NT and on
// nothing else.
template <int NV, int NT = 256>
__device__ void block_sum(double (&v)[NV], double* red /* [NT / 64][NV] */) {
    constexpr int NW = NT / 64;
    static_assert(NW == 4 || NW == 8 || NW == 16, "");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum_f64(v[k]);
    __syncthreads();  // red may still be read from a previous call
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wave * NV + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double q4[NW / 4];
#pragma unroll
        for (int g = 0; g < NW / 4; ++g)
            q4[g] = (red[(4 * g + 0) * NV + k] + red[(4 * g + 1) * NV + k]) + (red[(4 * g + 2) * NV + k] + red[(4 * g + 3) * NV + k]);
        v[k] = NW == 4 ? q4[0] : NW == 8 ? q4[0] + q4[1 % (NW / 4)] : (q4[0] + q4[1 % (NW / 4)]) + (q4[2 % (NW / 4)] + q4[3 % (NW / 4)]);
    }
}

}  // namespace
