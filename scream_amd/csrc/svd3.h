// The float64 3x3 singular value decomposition shared by the pose solves (kabsch.hip: the A9 solve; icp_p2p.hip: the ICP update
// of scream_icp_p2p; icp_raw.hip: the update of scream_icp_raw): a one-sided (Hestenes) Jacobi sweep held entirely in registers.
// Every file that includes this is compiled with -ffp-contract=off.  tests/pose_ref.py (jacobi_svd3) restates it.
#pragma once
#include <math.h>

namespace {

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Columns g[c][0..2] of G = H V and v[c][0..2] of V.  After convergence G's columns are orthogonal:
// H = U S V^T with s_c = |g_c|, u_c = g_c / s_c.
__device__ void jacobi_svd3(const double H[3][3], double U[3][3], double V[3][3], double sig[3]) {
    double g[3][3], v[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            g[c][i] = H[i][c];
            v[c][i] = (i == c) ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = (pq == 2) ? 1 : 0;
            const int q = (pq == 0) ? 1 : 2;
            const double alpha = dot3(g[p], g[p]), beta = dot3(g[q], g[q]), gamma = dot3(g[p], g[q]);
            // scale-free: |cos| of the angle between the two columns against 1e-16, whatever |H| (an absolute term here stopped the
            // sweep early for |H| < 1e-13 and skipped it altogether below 1e-15; the reference's LAPACK SVD is scale-invariant).
            // alpha * beta cannot leave the double range for any fp32 H; gamma == 0 covers a zero column.
            const double lim = 1e-16 * sqrt(alpha * beta);
            if (gamma != 0.0 && fabs(gamma) > lim) {
                off += fabs(gamma);
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double gp = g[p][i], gq = g[q][i];
                    g[p][i] = cs * gp - sn * gq;
                    g[q][i] = sn * gp + cs * gq;
                    const double vp = v[p][i], vq = v[q][i];
                    v[p][i] = cs * vp - sn * vq;
                    v[q][i] = sn * vp + cs * vq;
                }
            }
        }
        if (off == 0.0) break;
    }
    double s[3] = {sqrt(dot3(g[0], g[0])), sqrt(dot3(g[1], g[1])), sqrt(dot3(g[2], g[2]))};
    // sort columns by descending singular value (LAPACK order; the det fix applies to the smallest)
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int a = (pass == 1) ? 1 : 0, b = a + 1;
        if (s[a] < s[b]) {
            const double ts = s[a];
            s[a] = s[b];
            s[b] = ts;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double tg = g[a][i];
                g[a][i] = g[b][i];
                g[b][i] = tg;
                tg = v[a][i];
                v[a][i] = v[b][i];
                v[b][i] = tg;
            }
        }
    }
    double u[3][3];
    if (!(s[0] > 0.0)) {
        // H == 0 (no correspondences): torch.svd returns U = V = I -> identity transform (utils.py:155-175)
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                u[c][i] = (i == c) ? 1.0 : 0.0;
                v[c][i] = (i == c) ? 1.0 : 0.0;
            }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) u[0][i] = g[0][i] / s[0];
        if (s[1] > 1e-14 * s[0]) {
#pragma unroll
            for (int i = 0; i < 3; ++i) u[1][i] = g[1][i] / s[1];
        } else {
            // rank 1: any unit vector orthogonal to u0 (rotation about u0 is undetermined in the reference too)
            const int k = (fabs(u[0][0]) <= fabs(u[0][1]) && fabs(u[0][0]) <= fabs(u[0][2])) ? 0
                          : (fabs(u[0][1]) <= fabs(u[0][2]) ? 1 : 2);
            double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
            const double pr = dot3(e, u[0]);
            double w[3] = {e[0] - pr * u[0][0], e[1] - pr * u[0][1], e[2] - pr * u[0][2]};
            const double nw = sqrt(dot3(w, w));
#pragma unroll
            for (int i = 0; i < 3; ++i) u[1][i] = w[i] / nw;
        }
        if (s[2] > 1e-14 * s[0]) {
#pragma unroll
            for (int i = 0; i < 3; ++i) u[2][i] = g[2][i] / s[2];
        } else {  // rank <= 2: complete the basis; the sign cancels against det(V U^T) below
            u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
            u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
            u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        sig[c] = s[c];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            U[i][c] = u[c][i];
            V[i][c] = v[c][i];
        }
    }
}

__device__ __forceinline__ double det3(const double M[3][3]) {
    return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
}

}  // namespace
