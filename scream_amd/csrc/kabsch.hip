// A8 + A9 + A10: correspondence gather fused into the weighted Kabsch / Procrustes solve, and RE/TE.
//
// Reference: evaluate_3d_match.py:96-101 (gather), utils.py:138-178 (rigid_transform_3d; the reference
// builds a dense K x K diag_embed and runs the 3x3 SVD on the HOST via H.cpu()), utils.py:181-189.
// Here one workgroup owns one pair: two streaming passes over the correspondences (centroids, then
// the 3x3 covariance H), sums carried in fp64 and reduced wave -> workgroup deterministically, then
// the 3x3 SVD as a one-sided (Hestenes) Jacobi sweep held entirely in registers, evaluated redundantly by
// every lane of wave 0 (the data is wave-uniform; no LDS, no divergence).  The rotation
// R = V diag(1,1,det(V U^T)) U^T is invariant to the sign/order ambiguities of the SVD whenever the
// reference's own result is well defined, so parity is checked on R|t, not on U, S, V.
// Compiled with -ffp-contract=off: the fp32 steps (x / s + c, x - centroid, sum / (K + 1e-6)) are the
// reference's individually rounded operations.
#include "common.h"
#include "pose_solve.h"  // solve_pose, block_sum: shared with icp_p2p.hip

namespace {

struct CorrFetch {  // evaluate_3d_match.py:96-101
    const float* src;
    const float* ref;
    const int32_t* idx;
    const uint8_t* valid;
    int64_t src_row0, ref_row0;
    float s, c0, c1, c2;
    int n;
    __device__ __forceinline__ bool get(int i, float a[3], float b[3], float& w) const {
        const int64_t row = src_row0 + i;
        if (!valid[row]) return false;
        const int64_t rrow = ref_row0 + (idx ? (int64_t)idx[row] : (int64_t)i);
        a[0] = src[row * 3 + 0] / s + c0;
        a[1] = src[row * 3 + 1] / s + c1;
        a[2] = src[row * 3 + 2] / s + c2;
        b[0] = ref[rrow * 3 + 0] / s + c0;
        b[1] = ref[rrow * 3 + 1] / s + c1;
        b[2] = ref[rrow * 3 + 2] / s + c2;
        w = 1.0f;
        return true;
    }
};

struct DenseFetch {  // utils.py:138-151
    const float* A;
    const float* B;
    const float* w;
    float thr;
    int n;
    __device__ __forceinline__ bool get(int i, float a[3], float b[3], float& wt) const {
        wt = w ? w[i] : 1.0f;
        if (wt < thr) wt = 0.f;  // weights[weights < weight_threshold] = 0
        if (wt == 0.f) return false;
        a[0] = A[i * 3 + 0];
        a[1] = A[i * 3 + 1];
        a[2] = A[i * 3 + 2];
        b[0] = B[i * 3 + 0];
        b[1] = B[i * 3 + 1];
        b[2] = B[i * 3 + 2];
        return true;
    }
};

template <class Fetch, int NT = 256>
__device__ void kabsch_block(const Fetch& f, float* T_out, int32_t* n_corr_out) {
    __shared__ double red[NT / 64 * 9];
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < f.n; i += NT) {
        float a[3], b[3], w;
        if (f.get(i, a, b, w)) {
            acc[0] += (double)(a[0] * w);
            acc[1] += (double)(a[1] * w);
            acc[2] += (double)(a[2] * w);
            acc[3] += (double)(b[0] * w);
            acc[4] += (double)(b[1] * w);
            acc[5] += (double)(b[2] * w);
            acc[6] += (double)w;
            acc[7] += 1.0;
        }
    }
    block_sum<9, NT>(acc, red);
    const float denom = (float)acc[6] + 1e-6f;  // utils.py:155-158
    const float cA[3] = {(float)acc[0] / denom, (float)acc[1] / denom, (float)acc[2] / denom};
    const float cB[3] = {(float)acc[3] / denom, (float)acc[4] / denom, (float)acc[5] / denom};
    const int count = (int)acc[7];

    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = 0.0;
    for (int i = threadIdx.x; i < f.n; i += NT) {
        float a[3], b[3], w;
        if (f.get(i, a, b, w)) {
            const float am[3] = {a[0] - cA[0], a[1] - cA[1], a[2] - cA[2]};
            const float bm[3] = {(b[0] - cB[0]) * w, (b[1] - cB[1]) * w, (b[2] - cB[2]) * w};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) h[r * 3 + c] += (double)am[r] * (double)bm[c];
        }
    }
    block_sum<9, NT>(h, red);
    if (threadIdx.x < 64) {  // wave 0, every lane redundantly (wave-uniform data)
        double H[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) H[r][c] = (double)(float)h[r * 3 + c];  // the reference holds H in fp32
        float T[16];
        solve_pose(H, cA, cB, T);
        if (threadIdx.x < 16) T_out[threadIdx.x] = T[threadIdx.x];
        if (threadIdx.x == 0 && n_corr_out) *n_corr_out = count;
    }
}

__global__ __launch_bounds__(256) void kabsch_corr_kernel(const float* __restrict__ src, const float* __restrict__ ref,
                                                         const int32_t* __restrict__ src_row0,
                                                         const int32_t* __restrict__ src_len,
                                                         const int32_t* __restrict__ ref_row0,
                                                         const int32_t* __restrict__ idx,
                                                         const uint8_t* __restrict__ valid,
                                                         const float* __restrict__ s, const float* __restrict__ c,
                                                         float* __restrict__ T_out, int32_t* __restrict__ n_corr) {
    const int p = blockIdx.x;
    CorrFetch f{src, ref, idx, valid, src_row0[p], ref_row0[p], s[p], c[p * 3 + 0], c[p * 3 + 1], c[p * 3 + 2],
                src_len[p]};
    kabsch_block(f, T_out + p * 16, n_corr ? n_corr + p : nullptr);
}

__global__ __launch_bounds__(256) void kabsch_dense_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                          const float* __restrict__ w, float thr, int K,
                                                          float* __restrict__ T_out) {
    const int p = blockIdx.x;
    DenseFetch f{A + (int64_t)p * K * 3, B + (int64_t)p * K * 3, w ? w + (int64_t)p * K : nullptr, thr, K};
    kabsch_block(f, T_out + p * 16, nullptr);
}

// utils.py:181-189 with the fp32 operation order of torch-CPU (3-term fma chains for the 3x3 product).
__global__ __launch_bounds__(64) void transformation_error_kernel(const float* __restrict__ Tp,
                                                                 const float* __restrict__ Tg, int n,
                                                                 float* __restrict__ re, float* __restrict__ te) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* P = Tp + i * 16;
    const float* G = Tg + i * 16;
    float diag[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        float d = P[0 * 4 + j] * G[0 * 4 + j];
        d = __fmaf_rn(P[1 * 4 + j], G[1 * 4 + j], d);
        d = __fmaf_rn(P[2 * 4 + j], G[2 * 4 + j], d);
        diag[j] = d;
    }
    const float tr = (diag[0] + diag[1]) + diag[2];
    float x = (tr - 1.0f) / 2.0f;
    x = fminf(fmaxf(x, -1.0f), 1.0f);
    re[i] = (acosf(x) * 180.0f) / 3.14159265358979323846f;
    const float dx = P[3] - G[3], dy = P[7] - G[7], dz = P[11] - G[11];
    te[i] = sqrtf((dx * dx + dy * dy) + dz * dz);
}

// loss[p] = mean_n sum_xyz |pred_n - (R_p a_n + t_p)| (models/pointnet.py:93-99, the L1 point loss the evaluators report per pair).
// One workgroup per pair; the terms in fp32 like the reference's, their sum in fp64 in a fixed order (the torch expression costs
// seven small launches per pair).
__global__ __launch_bounds__(256) void point_loss_kernel(const float* __restrict__ pred, const float* __restrict__ src,
                                                        const int32_t* __restrict__ row0, const int32_t* __restrict__ len,
                                                        const float* __restrict__ R, const float* __restrict__ t,
                                                        float* __restrict__ out) {
    __shared__ double red[4];
    const int p = blockIdx.x, n = len[p];
    const int64_t r0 = row0[p];
    const float* Rp = R + p * 9;
    const float* tp = t + p * 3;
    double acc[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += 256) {
        const float x = src[(r0 + i) * 3 + 0], y = src[(r0 + i) * 3 + 1], z = src[(r0 + i) * 3 + 2];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float reg = ((Rp[k * 3 + 0] * x + Rp[k * 3 + 1] * y) + Rp[k * 3 + 2] * z) + tp[k];
            s += fabsf(pred[(r0 + i) * 3 + k] - reg);
        }
        acc[0] += (double)s;
    }
    block_sum<1, 256>(acc, red);
    if (threadIdx.x == 0) out[p] = n > 0 ? (float)(acc[0] / n) : 0.f;
}

}  // namespace

extern "C" int scream_kabsch_corr(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                                  const int32_t* ref_row0, const int32_t* idx, const uint8_t* valid, const float* s,
                                  const float* c, int32_t n_pairs, float* T_out, int32_t* n_corr, void* stream) {
    SCREAM_REQUIRE(src && ref && src_row0 && src_len && ref_row0 && valid && s && c && T_out, SCREAM_EINVAL);
    SCREAM_REQUIRE(n_pairs >= 0, SCREAM_EINVAL);
    if (n_pairs == 0) return 0;
    kabsch_corr_kernel<<<dim3(n_pairs), dim3(256), 0, as_stream(stream)>>>(src, ref, src_row0, src_len, ref_row0, idx,
                                                                           valid, s, c, T_out, n_corr);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_rigid_transform_3d(const float* A, const float* B, const float* w, float weight_threshold,
                                         int32_t bs, int32_t K, float* T_out, void* stream) {
    SCREAM_REQUIRE(T_out && bs >= 0 && K >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(K == 0 || (A && B), SCREAM_EINVAL);
    if (bs == 0) return 0;
    kabsch_dense_kernel<<<dim3(bs), dim3(256), 0, as_stream(stream)>>>(A, B, w, weight_threshold, K, T_out);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_point_loss(const float* src_pred, const float* src, const int32_t* src_row0, const int32_t* src_len,
                                 const float* rot, const float* trans, int32_t n_pairs, float* loss, void* stream) {
    SCREAM_REQUIRE(src_pred && src && src_row0 && src_len && rot && trans && loss && n_pairs >= 0, SCREAM_EINVAL);
    if (n_pairs == 0) return 0;
    point_loss_kernel<<<dim3(n_pairs), dim3(256), 0, as_stream(stream)>>>(src_pred, src, src_row0, src_len, rot, trans, loss);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_transformation_error(const float* T_pred, const float* T_gt, int32_t n, float* re, float* te,
                                           void* stream) {
    SCREAM_REQUIRE(T_pred && T_gt && re && te && n >= 0, SCREAM_EINVAL);
    if (n == 0) return 0;
    transformation_error_kernel<<<dim3((n + 63) / 64), dim3(64), 0, as_stream(stream)>>>(T_pred, T_gt, n, re, te);
    SCREAM_LAUNCH_CHECK();
    return 0;
}
