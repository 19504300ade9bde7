// What the weight-gradient entry points share (backward.hip: the fp32-input and the split-operand kernel; gemm_bf16.hip: one bf16
// product): the row slices and their workspace carve, the partial kernel on the 16-bit matrix cores as a template over the
// operand policy, the index-order reduce launch and the host front end.  Every reduction is a fixed-order sum written with
// ordinary vector stores: no float atomics, two identical calls are bitwise identical.
#pragma once
#include "common.h"
#include "split.h"

namespace {

constexpr int WG_T = 128;
constexpr int WG_R = 32;

// dW (+)= sum over slices in slice order; one element per thread.  Also the column sums when colpart is given.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int n_slices, int64_t nk,
                                                           float* __restrict__ dW, int accumulate,
                                                           const float* __restrict__ colpart, int N,
                                                           float* __restrict__ colsum) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < nk) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};  // four chains: slice s goes to chain s % 4
        int q = 0;
        for (; q + 4 <= n_slices; q += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += part[(int64_t)(q + u) * nk + idx];
        for (int u = 0; q + u < n_slices; ++u) s[u] += part[(int64_t)(q + u) * nk + idx];
        const float t = (s[0] + s[1]) + (s[2] + s[3]);
        dW[idx] = accumulate ? dW[idx] + t : t;
    }
    if (colpart && idx < N) {
        float t = 0.f;
        for (int q = 0; q < n_slices; ++q) t += colpart[(int64_t)q * N + idx];
        colsum[idx] = accumulate ? colsum[idx] + t : t;
    }
}

// Row slices of the weight gradient: about 1024 blocks (four per CU), at least 128 rows per slice.
int64_t wgrad_slice_rows(int64_t rows, int N, int K) {
    const int64_t tiles = (int64_t)(N / WG_T) * (K / WG_T);
    int64_t slices = (1024 + tiles - 1) / tiles;
    const int64_t max_slices = (rows + 127) / 128;
    if (slices > max_slices) slices = max_slices;
    if (slices < 1) slices = 1;
    const int64_t per = (rows + slices - 1) / slices;
    return (per + WG_R - 1) / WG_R * WG_R;
}

// ------------------------------------------------------------------------------------------------ weight gradient, split
// The same sum on the 16-bit matrix cores, a template over the operand split (split.h; instantiated for SplitBf3: bf16 keeps
// fp32's exponent range, so a gradient of any scale -- tiny, or multiplied by a loss scale of 2^16 and more -- needs no
// exponent, cannot overflow, and a power of two on dY comes out of dW bit for bit).  Same block tile (128 x 128, 4 waves of
// 64 x 64), same row slices and the same reduce launch as above.  Per 32-row chunk (two 16-deep steps):
//   * waves 0-1 stage dY, waves 2-3 stage X: thread (rg, cg) of its pair loads rows 8 rg .. 8 rg + 7 of columns 4 cg .. 4 cg + 3
//     (eight 16-byte loads, every wave instruction two full 512-byte row segments), one chunk ahead of the MFMAs;
//   * the transposing write pass: for each of its four columns the thread holds the eight consecutive ROWS -- exactly one
//     lane's operand of a 16-deep step, the row being the contraction index -- splits them once (split8<SP>) and writes one
//     16-byte vector per plane into the image [operand][plane][row group][position];
//   * column c of the tile sits at position 32 (c & 3) + (c >> 2), so that writes (32 lanes = 32 consecutive positions) and
//     fragment reads (lane i of a 32-wide MFMA tile = position 32 t + i) are both 512 contiguous bytes per half wave: no
//     bank conflicts, no padding.  An MFMA tile therefore owns the columns 4 i + t of the block tile; the epilogue undoes it.
//   * per step and wave: NP fragment reads per 32-column tile, then SP::products (six MFMAs for SplitBf3) per tile pair.
// colsum stays an fp32 sum of the unsplit dY, taken from the staging registers (rows in order, then the four row groups in
// order).  LDS: 2 NP x 4 x 128 x 16 B = 48 KiB (SplitBf3) + 2 KiB for the column sums.
constexpr int WS_G = WG_R / 8;  // row groups of eight per chunk

template <class SP>
__global__ __launch_bounds__(256) void wgrad_split_partial_kernel(const float* __restrict__ dY, int64_t ldy,
                                                                  const float* __restrict__ X, int64_t ldx, int64_t rows,
                                                                  int N, int K, int64_t slice_rows, float* __restrict__ part,
                                                                  float* __restrict__ colpart) {
    typedef typename SP::vec V;
    constexpr int NP = SP::NP;
    __shared__ __attribute__((aligned(16))) V sm[2 * NP * WS_G * WG_T];
    __shared__ float scol[WS_G * WG_T];
    const int kt = K / WG_T;
    const int n0 = (blockIdx.x / kt) * WG_T, k0 = (blockIdx.x % kt) * WG_T;
    const int64_t r_begin = (int64_t)blockIdx.y * slice_rows;
    const int64_t r_end = min(rows, r_begin + slice_rows);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1, i = lane & 31, half = lane >> 5;
    const bool do_col = colpart != nullptr && k0 == 0;
    // staging role: operand (wave uniform), row group, column group
    const int op = tid >> 7, rg = (tid >> 5) & 3, cg = tid & 31;
    const float* src = op ? X + k0 + 4 * cg : dY + n0 + 4 * cg;
    const int64_t ld = op ? ldx : ldy;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    float csum[4] = {0.f, 0.f, 0.f, 0.f};

    f32x4 v[8];
    auto load = [&](int64_t r0) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int64_t row = r0 + 8 * rg + q;
            v[q] = row < r_end ? ld4(src + row * ld) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    if (r_begin < r_end) load(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += WG_R) {
        __syncthreads();  // the previous chunk's fragment reads are done
        if (do_col && op == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float t = 0.f;
#pragma unroll
                for (int q = 0; q < 8; ++q) t += v[q][j];
                csum[j] += t;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            V p[NP];
            split8<SP>(f32x4{v[0][j], v[1][j], v[2][j], v[3][j]}, f32x4{v[4][j], v[5][j], v[6][j], v[7][j]}, p);
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) sm[((op * NP + pl) * WS_G + rg) * WG_T + j * 32 + cg] = p[pl];
        }
        __syncthreads();
        if (r0 + WG_R < r_end) load(r0 + WG_R);
#pragma unroll
        for (int s = 0; s < WG_R / 16; ++s) {
            V fa[2][NP], fb[2][NP];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int pl = 0; pl < NP; ++pl) {
                    fa[t][pl] = sm[(pl * WS_G + 2 * s + half) * WG_T + wn * 64 + t * 32 + i];
                    fb[t][pl] = sm[((NP + pl) * WS_G + 2 * s + half) * WG_T + wk * 64 + t * 32 + i];
                }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) SP::template products<false>(acc[a][b], fa[a], fb[b], acc[a][b]);
        }
    }
    // acc[a][b][e] = dW[n0 + 4 mfma32_row(e, half) + 2 wn + a][k0 + 4 i + 2 wk + b]  (position p <-> column 4 (p & 31) + (p >> 5))
    float* out = part + (int64_t)blockIdx.y * N * K;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float* o = out + (int64_t)(n0 + 4 * mfma32_row(e, half) + 2 * wn + a) * K + k0 + 4 * i + 2 * wk;
            o[0] = acc[a][0][e];
            o[1] = acc[a][1][e];
        }
    if (do_col) {  // block uniform
        if (op == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) scol[rg * WG_T + 4 * cg + j] = csum[j];
        }
        __syncthreads();
        if (tid < WG_T) {
            float t = 0.f;
#pragma unroll
            for (int g = 0; g < WS_G; ++g) t += scol[g * WG_T + tid];
            colpart[(int64_t)blockIdx.y * N + n0 + tid] = t;
        }
    }
}

// THE row slices of a weight gradient and where their partial sums go: part [slices][N][K], then colpart [slices][N].  From a
// null base it only measures.
struct WgradWs {
    int64_t per, slices, bytes;
    float *part, *colpart;
};
WgradWs wgrad_carve(void* base, int64_t rows, int32_t N, int32_t K) {
    WgradWs w;
    w.per = wgrad_slice_rows(rows, N, K);
    w.slices = rows > 0 ? (rows + w.per - 1) / w.per : 0;
    Carver cv{base};
    w.part = cv.take<float>(w.slices * N * K);
    w.colpart = cv.take<float>(w.slices * N);
    w.bytes = cv.used;
    return w;
}

// dW (+)= dY^T X with the row slices' partial products from Partial (the fp32-input, the split-operand or the bf16 kernel)
template <auto Partial>
int wgrad_run(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N, int32_t K, float* dW,
              int32_t accumulate, float* colsum, void* workspace, int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(dY && X && dW, SCREAM_EINVAL);
    SCREAM_REQUIRE(rows >= 0 && N > 0 && K > 0 && N % WG_T == 0 && K % WG_T == 0, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(ldy >= N && ldx >= K && ldy % 4 == 0 && ldx % 4 == 0 && aligned16(dY) && aligned16(X), SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    if (rows == 0) {  // an empty sum: dW (+)= 0
        if (!accumulate) {
            if (hipMemsetAsync(dW, 0, (size_t)N * K * sizeof(float), st) != hipSuccess) return SCREAM_EINVAL;
            if (colsum && hipMemsetAsync(colsum, 0, (size_t)N * sizeof(float), st) != hipSuccess) return SCREAM_EINVAL;
        }
        return 0;
    }
    const WgradWs w = wgrad_carve(workspace, rows, N, K);
    SCREAM_REQUIRE(workspace && workspace_bytes >= w.bytes && aligned16(workspace), SCREAM_EINVAL);
    SCREAM_REQUIRE(w.slices <= 65535, SCREAM_EUNSUPPORTED);
    float* colpart = colsum ? w.colpart : nullptr;
    const int tiles = (N / WG_T) * (K / WG_T);
    Partial<<<dim3(tiles, (unsigned)w.slices), dim3(256), 0, st>>>(dY, ldy, X, ldx, rows, N, K, w.per, w.part, colpart);
    SCREAM_LAUNCH_CHECK();
    const int64_t nk = (int64_t)N * K;
    wgrad_reduce_kernel<<<dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st>>>(w.part, (int)w.slices, nk, dW, accumulate, colpart,
                                                                                 N, colsum);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

}  // namespace
