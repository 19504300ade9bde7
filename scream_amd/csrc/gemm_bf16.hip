// The matrix products of train_backend "bf16": ONE bf16 product per GEMM, fp32 accumulation (include/scream_hip.h states the
// arithmetic).  Operands are fp32 in memory and rounded to bf16 (round to nearest even, v_cvt_pk_bf16_f32) in registers on
// their way into the kernel; nothing is packed or transposed by another launch.
//
//   forward        C[M,N]  = epilogue(A[M,K] . W[N,K]^T)      scream_gemm_bf16_f32
//   data gradient  dX[M,K] = dY[M,N] . W[N,K]                 scream_gemm_dgrad_bf16_f32  (sums over N in one launch)
//   weight grad.   dW[N,K] (+)= dY[rows,N]^T X[rows,K]        scream_gemm_wgrad_bf16_f32  (wgrad.h's kernel with one plane)
//
// Forward and data gradient are one kernel, out[M,NO] = epi(act[M,KC] . B[KC,NO]) with B[k][n] = W[n][k] (forward) or W[k][n]
// (data gradient).  Geometry of gemm_f32.hip, so that its epilogues (gemm_epilogue.h) serve unchanged: block tile 128 x 256,
// four waves stacked in M, wave tile 32 x 256 = 8 accumulator tiles of v_mfma_f32_32x32x16_bf16; k-tiles of 32 = two 16-deep
// steps.  Inside a k-tile lane (r, half) owns k = 16 half + 8 s + j (step s, element j) for both operands: any permutation of
// the contraction index shared by both is legal.
//   * activations never touch LDS: lane (r, half) loads its 64 contiguous bytes of row r per k-tile into registers, one tile
//     ahead, and converts eight values per step;
//   * the weight tile goes through registers (one tile ahead), is converted, and is written to LDS as the image
//     [k-group of eight g][column n] of 16-byte vectors (eight bf16 = one lane's B fragment of one step).  The forward's thread
//     holds eight consecutive k of one row of W (two 16-byte loads); the data gradient's thread holds eight ROWS of W at four
//     columns (eight 16-byte loads, every wave instruction one contiguous KiB) and writes each column's eight values as one
//     vector: the transpose happens in that write, never in a launch of its own;
//   * column n sits at position n ^ ((n >> 3) & 3) and a k-group is 258 positions long: the forward's write (eight lanes =
//     two columns x four groups), the data gradient's write (eight lanes = columns 4 apart) and the fragment read (32 lanes =
//     32 consecutive columns) all touch every 16-byte bank slot once;
//   * two LDS buffers, one barrier per k-tile; the epilogue's slabs reuse them.
// Reductions: every output element is one k-ordered fp32 chain in one wave: no atomics, bitwise repeatable.
#include "gemm_epilogue.h"
#include "matrix_front.h"
#include "wgrad.h"

namespace {

// the one-plane operand policy: x -> bf16(x), one product per 16-deep step (the interface of split.h's policies)
struct Bf16One {
    static constexpr int NP = 1;
    typedef bf16x8 vec;
    static __device__ __forceinline__ void split1(float x, int i, vec (&p)[1]) { p[0][i] = (__bf16)x; }
    static __device__ __forceinline__ f32x16 mfma(vec a, vec b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    template <bool MIRROR = false>
    static __device__ __forceinline__ void products(f32x16& acc, const vec (&x)[1], const vec (&y)[1], const f32x16& c0) {
        acc = mfma(x[0], y[0], c0);
    }
};

__device__ __forceinline__ bf16x8 to_bf16x8(const f32x4 lo, const f32x4 hi) {
    bf16x8 p[1];
    split8<Bf16One>(lo, hi, p);
    return p[0];
}

constexpr int BM = 128;
constexpr int BN = 256;
constexpr int BK = 32;
constexpr int THREADS = 256;
constexpr int KG = BK / 8;        // k-groups of eight per k-tile
constexpr int KG_LD = BN + 2;     // positions per k-group: two slots of skew between the groups
constexpr int WTILE = KG * KG_LD; // vectors per buffer
constexpr int SMEM_FLOATS = 2 * WTILE * 4 > 4 * 8 * 256 ? 2 * WTILE * 4 : 4 * 8 * 256;  // two buffers | the epilogue's slabs

__device__ __forceinline__ int wpos(int n) { return n ^ ((n >> 3) & 3); }

// W_ROWS_ARE_K false: W [NO, KC] (the forward), true: W [KC, NO] (the data gradient); ldw = its row length
template <int EPI, bool W_ROWS_ARE_K>
__global__ __launch_bounds__(THREADS, 2) void gemm_bf16_kernel(const float* __restrict__ A, int64_t lda,
                                                              const float* __restrict__ W, int64_t ldw,
                                                              float* __restrict__ C, int64_t ldc, int n_tiles, int KC,
                                                              EpiArgs ep) {
    __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
    bf16x8* img = reinterpret_cast<bf16x8*>(smem);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, half = lane >> 5;
    const int64_t m0 = (int64_t)(blockIdx.x / n_tiles) * BM;
    const int n0 = (int)(blockIdx.x % n_tiles) * BN;

    const float* ga = A + (m0 + wave * 32 + r) * lda + half * 16;
    // forward: item tid + 256 u -> row n = item >> 2 of the tile, k-group item & 3;  data gradient: wave = k-group, lane = 4 columns
    const float* gw = W_ROWS_ARE_K ? W + (int64_t)(wave * 8) * ldw + n0 + 4 * lane
                                   : W + (int64_t)(n0 + (tid >> 2)) * ldw + 8 * (tid & 3);
    f32x4 an[4], ac[4], wr[8];
    auto load = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 4; ++j) an[j] = ld4(ga + kt * BK + 4 * j);
        if (W_ROWS_ARE_K) {
#pragma unroll
            for (int q = 0; q < 8; ++q) wr[q] = ld4(gw + (int64_t)(kt * BK + q) * ldw);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                wr[2 * u] = ld4(gw + (int64_t)(64 * u) * ldw + kt * BK);
                wr[2 * u + 1] = ld4(gw + (int64_t)(64 * u) * ldw + kt * BK + 4);
            }
        }
    };
    auto stage = [&](int buf) {
        bf16x8* dst = img + buf * WTILE;
        if (W_ROWS_ARE_K) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                dst[wave * KG_LD + wpos(4 * lane + j)] = to_bf16x8(f32x4{wr[0][j], wr[1][j], wr[2][j], wr[3][j]},
                                                                   f32x4{wr[4][j], wr[5][j], wr[6][j], wr[7][j]});
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) dst[(tid & 3) * KG_LD + wpos(64 * u + (tid >> 2))] = to_bf16x8(wr[2 * u], wr[2 * u + 1]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ac[j] = an[j];
    };

    f32x16 acc[8];
#pragma unroll
    for (int tn = 0; tn < 8; ++tn)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[tn][e] = 0.f;

    const int KT = KC / BK;
    load(0);
    stage(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        if (kt + 1 < KT) load(kt + 1);
        const bf16x8* src = img + (kt & 1) * WTILE;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const bf16x8 fa = to_bf16x8(ac[2 * s], ac[2 * s + 1]);
            const bf16x8* row = src + (2 * half + s) * KG_LD;
#pragma unroll
            for (int tn = 0; tn < 8; ++tn) acc[tn] = Bf16One::mfma(fa, row[wpos(tn * 32 + r)], acc[tn]);
        }
        if (kt + 1 < KT) stage((kt + 1) & 1);  // the buffer that k-tile kt - 1 was read from, a barrier ago
        __syncthreads();
    }
    // the loop ended on a barrier: both buffers are free for the epilogue's slabs
    gemm_epilogue<EPI, 4>(acc, smem, wave, lane, tid, true, m0, n0, ep, C, ldc);
}

template <int EPI, bool W_ROWS_ARE_K>
int launch(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int NO, int KC,
           const EpiArgs& ep, hipStream_t st) {
    const int n_tiles = NO / BN;
    const int grid = persistent_grid((M / BM) * n_tiles, INT32_MAX);  // one block per tile
    if (grid <= 0) return grid;
    gemm_bf16_kernel<EPI, W_ROWS_ARE_K><<<dim3(grid), dim3(THREADS), 0, st>>>(A, lda, W, ldw, C, ldc, n_tiles, KC, ep);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int scream_gemm_bf16_f32(const float* A, int64_t lda, const float* W, float* C, int64_t ldc, int64_t M, int32_t N,
                                    int32_t K, int32_t epilogue, int32_t n_act, const float* bias, void* stream) {
    if (int rc = check_gemm(A, lda, W, C, ldc, M, N, K, K_MULT_64)) return rc;
    SCREAM_REQUIRE(epilogue != SCREAM_EPI_RES_LN, SCREAM_EUNSUPPORTED);  // training runs its LayerNorms as launches of their own
    const EpiArgs ep{n_act, bias, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    return dispatch_epilogue(epilogue, N, ep, [&](auto epi) {
        constexpr int E = decltype(epi)::value;
        if constexpr (E == SCREAM_EPI_RES_LN) return (int)SCREAM_EUNSUPPORTED;
        else return launch<E, false>(A, lda, W, K, C, ldc, M, N, K, ep, as_stream(stream));
    });
}

extern "C" int scream_gemm_dgrad_bf16_f32(const float* dY, int64_t ldy, const float* W, float* dX, int64_t ldx, int64_t M,
                                          int32_t N, int32_t K, void* stream) {
    if (int rc = check_gemm(dY, ldy, W, dX, ldx, M, K, N, K_MULT_64)) return rc;  // K output columns, N summed
    const EpiArgs ep{0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    return launch<SCREAM_EPI_NONE, true>(dY, ldy, W, K, dX, ldx, M, K, N, ep, as_stream(stream));
}

extern "C" int64_t scream_wgrad_bf16_workspace_bytes(int64_t rows, int32_t N, int32_t K) {
    if (rows < 0 || N <= 0 || K <= 0 || N % WG_T || K % WG_T) return -1;
    return wgrad_carve(nullptr, rows, N, K).bytes;
}

extern "C" int scream_gemm_wgrad_bf16_f32(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N,
                                          int32_t K, float* dW, int32_t accumulate, float* colsum, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
    return wgrad_run<wgrad_split_partial_kernel<Bf16One>>(dY, ldy, X, ldx, rows, N, K, dW, accumulate, colsum, workspace,
                                                          workspace_bytes, stream);
}
