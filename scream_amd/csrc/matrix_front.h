// The host front end that the GEMM-like entry points share (gemm_f32.hip, gemm_split.hip, proj_ring.hip): argument checks, the
// way from the runtime epilogue to its instantiation, the persistent grid (the layer tail's too).  Host only; the split predicates,
// with_split and the exponent ranges are in split.h.  An extern "C" body reads: shared checks, what is peculiar to it, launch.
// The ORDER of the checks is part of the contract: it decides which of SCREAM_EINVAL / SCREAM_EUNSUPPORTED a call that breaks
// two rules gets (tests/test_matrix_front_host.py holds the table).
#pragma once
#include <type_traits>

#include "common.h"

namespace {

constexpr int FRONT_BN = 256;  // output columns of a block tile, in every one of these kernels

// the contraction length: a multiple of 64 for the fp32 kernel; the split kernel's k-loop wants K = 64 + 192 j -- an EVEN number of
// 32-deep k-tiles (stage = kt & 1), in groups of three after the first two
enum KRule { K_MULT_64, K_64_PLUS_192 };
static inline bool mnk_ok(int64_t M, int32_t N, int32_t K, KRule rule) {
    return M >= 0 && M % SCREAM_ROW_TILE == 0 && N > 0 && N % FRONT_BN == 0 && K > 0 && K % 64 == 0 &&
           (rule == K_MULT_64 || (K / 32 - 2) % 3 == 0);
}

// C[M,N] = epilogue(A[M,K] . W[N,K]^T)
static inline int check_gemm(const void* A, int64_t lda, const void* W, const void* C, int64_t ldc, int64_t M, int32_t N, int32_t K,
                             KRule rule) {
    SCREAM_REQUIRE(A && W && C, SCREAM_EINVAL);
    SCREAM_REQUIRE(mnk_ok(M, N, K, rule), SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(lda >= K && ldc >= N && lda % 4 == 0 && ldc % 4 == 0 && aligned16(A) && aligned16(W) && aligned16(C), SCREAM_EINVAL);
    return 0;
}

// launch(Epi<SCREAM_EPI_*>{}) behind what that epilogue asks of its arguments (ep: an EpiArgs)
template <int E> using Epi = std::integral_constant<int, E>;
template <class EP, class F>
int dispatch_epilogue(int32_t epilogue, int32_t N, const EP& ep, F&& launch) {
    switch (epilogue) {
        case SCREAM_EPI_NONE: return launch(Epi<SCREAM_EPI_NONE>{});
        case SCREAM_EPI_ELU1:
            SCREAM_REQUIRE(ep.n_act >= 0 && ep.n_act % FRONT_BN == 0, SCREAM_EUNSUPPORTED);
            return launch(Epi<SCREAM_EPI_ELU1>{});
        case SCREAM_EPI_RELU: return launch(Epi<SCREAM_EPI_RELU>{});
        case SCREAM_EPI_BIAS_RELU:
            SCREAM_REQUIRE(ep.bias, SCREAM_EINVAL);
            return launch(Epi<SCREAM_EPI_BIAS_RELU>{});
        case SCREAM_EPI_RES_LN:
            SCREAM_REQUIRE(N == FRONT_BN, SCREAM_EUNSUPPORTED);
            SCREAM_REQUIRE(ep.residual && ep.gamma && ep.beta && ep.ldr >= N && ep.ldr % 4 == 0 && aligned16(ep.residual), SCREAM_EINVAL);
            return launch(Epi<SCREAM_EPI_RES_LN>{});
        default: return SCREAM_EINVAL;
    }
}

// The fused q/k/v projection: N = n_q + 512 L, n_q query columns (0 or 256) in front of L key/value tile pairs.  multi_kv: L > 1
// (several layers' key/value projections of the same rows) is allowed, and then only without queries.
static inline int check_qkv(const void* A, int64_t lda, const void* W, const void* Q, int64_t ldq, int64_t M, int32_t N, int32_t K,
                            int32_t n_q, const int32_t* tile_cloud, const int32_t* cloud_row0, const int32_t* cloud_len,
                            int64_t row_base, const void* kv_partial, KRule rule, bool multi_kv) {
    SCREAM_REQUIRE(A && W && kv_partial && tile_cloud && cloud_row0 && cloud_len, SCREAM_EINVAL);
    SCREAM_REQUIRE(mnk_ok(M, N, K, rule), SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE((n_q == 0 || n_q == FRONT_BN) && N > n_q && (N - n_q) % (2 * FRONT_BN) == 0 &&
                       ((multi_kv && n_q == 0) || N == n_q + 2 * FRONT_BN) && row_base >= 0 && row_base % SCREAM_ROW_TILE == 0,
                   SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(n_q == 0 || (Q && ldq >= n_q && ldq % 4 == 0 && aligned16(Q)), SCREAM_EINVAL);
    SCREAM_REQUIRE(lda >= K && lda % 4 == 0 && aligned16(A) && aligned16(W), SCREAM_EINVAL);
    return 0;
}

// Blocks of a persistent grid over `total` work items, one per item up to max_grid; 0: nothing to launch, and the caller returns 0.
// Negative: a kernel that numbers its items in 32 bits (index32) refuses 2^31 of them and more, and the caller returns that.
static inline int persistent_grid(int64_t total, int max_grid, bool index32 = true) {
    if (index32 && total >= (1ll << 31)) return SCREAM_EUNSUPPORTED;
    return (int)(total < max_grid ? total : max_grid);
}

}  // namespace
