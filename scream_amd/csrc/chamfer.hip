// The Chamfer distance of packed cloud pairs and its gradient (evaluate_open_gf.py:25-41 of the reference: square_distance, two
// min, two means), brute force, without the N x M matrix.  include/scream_hip.h states the contract operation by operation;
// tests/chamfer_ref.py restates it in numpy.
//
// Forward.  The distance is the DIFFERENCE form, every fp32 operation rounded once (-ffp-contract=off, explicit intrinsics):
//   d(n,m) = ((dx*dx + dy*dy) + dz*dz),  dx = a_n.x - b_m.x, ...
// (a - b)^2 and (b - a)^2 are the same bits, so ONE scan kernel serves both directions: the first half of grid x scans b for the
// rows of a, the second half a for the rows of b.  Its shape is nn_search.hip's: a block stages 1024 targets in LDS as float4,
// every lane reads them by wave-uniform broadcast, a thread carries QPT queries, the scan keeps the minimum of each chunk of NC
// targets and rescans the chunk that lowered a query's best for the FIRST target attaining it (strict <: the lowest index wins),
// and a long target cloud is split over blocks that merge 64-bit (distance, index) keys with an INTEGER atomicMin (the minimum
// of a set does not depend on the order it is taken in).  No float atomics.
// The sums are float64 of the widened minima: a 256-row chunk s = v[0]; s += v[1]; ... by one thread, then the chunks of a
// cloud in ascending order (the chunk and cloud sums of prep.hip), so a pair's value depends on that pair alone.
//
// Backward.  da[n] = (a_n - b_j) w_ab + acc w_ba,  acc = sum over the m with idx_ba[m] == n of (a_n - b_m) IN ASCENDING m.
// The second term is a scatter; it is computed as a re-scan, without atomics, a sort or scratch: the wave that owns 64 rows of
// a reads idx_ba of its pair 64 entries at a time (lane l the entry m0 + l, staged through LDS together with b's coordinates),
// a ballot marks the entries that name one of the wave's rows, and the marked entries are handed to their owners one after the
// other from the lowest bit upwards -- ascending m by construction.  A miss costs a compare and a ballot per 64 entries.
// Non-finite input is outside the contract; every index read back is clamped into its cloud before it addresses anything.
#include <stdint.h>

#include "common.h"

namespace {

constexpr int QPT = 4;          // queries per thread
constexpr int QB = 256 * QPT;   // queries per block
constexpr int RT = 1024;        // targets per LDS tile
constexpr int NC = 32;          // targets per chunk of the scan
constexpr int CHUNK = 256;      // rows per chunk sum
constexpr int MAX_SPLITS = 64;

inline int32_t n_chunks(int32_t max_len) { return (int32_t)(((int64_t)max_len + CHUNK - 1) / CHUNK); }
__device__ __forceinline__ int chunks_of(int n) { return (n + CHUNK - 1) / CHUNK; }

__device__ __forceinline__ uint32_t f32_orderable(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_orderable(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct Clouds {
    const float* a;
    const int32_t* a_row0;
    const int32_t* a_len;
    int64_t a_rows;
    int32_t max_a_len;
    const float* b;
    const int32_t* b_row0;
    const int32_t* b_len;
    int64_t b_rows;
    int32_t max_b_len;
    int32_t n_pairs;
};

// one side of pair p as the queries (q) and the other as the targets (t); dir 0: q = a, 1: q = b
struct Side {
    const float* q;
    const float* t;
    int64_t q0, t0;
    int nq, nt;
};
// a pair whose rows leave the arrays (or exceed the declared maxima) has no rows on either side: it reads and writes nothing
__device__ __forceinline__ Side side_of(const Clouds& C, int p, int dir) {
    const int64_t a0 = C.a_row0[p], b0 = C.b_row0[p];
    int na = C.a_len[p], nb = C.b_len[p];
    const bool ok = a0 >= 0 && na >= 0 && na <= C.max_a_len && a0 + na <= C.a_rows && b0 >= 0 && nb >= 0 && nb <= C.max_b_len &&
                    b0 + nb <= C.b_rows;
    if (!ok) na = nb = 0;
    Side s;
    if (dir == 0)
        s.q = C.a, s.t = C.b, s.q0 = a0, s.t0 = b0, s.nq = na, s.nt = nb;
    else
        s.q = C.b, s.t = C.a, s.q0 = b0, s.t0 = a0, s.nq = nb, s.nt = na;
    return s;
}

// every packed row of both sides: no key yet, idx -1, d 0 (what rows outside any cloud and rows without a target keep)
__global__ __launch_bounds__(256) void chamfer_init_kernel(uint64_t* __restrict__ keys_a, int32_t* __restrict__ idx_ab, float* __restrict__ d_ab,
                                                          int64_t a_rows, unsigned a_blocks, uint64_t* __restrict__ keys_b,
                                                          int32_t* __restrict__ idx_ba, float* __restrict__ d_ba, int64_t b_rows) {
    const bool second = blockIdx.x >= a_blocks;
    const int64_t i = (int64_t)(blockIdx.x - (second ? a_blocks : 0)) * 256 + threadIdx.x;
    if (i >= (second ? b_rows : a_rows)) return;
    (second ? keys_b : keys_a)[i] = ~0ull;
    (second ? idx_ba : idx_ab)[i] = -1;
    (second ? d_ba : d_ab)[i] = 0.0f;
}

// grid (2 qblocks, splits, n_pairs), qblocks = ceil(max(max_a_len, max_b_len) / QB): the first qblocks of x are direction 0
__global__ __launch_bounds__(256) void chamfer_scan_kernel(Clouds C, int qblocks, int t_per_split, uint64_t* __restrict__ keys_a,
                                                          uint64_t* __restrict__ keys_b) {
    __shared__ __attribute__((aligned(16))) float tile[RT * 4];
    const int dir = blockIdx.x >= (unsigned)qblocks ? 1 : 0, p = blockIdx.z;
    const Side S = side_of(C, p, dir);
    const int nq = S.nq, nt = S.nt;
    const int qb0 = (blockIdx.x - dir * qblocks) * QB;
    const int j_begin = blockIdx.y * t_per_split;
    const int j_end = min(nt, j_begin + t_per_split);
    if (qb0 >= nq || j_begin >= j_end) return;  // block-uniform
    const int tid = threadIdx.x;
    const float* tp = S.t + S.t0 * 3;

    const bool wave_has_queries = qb0 + (tid & ~63) < nq;  // wave-uniform
    float ax[QPT], ay[QPT], az[QPT], best[QPT];
    int bi[QPT];
#pragma unroll
    for (int u = 0; u < QPT; ++u) {
        const int qi = qb0 + tid + 256 * u;
        const int64_t row = S.q0 + min(qi, nq - 1);  // clamp: out-of-range slots recompute the last point, never stored
        ax[u] = S.q[row * 3 + 0];
        ay[u] = S.q[row * 3 + 1];
        az[u] = S.q[row * 3 + 2];
        best[u] = __builtin_inff();
        bi[u] = 0x7fffffff;
    }
    // (a distance is never -0: a square is >= +0 and +0 + +0 = +0, so == finds exactly the bits fminf kept)
    auto dist = [&](int u, const f32x4& b) __attribute__((always_inline)) {
        const float dx = __fsub_rn(ax[u], b[0]), dy = __fsub_rn(ay[u], b[1]), dz = __fsub_rn(az[u], b[2]);
        return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    };
    for (int jt = j_begin; jt < j_end; jt += RT) {
        const int cnt = min(RT, j_end - jt);
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) {
            const float* r = tp + (int64_t)(jt + i) * 3;
            f32x4 v = {r[0], r[1], r[2], 0.0f};
            *reinterpret_cast<f32x4*>(tile + i * 4) = v;
        }
        __syncthreads();
        if (!wave_has_queries) continue;
        int won[QPT];  // first target (tile-relative) of the chunk that lowered this query's best in this tile, or -1
#pragma unroll
        for (int u = 0; u < QPT; ++u) won[u] = -1;
        for (int c = 0; c < cnt; c += NC) {
            const int ce = min(NC, cnt - c);
            float cm[QPT];
#pragma unroll
            for (int u = 0; u < QPT; ++u) cm[u] = __builtin_inff();
            if (ce == NC) {
#pragma unroll 8
                for (int j = 0; j < NC; ++j) {
                    const f32x4 b = *reinterpret_cast<const f32x4*>(tile + (c + j) * 4);  // wave-uniform address: broadcast
#pragma unroll
                    for (int u = 0; u < QPT; ++u) cm[u] = fminf(cm[u], dist(u, b));
                }
            } else {
                for (int j = 0; j < ce; ++j) {
                    const f32x4 b = *reinterpret_cast<const f32x4*>(tile + (c + j) * 4);
#pragma unroll
                    for (int u = 0; u < QPT; ++u) cm[u] = fminf(cm[u], dist(u, b));
                }
            }
#pragma unroll
            for (int u = 0; u < QPT; ++u) {
                if (cm[u] < best[u]) {
                    best[u] = cm[u];
                    won[u] = c;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
            if (won[u] >= 0) {  // (per lane: the rescan reads the lane's own chunk)
                const int ce = min(NC, cnt - won[u]);
                int first = ce - 1;  // (finite input always finds its minimum again; anything else stays inside the chunk)
                for (int j = ce - 1; j >= 0; --j) {
                    const f32x4 b = *reinterpret_cast<const f32x4*>(tile + (won[u] + j) * 4);
                    if (dist(u, b) == best[u]) first = j;
                }
                bi[u] = jt + won[u] + first;
            }
        }
    }
    uint64_t* keys = (dir == 0 ? keys_a : keys_b) + S.q0;
#pragma unroll
    for (int u = 0; u < QPT; ++u) {
        const int qi = qb0 + tid + 256 * u;
        if (qi < nq && bi[u] != 0x7fffffff) {
            const uint64_t key = ((uint64_t)f32_orderable(best[u]) << 32) | (uint32_t)bi[u];
            atomicMin(reinterpret_cast<unsigned long long*>(keys + qi), (unsigned long long)key);
        }
    }
}

// grid (2 nc, n_pairs), nc = max(nca, ncb), the first nc of x direction 0: idx and d of the rows of a cloud from their keys, and the chunk sum of the widened minima
__global__ __launch_bounds__(CHUNK) void chamfer_finalize_kernel(Clouds C, const uint64_t* __restrict__ keys_a, const uint64_t* __restrict__ keys_b,
                                                                int32_t* __restrict__ idx_ab, float* __restrict__ d_ab,
                                                                int32_t* __restrict__ idx_ba, float* __restrict__ d_ba,
                                                                double* __restrict__ part, int nca, int ncb, int nc) {
    __shared__ double sh[CHUNK];
    const int dir = blockIdx.x >= (unsigned)nc ? 1 : 0, p = blockIdx.y, chunk = blockIdx.x - dir * nc, t = threadIdx.x;
    const Side S = side_of(C, p, dir);
    const int i = chunk * CHUNK + t, cnt = min(CHUNK, S.nq - chunk * CHUNK);
    if (cnt <= 0) return;
    float d = 0.0f;
    if (i < S.nq) {
        const uint64_t key = (dir == 0 ? keys_a : keys_b)[S.q0 + i];
        int32_t idx = -1;
        if (key != ~0ull) {  // (an empty target cloud leaves no key)
            d = f32_from_orderable((uint32_t)(key >> 32));
            idx = min((int32_t)((uint32_t)key & 0x7fffffffu), S.nt - 1);
        }
        (dir == 0 ? idx_ab : idx_ba)[S.q0 + i] = idx;
        (dir == 0 ? d_ab : d_ba)[S.q0 + i] = d;
    }
    sh[t] = (double)d;
    __syncthreads();
    if (t == 0) {
        double s = sh[0];
        for (int j = 1; j < cnt; ++j) s += sh[j];
        (dir == 0 ? part + (int64_t)p * nca : part + (int64_t)C.n_pairs * nca + (int64_t)p * ncb)[chunk] = s;
    }
}

__device__ __forceinline__ double cloud_sum(const double* part, int nc) {
    double acc = part[0];
    for (int j = 1; j < nc; ++j) acc += part[j];
    return acc;
}

// one block: loss_pair[p] = S_ab / N + S_ba / M (0 for an empty side);  loss = fp32((loss_pair[0] + loss_pair[1] + ...) / n_pairs)
__global__ __launch_bounds__(CHUNK) void chamfer_final_kernel(Clouds C, const double* __restrict__ part, int nca, int ncb,
                                                             double* __restrict__ loss_pair, float* __restrict__ loss) {
    for (int p = threadIdx.x; p < C.n_pairs; p += CHUNK) {
        const Side S = side_of(C, p, 0);
        double v = 0.0;
        if (S.nq > 0 && S.nt > 0) {
            const double s_ab = cloud_sum(part + (int64_t)p * nca, chunks_of(S.nq));
            const double s_ba = cloud_sum(part + (int64_t)C.n_pairs * nca + (int64_t)p * ncb, chunks_of(S.nt));
            v = s_ab / (double)S.nq + s_ba / (double)S.nt;
        }
        loss_pair[p] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = loss_pair[0];
        for (int p = 1; p < C.n_pairs; ++p) acc += loss_pair[p];
        loss[0] = (float)(acc / (double)C.n_pairs);
    }
}

__global__ __launch_bounds__(256) void chamfer_zero_kernel(float* __restrict__ da, int64_t na, unsigned a_blocks, float* __restrict__ db, int64_t nb) {
    const bool second = blockIdx.x >= a_blocks;
    const int64_t i = (int64_t)(blockIdx.x - (second ? a_blocks : 0)) * 256 + threadIdx.x;
    if (i < (second ? nb : na)) (second ? db : da)[i] = 0.0f;
}

// grid (n_dirs qblocks, n_pairs), qblocks = ceil(max len / 256), dir0 the first direction launched: the gradient rows of one side,
// one row per thread
__global__ __launch_bounds__(256) void chamfer_bwd_kernel(Clouds C, const float* __restrict__ dout, const int32_t* __restrict__ idx_ab,
                                                         const int32_t* __restrict__ idx_ba, float* __restrict__ da, float* __restrict__ db,
                                                         int qblocks, int dir0) {
    __shared__ __attribute__((aligned(16))) float tile[RT * 4];  // {x, y, z, bits of idx} of 1024 rows of the OTHER side
    const int second = blockIdx.x >= (unsigned)qblocks ? 1 : 0, dir = dir0 + second, p = blockIdx.y;
    const Side S = side_of(C, p, dir);
    const int nq = S.nq, nt = S.nt;
    const int qb0 = (blockIdx.x - second * qblocks) * 256;
    if (qb0 >= nq || nt <= 0) return;  // block-uniform (the rows of an empty pair keep their zeros)
    const int tid = threadIdx.x, lane = tid & 63, w0 = qb0 + (tid & ~63);  // w0: the first row of this wave
    const bool wave_has_rows = w0 < nq;
    const int qi = qb0 + tid;
    const int64_t qrow = S.q0 + min(qi, nq - 1);
    const double A[3] = {(double)S.q[qrow * 3 + 0], (double)S.q[qrow * 3 + 1], (double)S.q[qrow * 3 + 2]};
    const float* tp = S.t + S.t0 * 3;
    const int32_t* idx_t = (dir == 0 ? idx_ba : idx_ab) + S.t0;  // the other side's nearest rows of THIS side
    double acc[3] = {0.0, 0.0, 0.0};
    for (int jt = 0; jt < nt; jt += RT) {
        const int cnt = min(RT, nt - jt);
        __syncthreads();
        for (int i = tid; i < cnt; i += 256) {
            const float* r = tp + (int64_t)(jt + i) * 3;
            f32x4 v = {r[0], r[1], r[2], __int_as_float(idx_t[jt + i])};
            *reinterpret_cast<f32x4*>(tile + i * 4) = v;
        }
        __syncthreads();
        if (!wave_has_rows) continue;
        for (int m0 = 0; m0 < cnt; m0 += 64) {
            const int rel = m0 + lane < cnt ? __float_as_int(tile[(m0 + lane) * 4 + 3]) - w0 : -1;
            unsigned long long hits = __ballot((unsigned)rel < 64u);
            while (hits) {  // wave-uniform; lowest bit first: ascending m
                const int bit = __ffsll(hits) - 1;
                hits &= hits - 1;
                const int owner = __shfl(rel, bit);
                if (lane == owner) {
                    const float* bm = tile + (m0 + bit) * 4;
#pragma unroll
                    for (int k = 0; k < 3; ++k) acc[k] = acc[k] + (A[k] - (double)bm[k]);
                }
            }
        }
    }
    if (qi >= nq) return;
    const double g = (double)dout[0] / (double)C.n_pairs;
    const double w_q = (2.0 * g) / (double)nq, w_t = (2.0 * g) / (double)nt;
    const int j = (dir == 0 ? idx_ab : idx_ba)[qrow];
    const float* bj = tp + (int64_t)min(max(j, 0), nt - 1) * 3;
    float* o = (dir == 0 ? da : db) + qrow * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double near = j >= 0 ? (A[k] - (double)bj[k]) * w_q : 0.0;  // (j < 0: non-finite input found no neighbour)
        o[k] = (float)(near + acc[k] * w_t);
    }
}

inline bool clouds_ok(const Clouds& C) {
    return C.a && C.a_row0 && C.a_len && C.b && C.b_row0 && C.b_len && C.n_pairs > 0 && rows_ok(C.a_rows, C.max_a_len) &&
           rows_ok(C.b_rows, C.max_b_len);
}

}  // namespace

extern "C" int scream_chamfer_fwd(const float* a, const int32_t* a_row0, const int32_t* a_len, int64_t a_rows, int32_t max_a_len,
                                  const float* b, const int32_t* b_row0, const int32_t* b_len, int64_t b_rows, int32_t max_b_len,
                                  int32_t n_pairs, uint64_t* keys_a, uint64_t* keys_b, double* part, int32_t* idx_ab, float* d_ab,
                                  int32_t* idx_ba, float* d_ba, double* loss_pair, float* loss, void* stream) {
    const Clouds C = {a, a_row0, a_len, a_rows, max_a_len, b, b_row0, b_len, b_rows, max_b_len, n_pairs};
    SCREAM_REQUIRE(clouds_ok(C), SCREAM_EINVAL);
    SCREAM_REQUIRE(keys_a && keys_b && part && idx_ab && d_ab && idx_ba && d_ba && loss_pair && loss, SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned8(keys_a) && aligned8(keys_b) && aligned8(part) && aligned8(loss_pair), SCREAM_EINVAL);
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    hipStream_t st = as_stream(stream);
    const unsigned ablk = (unsigned)((a_rows + 255) / 256), bblk = (unsigned)((b_rows + 255) / 256);
    if (ablk + bblk > 0) {
        chamfer_init_kernel<<<dim3(ablk + bblk), dim3(256), 0, st>>>(keys_a, idx_ab, d_ab, a_rows, ablk, keys_b, idx_ba, d_ba, b_rows);
        SCREAM_LAUNCH_CHECK();
    }
    const int32_t max_len = max_a_len > max_b_len ? max_a_len : max_b_len;
    const int nca = n_chunks(max_a_len), ncb = n_chunks(max_b_len), nc = nca > ncb ? nca : ncb;
    if (max_a_len > 0 && max_b_len > 0) {
        // split the target range so that the launch is a whole number of rounds of equal blocks on the 256 CUs when it can be: the
        // split count in [1, 64] that minimises rounds x targets per split (nn_search.hip); results do not depend on it
        const int qblocks = (max_len + QB - 1) / QB;
        const int max_splits = (max_len + 255) / 256 < MAX_SPLITS ? (max_len + 255) / 256 : MAX_SPLITS;
        int splits = 1;
        int64_t best_cost = INT64_MAX;
        for (int sp = 1; sp <= max_splits; ++sp) {
            const int64_t blocks = (int64_t)qblocks * sp * 2 * n_pairs, per = (max_len + sp - 1) / sp;
            const int64_t cost = ((blocks + 255) / 256) * (per + 64);  // (+ 64: a block's fixed cost in units of targets)
            if (cost < best_cost) {
                best_cost = cost;
                splits = sp;
            }
        }
        const int t_per_split = (max_len + splits - 1) / splits;
        splits = (max_len + t_per_split - 1) / t_per_split;
        chamfer_scan_kernel<<<dim3(2 * qblocks, splits, n_pairs), dim3(256), 0, st>>>(C, qblocks, t_per_split, keys_a, keys_b);
        SCREAM_LAUNCH_CHECK();
    }
    if (nc > 0) {
        chamfer_finalize_kernel<<<dim3(2 * nc, n_pairs), dim3(CHUNK), 0, st>>>(C, keys_a, keys_b, idx_ab, d_ab, idx_ba, d_ba, part, nca, ncb, nc);
        SCREAM_LAUNCH_CHECK();
    }
    chamfer_final_kernel<<<dim3(1), dim3(CHUNK), 0, st>>>(C, part, nca, ncb, loss_pair, loss);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_chamfer_bwd(const float* dout, const float* a, const int32_t* a_row0, const int32_t* a_len, int64_t a_rows,
                                  int32_t max_a_len, const float* b, const int32_t* b_row0, const int32_t* b_len, int64_t b_rows,
                                  int32_t max_b_len, int32_t n_pairs, const int32_t* idx_ab, const int32_t* idx_ba, float* da, float* db,
                                  void* stream) {
    const Clouds C = {a, a_row0, a_len, a_rows, max_a_len, b, b_row0, b_len, b_rows, max_b_len, n_pairs};
    SCREAM_REQUIRE(clouds_ok(C), SCREAM_EINVAL);
    SCREAM_REQUIRE(dout && idx_ab && idx_ba, SCREAM_EINVAL);
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    if (!da && !db) return 0;
    hipStream_t st = as_stream(stream);
    const int64_t na = da ? a_rows * 3 : 0, nb = db ? b_rows * 3 : 0;
    const unsigned ablk = (unsigned)((na + 255) / 256), bblk = (unsigned)((nb + 255) / 256);
    if (ablk + bblk > 0) {
        chamfer_zero_kernel<<<dim3(ablk + bblk), dim3(256), 0, st>>>(da, na, ablk, db, nb);
        SCREAM_LAUNCH_CHECK();
    }
    const int32_t max_len = da && db ? (max_a_len > max_b_len ? max_a_len : max_b_len) : (da ? max_a_len : max_b_len);
    if (max_len > 0 && max_a_len > 0 && max_b_len > 0) {
        const int qblocks = (int)row_blocks(max_len);
        chamfer_bwd_kernel<<<dim3((da && db ? 2 : 1) * qblocks, n_pairs), dim3(256), 0, st>>>(C, dout, idx_ab, idx_ba, da, db, qblocks,
                                                                                            da ? 0 : 1);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}
