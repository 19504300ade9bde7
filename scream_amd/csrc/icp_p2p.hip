// Point-to-point ICP refinement (the "next" row of SURVEY.md 8f: evaluate_3d_match.py:106-119 calls
// open3d.registration_icp, which is not in this image -> parity with open3d itself is UNPINNED; the loop
// below follows open3d's published RegistrationICP: evaluate correspondences of the transformed source
// (nearest target within max_dist), estimate the rigid update from them (Kabsch, no scaling),
// compose, re-evaluate, stop when |d fitness| and |d inlier_rmse| both fall below their thresholds
// or after max_iter updates).  It is exactly loop{ A7 with a radius, A8, A9 } in metric space, so it reuses
// the search (icp_grid.hip, nn_search.hip) and the solve (pose_solve.h); all pairs of a batch iterate together and
// converged pairs freeze on the device (no host synchronisation inside the loop).
// Compiled with -ffp-contract=off, like kabsch.hip: every fp32 step is individually rounded.
#include "common.h"
#include "icp_grid.h"
#include "pose_solve.h"  // solve_pose, block_sum: shared with kabsch.hip

namespace {

// metric frame: x / s + c (evaluate_3d_match.py:106-107)
__global__ __launch_bounds__(256) void icp_to_metric_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ row0,
                                                           const int32_t* __restrict__ len, const float* __restrict__ s,
                                                           const float* __restrict__ c, float* __restrict__ out) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len[p]) return;
    const int64_t row = (int64_t)row0[p] + i;
    out[row * 3 + 0] = xyz[row * 3 + 0] / s[p] + c[p * 3 + 0];
    out[row * 3 + 1] = xyz[row * 3 + 1] / s[p] + c[p * 3 + 1];
    out[row * 3 + 2] = xyz[row * 3 + 2] / s[p] + c[p * 3 + 2];
}

// q = R x + t with the pair's current transform
__global__ __launch_bounds__(256) void icp_transform_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ row0,
                                                           const int32_t* __restrict__ len, const float* __restrict__ T,
                                                           float* __restrict__ out) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len[p]) return;
    const int64_t row = (int64_t)row0[p] + i;
    const float* t = T + p * 16;
    const float x = xyz[row * 3 + 0], y = xyz[row * 3 + 1], z = xyz[row * 3 + 2];
    out[row * 3 + 0] = t[0] * x + t[1] * y + t[2] * z + t[3];
    out[row * 3 + 1] = t[4] * x + t[5] * y + t[6] * z + t[7];
    out[row * 3 + 2] = t[8] * x + t[9] * y + t[10] * z + t[11];
}

__global__ __launch_bounds__(256) void fill_f32_kernel(float* __restrict__ p, float v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- the ICP iteration (round 3, second version): ONE launch per iteration --------------------------------------------------
// A search launch leaves, per 256-point chunk of a pair, a PARTIAL of its correspondences: count, sum |a - b|^2, sum a, sum b, sum a b^T
// (17 doubles; a = the transformed source point, b = its target).  The next launch starts, in EVERY block of the pair, by summing
// the pair's partials in a fixed order and deriving from them what rounds 1-3's separate update launch derived from a second
// gathering pass: fitness / inlier RMSE, the convergence test, and the Kabsch update composed into T -- then searches under the
// new T.  One dependent launch per iteration instead of two (rounds 1-2: three), no gather of idx -> target rows at all.
// The covariance about the fp32 centroids cA, cB (utils.py:155-166) is expanded from the one-pass sums in fp64:
//   sum (a - cA)(b - cB)^T = sum a b^T - cA (sum b)^T - (sum a) cB^T + n cA cB^T
// (the two-pass form rounds the differences to fp32 first: 1e-7 relative apart, both far inside the 1e-4 of the ICP tests; the
// A9 solve of the parity path, kabsch_block of kabsch.hip, is untouched).  Buffers indexed by the parity of the launch are written by the
// pair's block 0 and read by every block of the NEXT launch, so no block ever reads what another block of its own launch writes.
struct IcpState {  // per pair: fitness and inlier RMSE of the last evaluated search
    float fitness, rmse;
};

constexpr int ICP_NP = 17;  // doubles per chunk partial
constexpr int ICP_NG = 15;  // strided groups the partials of a pair are summed in (15 x 17 = 255 threads)

struct IcpArgs {
    const int32_t* src_row0;
    const int32_t* src_len;
    float* Tbuf;         // [2][n_pairs][16]: T of search it lives at parity it & 1
    IcpState* state;     // [2][n_pairs]: evaluation of search e at parity e & 1
    double* part;        // [2][n_chunks_total][ICP_NP]: partials of search it at parity it & 1; chunk c of pair p = chunk0[p] + c
    const int32_t* chunk0;  // [n_pairs] exclusive prefix sum of icp_chunks(src_len[p]) (icp_chunk0_kernel): collision-free for ANY order / overlap of the clouds
    int32_t* done;       // [n_pairs] 0 -> 1, once
    int32_t* act_len;    // [n_pairs] src_len, 0 once done (the brute-force yardstick's kernels take their work from it)
    int64_t part_stride; // n_chunks_total * ICP_NP
    int32_t n_pairs, max_iter;
    float rel_fitness, rel_rmse;
    float* T_out;        // [n_pairs][16] the caller's transforms
    float* fit_rmse_out; // may be NULL
    int32_t* iters_out;  // may be NULL
};

__device__ __forceinline__ int icp_chunks(int n) { return n > 0 ? (n + 255) / 256 : 1; }  // (an empty source still has its block 0)
__device__ __forceinline__ int64_t icp_chunk0(const IcpArgs& a, int p) { return a.chunk0[p]; }

// chunk0[p] = sum_{q < p} icp_chunks(src_len[q]); one thread (n_pairs is a batch size).  Until round 3 the slots were derived from
// src_row0[p] / 256 + p, which is collision-free only for clouds packed in ascending, non-overlapping order -- true for PackedBatch,
// not promised by the C ABI.
__global__ void icp_chunk0_kernel(const int32_t* __restrict__ src_len, int32_t n_pairs, int32_t* __restrict__ chunk0) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int32_t acc = 0;
    for (int p = 0; p < n_pairs; ++p) {
        chunk0[p] = acc;
        acc += icp_chunks(src_len[p]);
    }
}

// Whole block (256 threads).  Evaluates search e = it - 1 of pair p from its partials; returns (block-uniform) whether the pair
// stops.  If it goes on, T_sh (LDS) holds T_it = dT . T_e.  `writer`: this block publishes state / done / outputs / T_it.
__device__ bool icp_pose_step(const IcpArgs& a, int p, int it, bool writer, float* T_sh) {
    __shared__ double grp[ICP_NG][ICP_NP];
    __shared__ double tot[ICP_NP];
    __shared__ float dT_sh[16];
    __shared__ int stop_sh;
    const int e = it - 1, n = a.src_len[p], nb = icp_chunks(n);
    const double* part = a.part + (int64_t)(e & 1) * a.part_stride + icp_chunk0(a, p) * ICP_NP;
    const float* T_e = a.Tbuf + ((int64_t)(e & 1) * a.n_pairs + p) * 16;
    const int tid = threadIdx.x;
    if (tid < ICP_NG * ICP_NP) {
        const int k = tid % ICP_NP, g = tid / ICP_NP;
        double sum = 0.0;
        for (int c = g; c < nb; c += ICP_NG) sum += part[(int64_t)c * ICP_NP + k];
        grp[g][k] = sum;
    }
    __syncthreads();
    if (tid < ICP_NP) {
        double sum = grp[0][tid];
#pragma unroll
        for (int g = 1; g < ICP_NG; ++g) sum += grp[g][tid];
        tot[tid] = sum;
    }
    __syncthreads();
    if (tid < 64) {  // wave 0, every lane redundantly (wave-uniform data)
        const double cnt = tot[0];
        const float fitness = n > 0 ? (float)(cnt / n) : 0.f;
        const float rmse = cnt > 0 ? (float)sqrt(tot[1] / cnt) : 0.f;
        const IcpState prev = a.state[(int64_t)((e + 1) & 1) * a.n_pairs + p];  // evaluation e - 1 (unused at e == 0)
        const bool converged = e > 0 && fabsf(prev.fitness - fitness) < a.rel_fitness && fabsf(prev.rmse - rmse) < a.rel_rmse;
        const bool stop = converged || e >= a.max_iter;
        if (tid == 0) {
            stop_sh = stop ? 1 : 0;
            if (writer) {
                const IcpState o = {fitness, rmse};
                a.state[(int64_t)(e & 1) * a.n_pairs + p] = o;
                if (a.fit_rmse_out) {
                    a.fit_rmse_out[2 * p + 0] = fitness;
                    a.fit_rmse_out[2 * p + 1] = rmse;
                }
                if (a.iters_out) a.iters_out[p] = e;  // number of updates applied
                if (stop) {
                    a.done[p] = 1;
                    a.act_len[p] = 0;
                }
            }
        }
        if (stop) {
            if (writer && tid < 16) a.T_out[p * 16 + tid] = T_e[tid];
        } else {
            const float denom = (float)cnt + 1e-6f;  // utils.py:155-158 with unit weights
            const float cA[3] = {(float)tot[2] / denom, (float)tot[3] / denom, (float)tot[4] / denom};
            const float cB[3] = {(float)tot[5] / denom, (float)tot[6] / denom, (float)tot[7] / denom};
            double H[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double h = tot[8 + r * 3 + c] - (double)cA[r] * tot[5 + c] - tot[2 + r] * (double)cB[c] + cnt * (double)cA[r] * (double)cB[c];
                    H[r][c] = (double)(float)h;  // the reference holds H in fp32
                }
            float dT[16];
            solve_pose(H, cA, cB, dT);
            if (tid < 16) dT_sh[tid] = dT[tid];
        }
    }
    __syncthreads();
    const bool stop = stop_sh != 0;
    if (!stop) {
        if (tid < 16) {  // T_it = dT . T_e
            const int i = tid >> 2, j = tid & 3;
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) v += dT_sh[i * 4 + k] * T_e[k * 4 + j];
            T_sh[tid] = v;
            if (writer) a.Tbuf[((int64_t)(it & 1) * a.n_pairs + p) * 16 + tid] = v;
        }
        __syncthreads();
    }
    return stop;
}

// the block's partial of search `it`: one correspondence (or none) per thread, summed over the 256 threads in a fixed order.
// The squared residual is the DIFFERENCE a - b in fp64 (what open3d's inlier_rmse measures), not the search's fp32 value
// (-2 a.b + |a|^2) + |b|^2: that one selects the correspondence, but away from the origin it carries the cancellation error of
// |a|^2 and can be negative -- summed, it made the RMSE of coincident clouds NaN from a few metres out and biased it further out.
__device__ void icp_store_partial(const IcpArgs& a, int p, int c, int it, bool ok, float ax, float ay, float az, const float (&b)[3]) {
    __shared__ double red[4 * ICP_NP];
    double v[ICP_NP];
#pragma unroll
    for (int k = 0; k < ICP_NP; ++k) v[k] = 0.0;
    if (ok) {
        const float av[3] = {ax, ay, az};
        v[0] = 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double e = (double)av[k] - (double)b[k];
            v[1] += e * e;
            v[2 + k] = (double)av[k];
            v[5 + k] = (double)b[k];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) v[8 + r * 3 + cc] = (double)av[r] * (double)b[cc];
    }
    block_sum<ICP_NP, 256>(v, red);
    if (threadIdx.x < ICP_NP) {
        double out = v[0];
#pragma unroll
        for (int k = 1; k < ICP_NP; ++k)
            if ((int)threadIdx.x == k) out = v[k];
        a.part[(int64_t)(it & 1) * a.part_stride + (icp_chunk0(a, p) + c) * ICP_NP + threadIdx.x] = out;
    }
}

// grid (ceil(max_src_len / 256), n_pairs): [evaluate search it - 1, update T] + search it on the target grid + partial
__global__ __launch_bounds__(256) void icp_iter_kernel(IcpArgs a, const float* __restrict__ src_m, const int32_t* __restrict__ r_row0,
                                                      const scream_internal::GridParam* __restrict__ gp,
                                                      const int32_t* __restrict__ start, const float* __restrict__ sorted_prep,
                                                      const int32_t* __restrict__ sorted_idx, float thresh, int it) {
    __shared__ float T_sh[16];
    const int p = blockIdx.y, c = blockIdx.x;
    // (block 0 of this very launch may be setting the flag: a block that sees it early returns where it would have returned
    // after deriving the same stop -- the derivation is deterministic)
    if (a.done[p]) return;
    const int n = a.src_len[p];
    if (c >= icp_chunks(n)) return;
    if (it > 0) {
        if (icp_pose_step(a, p, it, c == 0, T_sh)) return;
    } else {
        if (threadIdx.x < 16) T_sh[threadIdx.x] = a.Tbuf[(int64_t)p * 16 + threadIdx.x];
        __syncthreads();
    }
    const int i = c * 256 + threadIdx.x;
    const bool in = i < n;
    float ax = 0.f, ay = 0.f, az = 0.f, d = 0.f, b[3] = {0.f, 0.f, 0.f};
    uint8_t ok = 0;
    if (in) {
        const int64_t row = (int64_t)a.src_row0[p] + i;
        const float x = src_m[row * 3 + 0], y = src_m[row * 3 + 1], z = src_m[row * 3 + 2];
        const float* t = T_sh;  // (the arithmetic of icp_transform_kernel)
        ax = t[0] * x + t[1] * y + t[2] * z + t[3];
        ay = t[4] * x + t[5] * y + t[6] * z + t[7];
        az = t[8] * x + t[9] * y + t[10] * z + t[11];
        int32_t bi;
        scream_internal::grid_search_point(gp[p], start + (int64_t)p * (ICP_GRID_CELLS + 1), sorted_prep + (int64_t)r_row0[p] * 4,
                                           sorted_idx + r_row0[p], ax, ay, az, thresh, bi, d, ok, b);
    }
    icp_store_partial(a, p, c, it, ok != 0, ax, ay, az, b);
}

// one block per pair: the evaluation (+ update) alone -- the last search's, and every iteration's on the brute-force yardstick
__global__ __launch_bounds__(256) void icp_pose_kernel(IcpArgs a, int it) {
    __shared__ float T_sh[16];
    const int p = blockIdx.x;
    if (a.done[p]) return;
    icp_pose_step(a, p, it, true, T_sh);
}

// the yardstick (scream_icp_p2p_brute_range): the partials of a search done by icp_transform_kernel + scream_nn_search (same per-thread values, same sums)
__global__ __launch_bounds__(256) void icp_partials_kernel(IcpArgs a, const float* __restrict__ q, const float* __restrict__ ref,
                                                          const int32_t* __restrict__ ref_row0, const int32_t* __restrict__ idx,
                                                          const uint8_t* __restrict__ valid, int it) {
    const int p = blockIdx.y, c = blockIdx.x;
    if (a.done[p]) return;
    const int n = a.src_len[p];
    if (c >= icp_chunks(n)) return;
    const int i = c * 256 + threadIdx.x;
    float ax = 0.f, ay = 0.f, az = 0.f, b[3] = {0.f, 0.f, 0.f};
    bool ok = false;
    if (i < n) {
        const int64_t row = (int64_t)a.src_row0[p] + i;
        ok = valid[row] != 0;
        if (ok) {
            const int64_t rrow = (int64_t)ref_row0[p] + idx[row];
            ax = q[row * 3 + 0];
            ay = q[row * 3 + 1];
            az = q[row * 3 + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k] = ref[rrow * 3 + k];
        }
    }
    icp_store_partial(a, p, c, it, ok, ax, ay, az, b);
}

// ---- host side: the arguments of a call, the workspace, and the three steps of scream_icp_p2p_range ---------------------------
struct IcpCall {  // the arguments of scream_icp_p2p_range, in its order
    const float *src, *ref;
    const int32_t *src_row0, *src_len, *ref_row0, *ref_len;
    const float *s, *c;
    int32_t n_pairs, max_src_len, max_ref_len;
    int64_t src_rows_total, ref_rows_total;
    float max_corr_dist;
    int32_t max_iter;
    float rel_fitness, rel_rmse;
    float *T, *fitness_rmse;
    int32_t* iters;
    int32_t it_begin, it_end;
    int32_t* done_flags;
    void* workspace;
    int64_t workspace_bytes;
    void* stream;
};

struct IcpWs {
    float *src_m, *ref_m;  // the clouds in the metric frame
    float* ref_prep;       // [ref_rows][4] {b, |b|^2}: what both searches read (nn_prepare_targets)
    float* ones;           // [n_pairs] the search's "scale" (it divides by it): these clouds are already metric
    IcpArgs a;             // the kernels' argument; the carve fills its workspace pointers, icp_open the rest
    int32_t* chunk0;       // a.chunk0, writable
    scream_internal::IcpGrid grid;  // a grid run only
    float* q;                       // a yardstick run only: the transformed source and what scream_nn_search writes
    uint64_t* keys;
    int32_t* idx;
    float* dmin;
    uint8_t* valid;
    int64_t bytes;
};

// THE layout of a run's workspace; from a null base it only measures.  act_len is the yardstick's, but the pose step clears it
// for every stopped pair whichever search runs, so it is always there.
IcpWs icp_carve(void* base, int64_t src_rows, int64_t ref_rows, int32_t n_pairs, bool brute) {
    Carver cv{base};
    IcpWs w{};
    w.src_m = cv.take<float>(src_rows * 3);
    w.ref_m = cv.take<float>(ref_rows * 3);
    w.ref_prep = cv.take<float>(ref_rows * 4);
    w.ones = cv.take<float>(n_pairs);
    w.a.Tbuf = cv.take<float>((int64_t)n_pairs * 32);
    w.a.state = cv.take<IcpState>((int64_t)n_pairs * 2);
    w.a.done = cv.take<int32_t>(n_pairs);
    w.a.act_len = cv.take<int32_t>(n_pairs);
    w.a.chunk0 = w.chunk0 = cv.take<int32_t>(n_pairs);
    w.a.part_stride = (src_rows / 256 + n_pairs + 1) * ICP_NP;  // a chunk per 256 rows, and a last or an only one per pair
    w.a.part = cv.take<double>(w.a.part_stride * 2);
    if (brute) {
        w.q = cv.take<float>(src_rows * 3);
        w.keys = cv.take<uint64_t>(src_rows);
        w.idx = cv.take<int32_t>(src_rows);
        w.dmin = cv.take<float>(src_rows);
        w.valid = cv.take<uint8_t>(src_rows);
    } else {
        scream_internal::icp_grid_carve(cv, ref_rows, n_pairs, &w.grid);
    }
    w.bytes = cv.used;
    return w;
}

// what a caller provides: enough for either search, and for aligning the pointer it hands in
int64_t icp_workspace_bytes(int64_t src_rows, int64_t ref_rows, int32_t n_pairs) {
    const int64_t grid = icp_carve(nullptr, src_rows, ref_rows, n_pairs, false).bytes;
    const int64_t brute = icp_carve(nullptr, src_rows, ref_rows, n_pairs, true).bytes;
    return (grid > brute ? grid : brute) + 256;
}

// argument checks + carve
int icp_open(const IcpCall& c, bool brute, IcpWs* w) {
    SCREAM_REQUIRE(c.src && c.ref && c.src_row0 && c.src_len && c.ref_row0 && c.ref_len && c.s && c.c && c.T && c.workspace, SCREAM_EINVAL);
    SCREAM_REQUIRE(c.n_pairs >= 0 && c.max_iter >= 0 && c.max_corr_dist > 0.f && c.it_begin >= 0 && c.it_end >= c.it_begin, SCREAM_EINVAL);
    SCREAM_REQUIRE(c.src_rows_total >= 0 && c.ref_rows_total >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(c.workspace_bytes >= icp_workspace_bytes(c.src_rows_total, c.ref_rows_total, c.n_pairs), SCREAM_EINVAL);
    void* base = reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(c.workspace) + 255) & ~(uintptr_t)255);
    *w = icp_carve(base, c.src_rows_total, c.ref_rows_total, c.n_pairs, brute);
    IcpArgs& a = w->a;
    a.src_row0 = c.src_row0;
    a.src_len = c.src_len;
    a.n_pairs = c.n_pairs;
    a.max_iter = c.max_iter;
    a.rel_fitness = c.rel_fitness;
    a.rel_rmse = c.rel_rmse;
    a.T_out = c.T;
    a.fit_rmse_out = c.fitness_rmse;
    a.iters_out = c.iters;
    return 0;
}

// the set-up of it_begin == 0: flags, T_0, metric clouds, the prepared targets and (a grid run) the grid over them
int icp_setup(const IcpCall& c, bool brute, const IcpWs& w, hipStream_t st) {
    const int32_t n_pairs = c.n_pairs;
    hipError_t e = hipMemsetAsync(w.a.done, 0, sizeof(int32_t) * n_pairs, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(w.a.state, 0, sizeof(IcpState) * 2 * n_pairs, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpyAsync(w.a.act_len, c.src_len, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpyAsync(w.a.Tbuf, c.T, sizeof(float) * 16 * n_pairs, hipMemcpyDeviceToDevice, st);  // T_0: parity 0
    if (e != hipSuccess) return (int)e;
    icp_chunk0_kernel<<<dim3(1), dim3(64), 0, st>>>(c.src_len, n_pairs, w.chunk0);
    fill_f32_kernel<<<dim3((n_pairs + 255) / 256), dim3(256), 0, st>>>(w.ones, 1.0f, n_pairs);
    if (c.max_src_len > 0)
        icp_to_metric_kernel<<<dim3((c.max_src_len + 255) / 256, n_pairs), dim3(256), 0, st>>>(c.src, c.src_row0, c.src_len, c.s, c.c, w.src_m);
    if (c.max_ref_len > 0)
        icp_to_metric_kernel<<<dim3((c.max_ref_len + 255) / 256, n_pairs), dim3(256), 0, st>>>(c.ref, c.ref_row0, c.ref_len, c.s, c.c, w.ref_m);
    SCREAM_LAUNCH_CHECK();
    if (brute) return 0;  // (scream_nn_search prepares the targets itself, in every iteration)
    // the targets do not move: prepare and bin them once (icp_grid.hip)
    const int rc = scream_internal::nn_prepare_targets(w.ref_m, c.ref_row0, c.ref_len, w.ones, n_pairs, c.max_ref_len, w.ref_prep, st);
    if (rc != 0) return rc;
    return scream_internal::icp_grid_build(w.ref_m, w.ref_prep, c.ref_row0, c.ref_len, n_pairs, c.max_ref_len, c.max_corr_dist, w.grid, st);
}

// launches [it_begin, it_end): launch `it` = [evaluate search it - 1, stop or update T] + search it; search max_iter is evaluated
// by a last pose launch (launch index max_iter + 1).  NOTHING here waits for the device: a pair that has stopped freezes on the
// device (its blocks return at their first instruction), and a caller that wants to stop LAUNCHING early asks for the schedule
// in pieces and reads done_flags between them (scream_hip.h).
int icp_enqueue(const IcpCall& c, bool brute, const IcpWs& w, hipStream_t st) {
    const IcpArgs& a = w.a;
    const int32_t n_pairs = c.n_pairs, max_iter = c.max_iter;
    const dim3 chunks((c.max_src_len > 0 ? c.max_src_len + 255 : 256) / 256, n_pairs);
    const float thresh = c.max_corr_dist * c.max_corr_dist;
    const int last = c.it_end < max_iter + 1 ? c.it_end : max_iter + 1;
    for (int it = c.it_begin; it < last; ++it) {
        if (brute) {  // the yardstick: the same steps as separate launches around scream_nn_search
            if (it > 0) icp_pose_kernel<<<dim3(n_pairs), dim3(256), 0, st>>>(a, it);
            if (c.max_src_len > 0)
                icp_transform_kernel<<<dim3((c.max_src_len + 255) / 256, n_pairs), dim3(256), 0, st>>>(
                    w.src_m, c.src_row0, a.act_len, a.Tbuf + (int64_t)(it & 1) * n_pairs * 16, w.q);
            SCREAM_LAUNCH_CHECK();
            const int rc = scream_nn_search(w.q, w.ref_m, c.src_row0, a.act_len, c.ref_row0, c.ref_len, w.ones, n_pairs, c.max_src_len,
                                            c.max_ref_len, c.src_rows_total, c.ref_rows_total, thresh, w.ref_prep, w.keys, w.idx, w.dmin,
                                            w.valid, c.stream);
            if (rc != 0) return rc;
            icp_partials_kernel<<<chunks, dim3(256), 0, st>>>(a, w.q, w.ref_m, c.ref_row0, w.idx, w.valid, it);
        } else {
            icp_iter_kernel<<<chunks, dim3(256), 0, st>>>(a, w.src_m, c.ref_row0, w.grid.params, w.grid.start, w.grid.sorted_prep,
                                                          w.grid.sorted_idx, thresh, it);
        }
        SCREAM_LAUNCH_CHECK();
    }
    if (c.it_end > max_iter + 1 && c.it_begin <= max_iter + 1) {
        icp_pose_kernel<<<dim3(n_pairs), dim3(256), 0, st>>>(a, max_iter + 1);
        SCREAM_LAUNCH_CHECK();
    }
    if (c.done_flags) {
        const hipError_t e = hipMemcpyAsync(c.done_flags, a.done, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// brute: every search by scream_nn_search instead of the target grid; everything else, and every result bit, is the same
int icp_range(const IcpCall& c, bool brute) {
    IcpWs w;
    int rc = icp_open(c, brute, &w);
    if (rc != 0 || c.n_pairs == 0) return rc;
    hipStream_t st = as_stream(c.stream);
    if (c.it_begin == 0) {
        rc = icp_setup(c, brute, w, st);
        if (rc != 0) return rc;
    }
    return icp_enqueue(c, brute, w, st);
}

}  // namespace

extern "C" int64_t scream_icp_workspace_bytes(int64_t src_rows_total, int64_t ref_rows_total, int32_t n_pairs) {
    if (src_rows_total < 0 || ref_rows_total < 0 || n_pairs < 0) return SCREAM_EINVAL;
    return icp_workspace_bytes(src_rows_total, ref_rows_total, n_pairs);
}

extern "C" int scream_icp_p2p_range(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                                    const int32_t* ref_row0, const int32_t* ref_len, const float* s, const float* c,
                                    int32_t n_pairs, int32_t max_src_len, int32_t max_ref_len, int64_t src_rows_total,
                                    int64_t ref_rows_total, float max_corr_dist, int32_t max_iter, float rel_fitness,
                                    float rel_rmse, float* T, float* fitness_rmse, int32_t* iters, int32_t it_begin,
                                    int32_t it_end, int32_t* done_flags, void* workspace, int64_t workspace_bytes, void* stream) {
    return icp_range(IcpCall{src, ref, src_row0, src_len, ref_row0, ref_len, s, c, n_pairs, max_src_len, max_ref_len, src_rows_total,
                             ref_rows_total, max_corr_dist, max_iter, rel_fitness, rel_rmse, T, fitness_rmse, iters, it_begin, it_end,
                             done_flags, workspace, workspace_bytes, stream},
                     false);
}

extern "C" int scream_icp_p2p_brute_range(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                                          const int32_t* ref_row0, const int32_t* ref_len, const float* s, const float* c,
                                          int32_t n_pairs, int32_t max_src_len, int32_t max_ref_len, int64_t src_rows_total,
                                          int64_t ref_rows_total, float max_corr_dist, int32_t max_iter, float rel_fitness,
                                          float rel_rmse, float* T, float* fitness_rmse, int32_t* iters, int32_t it_begin,
                                          int32_t it_end, int32_t* done_flags, void* workspace, int64_t workspace_bytes,
                                          void* stream) {
    return icp_range(IcpCall{src, ref, src_row0, src_len, ref_row0, ref_len, s, c, n_pairs, max_src_len, max_ref_len, src_rows_total,
                             ref_rows_total, max_corr_dist, max_iter, rel_fitness, rel_rmse, T, fitness_rmse, iters, it_begin, it_end,
                             done_flags, workspace, workspace_bytes, stream},
                     true);
}

// the whole schedule in one call: max_iter + 2 launches at most, none of them waited for
extern "C" int scream_icp_p2p(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                              const int32_t* ref_row0, const int32_t* ref_len, const float* s, const float* c,
                              int32_t n_pairs, int32_t max_src_len, int32_t max_ref_len, int64_t src_rows_total,
                              int64_t ref_rows_total, float max_corr_dist, int32_t max_iter, float rel_fitness,
                              float rel_rmse, float* T, float* fitness_rmse, int32_t* iters, void* workspace,
                              int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(max_iter >= 0 && max_iter < (1 << 30), SCREAM_EINVAL);
    return scream_icp_p2p_range(src, ref, src_row0, src_len, ref_row0, ref_len, s, c, n_pairs, max_src_len, max_ref_len, src_rows_total,
                                ref_rows_total, max_corr_dist, max_iter, rel_fitness, rel_rmse, T, fitness_rmse, iters, 0, max_iter + 2,
                                nullptr, workspace, workspace_bytes, stream);
}
