// Point-to-point ICP of RAW scans in float64 (scream_icp_raw_range / scream_icp_raw_nn): the pose refinement that
// datasets/kitti.py:105-126 runs with open3d.registration_icp on the unvoxelised clouds (two scans of ~120 k points spanning
// +-80 m, radius 0.2 m) before anything is voxelised.  scream_icp_p2p (icp_p2p.hip + icp_grid.hip) selects with the fp32 expanded
// form and bins into a dense grid capped at 2^17 cells; neither holds at this extent.  Here every step is ONE IEEE float64
// operation in a fixed order (this file is compiled with -ffp-contract=off), and the grid is sparse.
//
// The contract (include/scream_hip.h states it for callers; tests/rawicp_ref.py restates it in numpy):
//   transform   a_k = ((t_k0 x + t_k1 y) + t_k2 z) + t_k3 in float64 from the fp32 row and the float64 T
//   distance    d2 = (dx^2 + dy^2) + dz^2 from the direct differences d = a - b, b the fp32 target row widened
//   selection   the nearest target row; equal d2 goes to the LOWEST original target row
//   rule        a correspondence iff d2 < r2, strictly, r2 = max_corr_dist * max_corr_dist (the double product)
//   sums        per evaluation count, sum d2, sum a, sum b, sum a b^T (17 doubles).  A chunk = 256 consecutive source rows; a
//               row without a correspondence contributes 0.0 to every sum.  Inside a chunk: the 64 rows of a wave by the
//               butterfly  v += v[lane ^ 1], ^ 2, ^ 4, ^ 8, ^ 16, ^ 32  (every lane ends with the same value), then the four
//               waves as (w0 + w1) + (w2 + w3).  The chunk sums of a pair are then added SEQUENTIALLY in ascending chunk order
//               from 0.0 by one lane per quantity of the pair's pose block.  No float atomics; nothing depends on the batch.
//   evaluation  fitness = cnt / N, inlier_rmse = sqrt(sum d2 / cnt) (0 when cnt == 0; fitness 0 when N == 0)
//   stop        after the evaluation e (e = the number of updates applied) with e >= 1 and |d fitness| < rel_fitness and
//               |d rmse| < rel_rmse against evaluation e - 1, in float64, or with e == max_iter
//   update      cA = sum a / cnt, cB = sum b / cnt; H = sum a b^T - cA (sum b)^T, entry by entry; U, V from jacobi_svd3 (svd3.h);
//               delta = -1 if det3(V) * det3(U) < 0 else 1; R_ij = (V_i0 U_j0 + V_i1 U_j1) + delta * V_i2 * U_j2;
//               t_i = cB_i - ((R_i0 cA_0 + R_i1 cA_1) + R_i2 cA_2); T <- dT . T with every entry
//               ((dT_i0 T_0j + dT_i1 T_1j) + dT_i2 T_2j) + dT_i3 T_3j.  cnt == 0: the identity, T is not touched.
//
// The candidate filter.  The target is binned by voxel_sort.h with cell edge h = max_corr_dist: origin = min_bound - h / 2,
// cell(v) = floor((v - origin) / h) per axis, a monotone float64 function, and (key, row) sorted by key = i << (bj + bk) | j << bk
// | k.  A query scans cell(a - R) .. cell(a + R) per axis, clamped to the grid.  That range holds every b with d2 < r2: d2 < r2
// implies fl(dx^2) < fl(R^2) (sums of non-negative terms and roundings are monotone), hence |fl(a - b)| < R, hence a - R < b <
// a + R in the reals (fl(a - b) >= R whenever a - b >= R), hence fl(a - R) <= b <= fl(a + R) because b is representable, and the
// cell function is monotone.  The grid only filters: the result is the brute-force search's, bit for bit.
// For every (i, j) column of the range the cells k_lo .. k_hi are contiguous in key order, so a column costs two binary searches
// over the sorted keys; the searches of up to four columns are stepped together (eight independent loads per step).  Records
// {x, y, z, original row} (16 bytes) sit in sorted order.  Per iteration: one search launch (one thread per source row, one block
// per chunk) and one pose launch (one wave per pair: reduce, evaluate, stop or update).
//
// A pair whose target needs more than 2^21 cells on an axis, that holds a non-finite coordinate (source or target), whose rows
// do not fit what the caller declared, or a call whose radius is not positive and finite: iters = -1, T untouched, flag set;
// the other pairs are unaffected (the rule of voxel.hip).
#include <math.h>

#include "common.h"
#include "svd3.h"
#include "voxel_sort.h"

namespace {

constexpr int RI_NP = 17;  // doubles per partial

struct RawCarve {
    double* voxel;     // [n_pairs] the cell edge, for voxel_bounds_kernel
    int32_t* status;   // [n_pairs] 0 / -1
    int32_t* done;     // [n_pairs]
    int32_t* chunk0;   // [n_pairs] first chunk partial of the pair
    int32_t* src_ok;   // [n_pairs] source rows declared consistently and finite
    int32_t* n_src;    // [n_pairs] the validated source length (0 for a refused pair)
    double* state;     // [n_pairs][2] fitness, rmse of the last evaluation
    double* part;      // [chunks_cap][RI_NP]
    f32x4* rec;        // [tgt_rows] sorted records
    void* sort_ws;     // where the voxel sort's buffers begin (no kernel reads it; the kernels take this struct by value)
};
struct RawSetup {
    RawCarve cv;
    Carve sort;
    int64_t bytes;
};

inline int64_t chunks_cap(int64_t src_rows, int32_t n_pairs) { return src_rows / 256 + n_pairs + 1; }
// THE layout of a run: its own buffers, then the voxel sort's.  From a null base it only measures: `bytes` is what
// scream_icp_raw_workspace_bytes reports and what both entry points ask for.
inline RawSetup raw_carve(void* workspace, int64_t src_rows, int64_t tgt_rows, int32_t n_pairs) {
    Carver w{workspace};
    RawSetup su;
    RawCarve& c = su.cv;
    c.voxel = w.take<double>(n_pairs);
    c.status = w.take<int32_t>(n_pairs);
    c.done = w.take<int32_t>(n_pairs);
    c.chunk0 = w.take<int32_t>(n_pairs);
    c.src_ok = w.take<int32_t>(n_pairs);
    c.n_src = w.take<int32_t>(n_pairs);
    c.state = w.take<double>(2 * (int64_t)n_pairs);
    c.part = w.take<double>(chunks_cap(src_rows, n_pairs) * RI_NP);
    c.rec = w.take<f32x4>(tgt_rows);
    su.sort = voxel_carve(w, tgt_rows, n_pairs);
    c.sort_ws = su.sort.plan;
    su.bytes = w.used;
    return su;
}

__device__ __forceinline__ int raw_chunks(int n) { return n > 0 ? (n + 255) / 256 : 1; }  // an empty source keeps its block 0

__global__ __launch_bounds__(256) void raw_fill_kernel(double* __restrict__ p, double v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// grid n_pairs, block 256: the source rows against what the caller declared, and their finiteness
__global__ __launch_bounds__(256) void raw_src_check_kernel(const float* __restrict__ src, const int32_t* __restrict__ row0,
                                                           const int32_t* __restrict__ len, int32_t max_len, int64_t rows_total,
                                                           int32_t* __restrict__ src_ok) {
    __shared__ int bad_sh;
    const int p = blockIdx.x;
    const int64_t r0 = row0[p], n = len[p];
    const bool fits = r0 >= 0 && n >= 0 && n <= max_len && r0 + n <= rows_total;
    if (threadIdx.x == 0) bad_sh = fits ? 0 : 1;
    __syncthreads();
    if (!fits) {
        if (threadIdx.x == 0) src_ok[p] = 0;
        return;
    }
    int bad = 0;
    for (int64_t i = threadIdx.x; i < n * 3; i += 256) bad |= !isfinite(src[r0 * 3 + i]);
    if (bad) atomicOr(&bad_sh, 1);
    __syncthreads();
    if (threadIdx.x == 0) src_ok[p] = bad_sh ? 0 : 1;
}

// one thread: the status of every pair, its chunk slots (a prefix sum over the pairs, so the clouds may be packed in any order)
// and the start state.  A pair whose chunks would not fit the table (possible only when source clouds overlap) is refused.
__global__ void raw_status_kernel(const CloudPlan* __restrict__ plan, const int32_t* __restrict__ src_len, RawCarve cv, double radius,
                                  int32_t n_pairs, int64_t cap, int32_t* __restrict__ iters, int32_t* __restrict__ status_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool r_ok = radius > 0.0 && isfinite(radius) && isfinite(radius * radius);
    int64_t acc = 0;
    for (int p = 0; p < n_pairs; ++p) {
        bool ok = r_ok && plan[p].status == 0 && cv.src_ok[p] != 0;
        const int n = ok ? src_len[p] : 0;
        if (ok && acc + raw_chunks(n) > cap) ok = false;
        cv.status[p] = ok ? 0 : -1;
        cv.done[p] = ok ? 0 : 1;
        cv.n_src[p] = ok ? n : 0;
        cv.chunk0[p] = (int32_t)acc;
        cv.state[2 * p + 0] = 0.0;
        cv.state[2 * p + 1] = 0.0;
        if (ok) acc += raw_chunks(n);
        if (iters) iters[p] = ok ? 0 : -1;
        if (status_out) status_out[p] = ok ? 0 : -1;
    }
}

// grid (ceil(max_tgt_len / 256), n_pairs): the record of sorted position s
__global__ __launch_bounds__(256) void raw_records_kernel(const float* __restrict__ tgt, const CloudPlan* __restrict__ plan,
                                                         const int32_t* __restrict__ rows0, const int32_t* __restrict__ rows1,
                                                         f32x4* __restrict__ rec) {
    const CloudPlan& p = plan[blockIdx.y];
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (p.status || s >= p.len) return;
    const int32_t* rows = ((p.npass & 1) ? rows1 : rows0) + p.row0;
    const int row = min(max(rows[s], 0), p.len - 1);  // (the clamp keeps the address inside the cloud whatever the workspace held)
    const int64_t g = (int64_t)p.row0 + row;
    f32x4 r;
    r.x = tgt[g * 3 + 0];
    r.y = tgt[g * 3 + 1];
    r.z = tgt[g * 3 + 2];
    r.w = __int_as_float(row);
    rec[(int64_t)p.row0 + s] = r;
}

// The search of one query a under the plan p.  best_row = -1 and best_d2 = +inf when no target row has d2 < r2.
__device__ __forceinline__ void raw_search(const CloudPlan& p, const uint64_t* __restrict__ keys, const f32x4* __restrict__ rec,
                                           const double a[3], double R, double r2, int& best_row, double& best_d2, float b[3]) {
    best_row = -1;
    best_d2 = INFINITY;
    b[0] = b[1] = b[2] = 0.f;
    const int n = p.len;
    if (n <= 0) return;
    int64_t lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double top = (double)(((int64_t)1 << p.bits[k]) - 1);
        const double cl = floor(((a[k] - R) - p.origin[k]) / p.voxel), ch = floor(((a[k] + R) - p.origin[k]) / p.voxel);
        if (!(ch >= 0.0) || !(cl <= top)) return;  // beside the grid, or a is not finite
        lo[k] = (int64_t)fmax(cl, 0.0);
        hi[k] = (int64_t)fmin(ch, top);
    }
    int top_step = 1;
    while (top_step <= n / 2) top_step <<= 1;  // the largest power of two <= n (uniform over the pair)
    int brow = INT32_MAX;
    double best = INFINITY;
    f32x4 brec = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = lo[0]; i <= hi[0]; ++i)
        for (int64_t j0 = lo[1]; j0 <= hi[1]; j0 += 4) {
            uint64_t klo[4], khi[4];
            bool on[4];
            int pb[4], pe[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                on[c] = j0 + c <= hi[1];
                const uint64_t base = ((uint64_t)i << p.shift_i) | ((uint64_t)(j0 + c) << p.shift_j);
                klo[c] = base | (uint64_t)lo[2];
                khi[c] = base | (uint64_t)hi[2];
                pb[c] = 0;
                pe[c] = 0;
            }
            // pb = the number of keys < klo, pe = the number of keys <= khi
            for (int s = top_step; s > 0; s >>= 1) {
                uint64_t vb[4], ve[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    vb[c] = (on[c] && pb[c] + s <= n) ? keys[pb[c] + s - 1] : ~0ull;
                    ve[c] = (on[c] && pe[c] + s <= n) ? keys[pe[c] + s - 1] : ~0ull;
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (vb[c] < klo[c]) pb[c] += s;
                    if (ve[c] <= khi[c]) pe[c] += s;
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (!on[c]) continue;
#pragma unroll 4
                for (int s = pb[c]; s < pe[c]; ++s) {
                    const f32x4 r = rec[s];
                    const double dx = a[0] - (double)r.x, dy = a[1] - (double)r.y, dz = a[2] - (double)r.z;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const int row = __float_as_int(r.w);
                    if (d2 < best || (d2 == best && row < brow)) {
                        best = d2;
                        brow = row;
                        brec = r;
                    }
                }
            }
        }
    if (best < r2) {
        best_row = brow;
        best_d2 = best;
        b[0] = brec.x;
        b[1] = brec.y;
        b[2] = brec.z;
    }
}

__device__ __forceinline__ void raw_transform(const double* __restrict__ T, const float* __restrict__ x, double a[3]) {
    const double px = (double)x[0], py = (double)x[1], pz = (double)x[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = ((T[k * 4 + 0] * px + T[k * 4 + 1] * py) + T[k * 4 + 2] * pz) + T[k * 4 + 3];
}

// grid (chunks, n_pairs), block 256: search under the pair's current T and the chunk's partial
__global__ __launch_bounds__(256) void raw_search_kernel(const float* __restrict__ src, const int32_t* __restrict__ src_row0,
                                                        const int32_t* __restrict__ tgt_row0, const CloudPlan* __restrict__ plan,
                                                        const uint64_t* __restrict__ keys0, const uint64_t* __restrict__ keys1,
                                                        RawCarve cv, const double* __restrict__ T, double R, double r2) {
    __shared__ double red[4][RI_NP];
    const int pr = blockIdx.y, c = blockIdx.x;
    if (cv.done[pr]) return;  // stopped or refused (block-uniform; set by an EARLIER launch only)
    const int n = cv.n_src[pr];
    if (c >= raw_chunks(n)) return;
    const CloudPlan& p = plan[pr];
    const int i = c * 256 + threadIdx.x;
    double v[RI_NP];
#pragma unroll
    for (int k = 0; k < RI_NP; ++k) v[k] = 0.0;
    if (i < n) {
        double a[3];
        raw_transform(T + (int64_t)pr * 16, src + ((int64_t)src_row0[pr] + i) * 3, a);
        int row;
        double d2;
        float b[3];
        raw_search(p, ((p.npass & 1) ? keys1 : keys0) + p.row0, cv.rec + p.row0, a, R, r2, row, d2, b);
        if (row >= 0) {
            v[0] = 1.0;
            v[1] = d2;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[2 + k] = a[k];
                v[5 + k] = (double)b[k];
            }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) v[8 + r * 3 + cc] = a[r] * (double)b[cc];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < RI_NP; ++k) v[k] = wave_sum_f64(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < RI_NP; ++k) red[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < RI_NP) {
        const int k = threadIdx.x;
        cv.part[((int64_t)cv.chunk0[pr] + c) * RI_NP + k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    }
}

// grid (chunks, n_pairs), block 256: the search alone, under the caller's T
__global__ __launch_bounds__(256) void raw_nn_kernel(const float* __restrict__ src, const int32_t* __restrict__ src_row0,
                                                    const CloudPlan* __restrict__ plan, const uint64_t* __restrict__ keys0,
                                                    const uint64_t* __restrict__ keys1, RawCarve cv, const double* __restrict__ T,
                                                    double R, double r2, int32_t* __restrict__ idx, double* __restrict__ d2_out) {
    const int pr = blockIdx.y;
    if (cv.status[pr]) return;
    const int n = cv.n_src[pr], i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const CloudPlan& p = plan[pr];
    const int64_t g = (int64_t)src_row0[pr] + i;
    double a[3], d2;
    raw_transform(T + (int64_t)pr * 16, src + g * 3, a);
    int row;
    float b[3];
    raw_search(p, ((p.npass & 1) ? keys1 : keys0) + p.row0, cv.rec + p.row0, a, R, r2, row, d2, b);
    idx[g] = row;
    d2_out[g] = d2;
}

// grid n_pairs, block 64: evaluation e of the pair from its chunk partials; stop, or T <- dT . T
__global__ __launch_bounds__(64) void raw_pose_kernel(RawCarve cv, int e, int32_t max_iter, double rel_fitness, double rel_rmse,
                                                     double* __restrict__ T_all, double* __restrict__ fit_rmse,
                                                     int32_t* __restrict__ iters) {
    __shared__ double tot_sh[RI_NP];
    const int p = blockIdx.x, lane = threadIdx.x;
    if (cv.done[p]) return;
    const int n = cv.n_src[p], nb = raw_chunks(n);
    if (lane < RI_NP) {
        const double* part = cv.part + (int64_t)cv.chunk0[p] * RI_NP + lane;
        double s = 0.0;
        for (int c = 0; c < nb; ++c) s += part[(int64_t)c * RI_NP];
        tot_sh[lane] = s;
    }
    __syncthreads();
    double tot[RI_NP];
#pragma unroll
    for (int k = 0; k < RI_NP; ++k) tot[k] = tot_sh[k];
    const double cnt = tot[0];
    const double fitness = n > 0 ? cnt / (double)n : 0.0;
    const double rmse = cnt > 0.0 ? sqrt(tot[1] / cnt) : 0.0;
    const double pf = cv.state[2 * p + 0], prm = cv.state[2 * p + 1];  // evaluation e - 1
    const bool converged = e > 0 && fabs(pf - fitness) < rel_fitness && fabs(prm - rmse) < rel_rmse;
    const bool stop = converged || e >= max_iter;
    double* T = T_all + (int64_t)p * 16;
    double Told[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Told[k] = T[k];
    __syncthreads();  // every lane holds the state and T before lane 0 / lanes 0..15 replace them
    if (lane == 0) {
        cv.state[2 * p + 0] = fitness;
        cv.state[2 * p + 1] = rmse;
        if (fit_rmse) {
            fit_rmse[2 * p + 0] = fitness;
            fit_rmse[2 * p + 1] = rmse;
        }
        if (iters) iters[p] = e;  // the number of updates applied
        if (stop) cv.done[p] = 1;
    }
    if (stop || !(cnt > 0.0)) return;  // no correspondence: the identity update, T stays bit for bit
    const double cA[3] = {tot[2] / cnt, tot[3] / cnt, tot[4] / cnt}, cB[3] = {tot[5] / cnt, tot[6] / cnt, tot[7] / cnt};
    double H[3][3], U[3][3], V[3][3], sig[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) H[r][c] = tot[8 + r * 3 + c] - cA[r] * tot[5 + c];
    jacobi_svd3(H, U, V, sig);
    const double delta = det3(V) * det3(U) < 0.0 ? -1.0 : 1.0;
    double dT[16];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dT[i * 4 + j] = (V[i][0] * U[j][0] + V[i][1] * U[j][1]) + delta * V[i][2] * U[j][2];
        dT[i * 4 + 3] = cB[i] - ((dT[i * 4 + 0] * cA[0] + dT[i * 4 + 1] * cA[1]) + dT[i * 4 + 2] * cA[2]);
    }
    dT[12] = dT[13] = dT[14] = 0.0;
    dT[15] = 1.0;
    if (lane < 16) {  // entry (ii, jj) by the lane that owns it; constant indices keep dT and Told in registers
        double out = 0.0;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
                if (ii * 4 + jj == lane)
                    out = ((dT[ii * 4 + 0] * Told[0 * 4 + jj] + dT[ii * 4 + 1] * Told[1 * 4 + jj]) + dT[ii * 4 + 2] * Told[2 * 4 + jj]) +
                          dT[ii * 4 + 3] * Told[3 * 4 + jj];
        T[lane] = out;
    }
}

// enqueue the set-up of a carved run: target grid, records, pair status
int raw_setup(const float* src, const float* tgt, const int32_t* src_row0, const int32_t* src_len, const int32_t* tgt_row0,
              const int32_t* tgt_len, int32_t n_pairs, int32_t max_src_len, int32_t max_tgt_len, int64_t src_rows_total,
              int64_t tgt_rows_total, double radius, const RawSetup& su, int32_t* iters, int32_t* status_out, hipStream_t st) {
    const RawCarve& cv = su.cv;
    raw_fill_kernel<<<dim3((n_pairs + 255) / 256), dim3(256), 0, st>>>(cv.voxel, radius, n_pairs);
    SCREAM_LAUNCH_CHECK();
    const int rc = voxel_sort_enqueue(tgt, tgt_row0, tgt_len, n_pairs, max_tgt_len, cv.voxel, tgt_rows_total, su.sort, st);
    if (rc != 0) return rc;
    raw_src_check_kernel<<<dim3(n_pairs), dim3(256), 0, st>>>(src, src_row0, src_len, max_src_len, src_rows_total, cv.src_ok);
    SCREAM_LAUNCH_CHECK();
    raw_status_kernel<<<dim3(1), dim3(64), 0, st>>>(su.sort.plan, src_len, cv, radius, n_pairs, chunks_cap(src_rows_total, n_pairs),
                                                   iters, status_out);
    SCREAM_LAUNCH_CHECK();
    if (max_tgt_len > 0) {
        raw_records_kernel<<<dim3((max_tgt_len + 255) / 256, n_pairs), dim3(256), 0, st>>>(tgt, su.sort.plan, su.sort.rows[0],
                                                                                          su.sort.rows[1], cv.rec);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}

bool raw_args_ok(int32_t n_pairs, int32_t max_src_len, int32_t max_tgt_len, int64_t src_rows_total, int64_t tgt_rows_total) {
    return n_pairs >= 0 && max_src_len >= 0 && max_tgt_len >= 0 && src_rows_total >= 0 && tgt_rows_total >= 0 &&
           src_rows_total <= INT32_MAX && tgt_rows_total <= INT32_MAX;
}

}  // namespace

extern "C" int64_t scream_icp_raw_workspace_bytes(int64_t src_rows_total, int64_t tgt_rows_total, int32_t n_pairs) {
    if (!raw_args_ok(n_pairs, 0, 0, src_rows_total, tgt_rows_total)) return SCREAM_EINVAL;
    return raw_carve(nullptr, src_rows_total, tgt_rows_total, n_pairs).bytes;
}

extern "C" int scream_icp_raw_range(const float* src, const float* tgt, const int32_t* src_row0, const int32_t* src_len,
                                    const int32_t* tgt_row0, const int32_t* tgt_len, int32_t n_pairs, int32_t max_src_len,
                                    int32_t max_tgt_len, int64_t src_rows_total, int64_t tgt_rows_total, double max_corr_dist,
                                    int32_t max_iter, double rel_fitness, double rel_rmse, double* T, double* fitness_rmse,
                                    int32_t* iters, int32_t it_begin, int32_t it_end, int32_t* done_flags, void* workspace,
                                    int64_t workspace_bytes_given, void* stream) {
    SCREAM_REQUIRE(src && tgt && src_row0 && src_len && tgt_row0 && tgt_len && T && workspace, SCREAM_EINVAL);
    SCREAM_REQUIRE(raw_args_ok(n_pairs, max_src_len, max_tgt_len, src_rows_total, tgt_rows_total), SCREAM_EINVAL);
    SCREAM_REQUIRE(max_iter >= 0 && max_iter < (1 << 30) && it_begin >= 0 && it_end >= it_begin, SCREAM_EINVAL);
    const RawSetup su = raw_carve(workspace, src_rows_total, tgt_rows_total, n_pairs);
    SCREAM_REQUIRE(workspace_bytes_given >= su.bytes && aligned256(workspace), SCREAM_EINVAL);
    if (n_pairs == 0) return 0;
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    hipStream_t st = as_stream(stream);
    if (it_begin == 0) {
        const int rc = raw_setup(src, tgt, src_row0, src_len, tgt_row0, tgt_len, n_pairs, max_src_len, max_tgt_len, src_rows_total,
                                 tgt_rows_total, max_corr_dist, su, iters, nullptr, st);
        if (rc != 0) return rc;
    }
    const dim3 chunks((max_src_len > 0 ? max_src_len + 255 : 256) / 256, n_pairs);
    const double r2 = max_corr_dist * max_corr_dist;
    // launch pair `it` = search under T_it, then evaluation it: stop, or T_{it+1} = dT . T_it.  Nothing here waits for the device.
    const int last = it_end < max_iter + 1 ? it_end : max_iter + 1;
    for (int it = it_begin; it < last; ++it) {
        raw_search_kernel<<<chunks, dim3(256), 0, st>>>(src, src_row0, tgt_row0, su.sort.plan, su.sort.keys[0], su.sort.keys[1], su.cv, T,
                                                        max_corr_dist, r2);
        SCREAM_LAUNCH_CHECK();
        raw_pose_kernel<<<dim3(n_pairs), dim3(64), 0, st>>>(su.cv, it, max_iter, rel_fitness, rel_rmse, T, fitness_rmse, iters);
        SCREAM_LAUNCH_CHECK();
    }
    if (done_flags) {
        const hipError_t e = hipMemcpyAsync(done_flags, su.cv.done, sizeof(int32_t) * n_pairs, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int scream_icp_raw_nn(const float* src, const float* tgt, const int32_t* src_row0, const int32_t* src_len,
                                 const int32_t* tgt_row0, const int32_t* tgt_len, int32_t n_pairs, int32_t max_src_len,
                                 int32_t max_tgt_len, int64_t src_rows_total, int64_t tgt_rows_total, double radius, const double* T,
                                 int32_t* idx, double* d2, int32_t* status, void* workspace, int64_t workspace_bytes_given,
                                 void* stream) {
    SCREAM_REQUIRE(src && tgt && src_row0 && src_len && tgt_row0 && tgt_len && T && idx && d2 && workspace, SCREAM_EINVAL);
    SCREAM_REQUIRE(raw_args_ok(n_pairs, max_src_len, max_tgt_len, src_rows_total, tgt_rows_total), SCREAM_EINVAL);
    const RawSetup su = raw_carve(workspace, src_rows_total, tgt_rows_total, n_pairs);
    SCREAM_REQUIRE(workspace_bytes_given >= su.bytes && aligned256(workspace), SCREAM_EINVAL);
    if (n_pairs == 0) return 0;
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    hipStream_t st = as_stream(stream);
    const int rc = raw_setup(src, tgt, src_row0, src_len, tgt_row0, tgt_len, n_pairs, max_src_len, max_tgt_len, src_rows_total,
                             tgt_rows_total, radius, su, nullptr, status, st);
    if (rc != 0) return rc;
    if (max_src_len > 0) {
        raw_nn_kernel<<<dim3((max_src_len + 255) / 256, n_pairs), dim3(256), 0, st>>>(src, src_row0, su.sort.plan, su.sort.keys[0],
                                                                                     su.sort.keys[1], su.cv, T, radius, radius * radius,
                                                                                     idx, d2);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}
