// Fixed-radius search for a batch of cloud pairs: ALL target points within the radius of every transformed source point (the
// reference's utils.get_correspondences, utils.py:94-108 -- one FLANN query per point in a Python loop), as a count launch and
// a fill launch over one shared workspace.
//
// The membership test is the contract of include/scream_hip.h, one IEEE float64 operation per step (pair p, M = T[p], source
// row x and target row b in fp32):
//     a_k = ((M[k][0]*x0 + M[k][1]*x1) + M[k][2]*x2) + M[k][3];   d_k = a_k - float64(b_k)
//     d2  = (d0*d0 + d1*d1) + d2*d2;   j is a neighbour of i  iff  d2 < radius * radius          (strict)
// and the neighbours of i are listed in ascending (d2, j).  Compiled with -ffp-contract=off.  Counts, ranks and (d2, j)
// comparisons do not depend on the order the candidates are visited in, so the result is a pure function of the pair: bitwise
// repeatable, independent of the other pairs and of the launch shape, equal to the brute-force float64 restatement of
// tests/radius_ref.py.  No floating-point atomics; the integer atomics below (cell counts, scatter cursors) only decide the
// order of the records INSIDE a cell, which no result depends on.
//
// The grid is a candidate filter only: cell_grid.h (D = 3, over the TARGET cloud) builds it and states why a query that scans
// cell(lo) .. cell(hi)  per axis with lo <= b_k <= hi for every neighbour b loses nobody.  The step that is this op's own: a query
// at a scans  cell(a - R) .. cell(a + R)  (both sums rounded to float64).  A neighbour has d2 < R2.  Every addend of d2 is
// non-negative and rounding is monotone, so fl(d_k * d_k) <= d2 < fl(R * R), hence d_k^2 < R^2 in real numbers (d_k^2 >= R^2
// would round to >= fl(R * R)), hence |fl(a_k - b_k)| < R, hence |a_k - b_k| < R in real numbers (|a_k - b_k| >= R would round
// to >= R, R being a float64).  So a_k - R < b_k < a_k + R; b_k is itself a float64 and rounding is monotone, so
// fl(a_k + R) >= b_k >= fl(a_k - R).  The scanned range is at most three cells per axis (cell_grid.h); the nine (y, z) runs
// below rely on that.  At most side^3 <= RAD_MAX_SIDE^3 cells per pair, side fixed per call from max_t_len: about
// RAD_CELLS_PER_ROW cells per row of the call's largest target.
//
//   grid     cell_grid_enqueue: zero, plan, count, scan, scatter
//   query    one thread per source row: the eighteen cell-start loads of its nine runs go out together (into LDS, so the run
//            loops are not unrolled), then the candidates four at a time.  The count launch and the fill launch enumerate through
//            the same for_each_candidate / dist2, so they cannot disagree.
//   fill     rank of a neighbour = number of candidates that are smaller in (d2, j): a second enumeration per neighbour, no
//            per-thread list, any count.  Cost per source row: (candidates) x (neighbours + 1) distance evaluations -- about
//            40 x 11 at 0.03 m on 0.025 m clouds; a radius that makes every point a neighbour of every point costs t_len^2 per row.
// Non-finite coordinates or matrices are outside the contract; every cell index goes through a clamp that maps NaN to 0, every
// loop is bounded by the scanned counters clamped to the cloud's length, every store is bounded by offset[], so such input
// cannot fault or hang.
#include <math.h>

#include "cell_grid.h"
#include "common.h"

namespace {

constexpr int RAD_MAX_SIDE = 64;  // 64^3 cells per pair at most (a 3 m room at the 0.03 m radius: 0.047 m cells)
constexpr int RAD_MIN_SIDE = 4;
constexpr int RAD_CELLS_PER_ROW = 8;  // indoor clouds are surfaces: most cells of a 3-D grid stay empty
constexpr double RAD_EDGE_SLACK = 1.0 + 1.0 / 1024.0;      // cell edge >= R * this: a query scans at most 3 cells per axis
constexpr int RAD_BLOCK = 256;

using RadPlan = GridPlan<3>;  // binned: the target; querying: the source

// cells per axis of every pair of a call
inline int grid_side(int32_t max_t_len) {
    int s = RAD_MIN_SIDE;
    while (s < RAD_MAX_SIDE && (int64_t)s * s * s < (int64_t)RAD_CELLS_PER_ROW * max_t_len) s *= 2;
    return s;
}

// ---- the query side: everything the count launch and the fill launch share

struct Query {
    double a[3];
    const f32x4* rec;  // the pair's records
    int* run;          // this thread's eighteen run bounds in LDS: run[r * RAD_BLOCK] = begin, run[(9 + r) * RAD_BLOCK] = end of run r
};

// The transformed source point and its nine runs of candidate records.  false: a thread beyond the pair's source rows.
__device__ __forceinline__ bool make_query(const RadPlan& p, const float* __restrict__ src, const double* __restrict__ T,
                                           const int32_t* __restrict__ cells, const f32x4* __restrict__ recs, double R, int i,
                                           int* lds, Query& q) {
    if (i >= p.q_len) return false;
    const int64_t row = (int64_t)p.q_row0 + i;
    const double x0 = (double)src[row * 3 + 0], x1 = (double)src[row * 3 + 1], x2 = (double)src[row * 3 + 2];
    const double* M = T + (int64_t)blockIdx.y * 16;
#pragma unroll
    for (int k = 0; k < 3; ++k) q.a[k] = ((M[k * 4 + 0] * x0 + M[k * 4 + 1] * x1) + M[k * 4 + 2] * x2) + M[k * 4 + 3];
    q.rec = recs + p.b_row0;
    q.run = lds + threadIdx.x;
    int c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c0[k] = cell_of(p, k, q.a[k] - R);
        c1[k] = cell_of(p, k, q.a[k] + R);
    }
    // nine (y, z) runs of x-contiguous cells; all eighteen cell-start loads go out together (a thread's time here is memory latency)
    int jb[9], je[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int y = c0[1] + r % 3, z = c0[2] + r / 3;
        const bool in = y <= c1[1] && z <= c1[2];
        const int base = in ? (z * p.n[1] + y) * p.n[0] : 0;
        const int first = base + c0[0], last = base + c1[0];
        const int b = first > 0 ? cells[first - 1] : 0, e = cells[last];
        jb[r] = in ? max(b, 0) : 0;
        je[r] = in ? min(e, p.b_len) : 0;
    }
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        q.run[r * RAD_BLOCK] = jb[r];
        q.run[(9 + r) * RAD_BLOCK] = je[r];
    }
    return true;
}

// THE distance of the contract
__device__ __forceinline__ double dist2(const Query& q, const f32x4& b) {
    const double d0 = q.a[0] - (double)b[0], d1 = q.a[1] - (double)b[1], d2 = q.a[2] - (double)b[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

// f(d2, target row) for every candidate record of the query, each exactly once, in an unspecified order
template <class F>
__device__ __forceinline__ void for_each_candidate(const Query& q, F&& f) {
    for (int r = 0; r < 9; ++r) {
        int j = q.run[r * RAD_BLOCK];
        const int je = q.run[(9 + r) * RAD_BLOCK];
        for (; j + 4 <= je; j += 4) {
            f32x4 b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = q.rec[j + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) f(dist2(q, b[u]), __float_as_int(b[u][3]));
        }
        for (; j < je; ++j) {
            const f32x4 b = q.rec[j];
            f(dist2(q, b), __float_as_int(b[3]));
        }
    }
}

// grid (ceil(max_s_len / 256), n_pairs)
__global__ __launch_bounds__(RAD_BLOCK) void radius_count_kernel(const float* __restrict__ src, const double* __restrict__ T,
                                                                const RadPlan* __restrict__ plan, int64_t cells_per_pair,
                                                                const int32_t* __restrict__ cells, const f32x4* __restrict__ recs,
                                                                double R, int32_t* __restrict__ count) {
    __shared__ int lds[18 * RAD_BLOCK];
    const RadPlan& p = plan[blockIdx.y];
    const int i = blockIdx.x * RAD_BLOCK + threadIdx.x;
    Query q;
    if (!make_query(p, src, T, cells + (int64_t)blockIdx.y * cells_per_pair, recs, R, i, lds, q)) return;
    const double R2 = R * R;
    int32_t n = 0;
    for_each_candidate(q, [&](double d2, int) { n += d2 < R2 ? 1 : 0; });
    count[(int64_t)p.q_row0 + i] = n;
}

// grid (ceil(max_s_len / 256), n_pairs)
__global__ __launch_bounds__(RAD_BLOCK) void radius_fill_kernel(const float* __restrict__ src, const double* __restrict__ T,
                                                               const RadPlan* __restrict__ plan, int64_t cells_per_pair,
                                                               const int32_t* __restrict__ cells, const f32x4* __restrict__ recs,
                                                               double R, int32_t K, const int64_t* __restrict__ offset,
                                                               int64_t s_rows, int32_t* __restrict__ pair_j) {
    __shared__ int lds[18 * RAD_BLOCK];
    const RadPlan& p = plan[blockIdx.y];
    const int i = blockIdx.x * RAD_BLOCK + threadIdx.x;
    Query q;
    if (!make_query(p, src, T, cells + (int64_t)blockIdx.y * cells_per_pair, recs, R, i, lds, q)) return;
    const double R2 = R * R;
    const int64_t row = (int64_t)p.q_row0 + i;
    // what the caller reserved for this row, inside what it reserved in all: no store leaves pair_j whatever offset[] holds
    const int64_t total = offset[s_rows], o0 = offset[row], o1 = offset[row + 1];
    if (!(o0 >= 0 && o0 <= o1 && o1 <= total)) return;
    int64_t room = o1 - o0;
    if (K > 0 && room > K) room = K;
    if (room == 0) return;
    for_each_candidate(q, [&](double d2, int j) {
        if (!(d2 < R2)) return;
        int32_t rank = 0;  // neighbours ahead of this one in (d2, j); they pass the predicate themselves, being no farther
        for_each_candidate(q, [&](double e2, int l) { rank += (e2 < d2 || (e2 == d2 && l < j)) ? 1 : 0; });
        if (rank < room) pair_j[o0 + rank] = j;
    });
}

// everything both entry points refuse, decided before any launch
inline int check_call(const void* src, const int32_t* s_row0, const int32_t* s_len, int32_t max_s_len, int64_t s_rows, const void* tgt,
                      const int32_t* t_row0, const int32_t* t_len, int32_t max_t_len, int64_t t_rows, const double* T, int32_t n_pairs,
                      double radius, const void* out, const void* workspace, int64_t workspace_bytes_given) {
    SCREAM_REQUIRE(radius > 0.0 && isfinite(radius), SCREAM_EINVAL);
    SCREAM_REQUIRE(n_pairs >= 0 && rows_ok(s_rows, max_s_len) && rows_ok(t_rows, max_t_len), SCREAM_EINVAL);
    if (n_pairs == 0) return 1;  // nothing to do
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(src && s_row0 && s_len && tgt && t_row0 && t_len && T && out && workspace, SCREAM_EINVAL);
    SCREAM_REQUIRE(workspace_bytes_given >= grid_carve<3>(nullptr, t_rows, n_pairs, grid_side(max_t_len)).bytes, SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(workspace), SCREAM_EINVAL);
    return 0;
}

}  // namespace

extern "C" int64_t scream_radius_workspace_bytes(int64_t tgt_rows_total, int32_t n_pairs, int32_t max_t_len) {
    if (n_pairs < 0 || !rows_ok(tgt_rows_total, max_t_len)) return SCREAM_EINVAL;
    return grid_carve<3>(nullptr, tgt_rows_total, n_pairs, grid_side(max_t_len)).bytes;
}

extern "C" int scream_radius_count(const float* src, const int32_t* s_row0, const int32_t* s_len, int32_t max_s_len,
                                   int64_t src_rows_total, const float* tgt, const int32_t* t_row0, const int32_t* t_len,
                                   int32_t max_t_len, int64_t tgt_rows_total, const double* T, int32_t n_pairs, double radius,
                                   int32_t* count, void* workspace, int64_t workspace_bytes_given, void* stream) {
    const int rc = check_call(src, s_row0, s_len, max_s_len, src_rows_total, tgt, t_row0, t_len, max_t_len, tgt_rows_total, T, n_pairs,
                              radius, count, workspace, workspace_bytes_given);
    if (rc != 0) return rc < 0 ? rc : 0;
    const int side = grid_side(max_t_len);
    const GridWs<3> ws = grid_carve<3>(workspace, tgt_rows_total, n_pairs, side);
    hipStream_t st = as_stream(stream);
    const int grid_rc = cell_grid_enqueue<3>(tgt, t_row0, t_len, max_t_len, tgt_rows_total, s_row0, s_len, max_s_len, src_rows_total, n_pairs,
                                             radius, RAD_EDGE_SLACK, side, ws, st);
    if (grid_rc != 0) return grid_rc;
    if (max_s_len > 0) {
        radius_count_kernel<<<dim3(row_blocks(max_s_len), n_pairs), dim3(RAD_BLOCK), 0, st>>>(src, T, ws.plan, ws.cells_per_pair, ws.cells, ws.recs,
                                                                                               radius, count);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int scream_radius_pairs(const float* src, const int32_t* s_row0, const int32_t* s_len, int32_t max_s_len,
                                   int64_t src_rows_total, const float* tgt, const int32_t* t_row0, const int32_t* t_len,
                                   int32_t max_t_len, int64_t tgt_rows_total, const double* T, int32_t n_pairs, double radius,
                                   void* workspace, int64_t workspace_bytes_given, int32_t K, const int64_t* offset, int32_t* pair_j,
                                   void* stream) {
    const int rc = check_call(src, s_row0, s_len, max_s_len, src_rows_total, tgt, t_row0, t_len, max_t_len, tgt_rows_total, T, n_pairs,
                              radius, pair_j, workspace, workspace_bytes_given);
    if (rc != 0) return rc < 0 ? rc : 0;
    SCREAM_REQUIRE(offset, SCREAM_EINVAL);
    if (max_s_len == 0) return 0;
    const GridWs<3> ws = grid_carve<3>(workspace, tgt_rows_total, n_pairs, grid_side(max_t_len));
    radius_fill_kernel<<<dim3(row_blocks(max_s_len), n_pairs), dim3(RAD_BLOCK), 0, as_stream(stream)>>>(
        src, T, ws.plan, ws.cells_per_pair, ws.cells, ws.recs, radius, K, offset, src_rows_total, pair_j);
    SCREAM_LAUNCH_CHECK();
    return 0;
}
