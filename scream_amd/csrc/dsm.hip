// DSM extraction for a batch of OpenGF windows (the reference's process_open_gf.py:219-228, its per-ground-point loop on the
// GPU) and the assembly of the [n,6] sample rows (process_open_gf.py:234-242).
//
// Per ground point q of a cloud: the window ("patch") point with the largest z among those within the radius of q in the xy
// plane; equal z -> the lowest patch row; nobody within the radius -> q itself.  The membership test is the contract of
// include/scream_hip.h, one IEEE operation per step:
//     dx = float32(p.x - q.x), dy = float32(p.y - q.y);  d2 = float64(dx)^2 + float64(dy)^2;  candidate iff d2 <= R^2
// with R = float64(float32(radius)), so R^2 and both products are exact in float64 and the sum is rounded once.  Maxima and
// (z, row) comparisons do not depend on the order the candidates are visited in, so the result is a pure function of the
// cloud: bitwise repeatable, independent of the other clouds and of the launch shape, and equal bit for bit to the brute-force
// float64 restatement of tests/dsm_ref.py.  No floating-point atomics; the integer atomics below (cell counts, scatter cursors)
// only decide the order of the records INSIDE a cell, which no result depends on.  Compiled with -ffp-contract=off.
//
// The grid is a candidate filter only: cell_grid.h (D = 2, the xy plane, over the patch) builds it and states why a query that
// scans  cell(lo) .. cell(hi)  per axis with lo <= p.x <= hi for every candidate p loses nobody.  The step that is this op's own:
// a query scans  cell(q - Rs) .. cell(q + Rs),  Rs = R * (1 + 2^-20).  A candidate has |float32(p.x - q.x)| <= R, so
// |p.x - q.x| <= R (1 + 2^-24) in real numbers (half an fp32 ulp of R at most, R being an fp32 value); q.x + Rs rounded to
// float64 is then still >= p.x, and q.x - Rs <= p.x (the slack R (2^-20 - 2^-24) is far above a float64 ulp of any fp32
// coordinate whose fp32 difference to q.x could be as small as R).  side^2 <= DSM_GRID_CELLS cells per cloud, side fixed per
// call from max_p_len: about one cell per row of the call's largest patch, so small clouds get small tables.
//
//   grid     cell_grid_enqueue: zero, plan, count, scan, scatter
//   query    one thread per ground point: at most three runs of records (one per grid row), candidates tested four at a time
//   assemble (second entry point) per-cloud fp32 min / max over dsm and dem rows, centre = float32(min + max) / 2, rows
//            float32(dsm - centre) | float32(dem - centre)
// A lone 100 m window is ~10^4 queries = 40 blocks on 256 CUs: latency-bound whatever the block shape.  The design point is the
// batched call (64 windows: 2 500 blocks of 256 queries, ten waves per SIMD's worth of independent loads).
// Non-finite coordinates are outside the contract; every loop of the query is bounded by the scanned counters clamped to the
// patch's length, so such input cannot fault or hang.
#include <math.h>

#include "cell_grid.h"
#include "common.h"

namespace {

constexpr int DSM_GRID_CELLS = 1 << 14;    // cells per cloud at most (128 x 128: a 100 m window at the 0.8 m radius has 125 x 125)
constexpr int DSM_MAX_SIDE = 128;
constexpr int DSM_MIN_SIDE = 8;
constexpr double DSM_EDGE_SLACK = 1.0 + 1.0 / 1024.0;       // cell edge >= R * this: a disc touches at most 3 cells per axis
constexpr double DSM_REACH_SLACK = 1.0 + 1.0 / 1048576.0;   // Rs = R * this (see the header of this file)
static_assert(DSM_MAX_SIDE * DSM_MAX_SIDE <= DSM_GRID_CELLS, "grid cap");

using DsmPlan = GridPlan<2>;  // binned: the patch; querying: the dem

// cells per axis of every cloud of a call: about one cell per patch row
inline int grid_side(int32_t max_p_len) {
    int s = DSM_MIN_SIDE;
    while (s < DSM_MAX_SIDE && (int64_t)s * s < (int64_t)max_p_len) s *= 2;
    return s;
}

// grid (ceil(max_d_len / 256), n_clouds)
__global__ __launch_bounds__(256) void dsm_query_kernel(const float* __restrict__ dem, const DsmPlan* __restrict__ plan, int side,
                                                       const int32_t* __restrict__ cells, const f32x4* __restrict__ recs,
                                                       double R, float* __restrict__ out_xyz, int32_t* __restrict__ out_idx) {
    const DsmPlan& p = plan[blockIdx.y];
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= p.q_len) return;
    const int64_t qrow = (int64_t)p.q_row0 + qi;
    const float qx = dem[qrow * 3 + 0], qy = dem[qrow * 3 + 1], qz = dem[qrow * 3 + 2];
    const double R2 = R * R, Rs = R * DSM_REACH_SLACK;
    float bx = qx, by = qy, bz = qz;
    int bi = -1;
    if (p.b_len > 0) {
        const int32_t* cell = cells + (int64_t)blockIdx.y * side * side;
        const f32x4* rec = recs + p.b_row0;
        const int x0 = cell_of(p, 0, (double)qx - Rs), x1 = cell_of(p, 0, (double)qx + Rs);
        const int y0 = cell_of(p, 1, (double)qy - Rs), y1 = cell_of(p, 1, (double)qy + Rs);
        auto take = [&](const f32x4& r) {
            const float dx = r[0] - qx, dy = r[1] - qy;
            const double d2 = (double)dx * (double)dx + (double)dy * (double)dy;
            const int i = __float_as_int(r[3]);
            if (d2 <= R2 && (bi < 0 || r[2] > bz || (r[2] == bz && i < bi))) {
                bx = r[0];
                by = r[1];
                bz = r[2];
                bi = i;
            }
        };
        for (int y = y0; y <= y1; ++y) {
            const int c0 = y * p.n[0] + x0, c1 = y * p.n[0] + x1;
            int j = c0 > 0 ? cell[c0 - 1] : 0, je = cell[c1];
            j = max(j, 0);
            je = min(je, p.b_len);
            for (; j + 4 <= je; j += 4) {
                f32x4 r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = rec[j + u];
#pragma unroll
                for (int u = 0; u < 4; ++u) take(r[u]);
            }
            for (; j < je; ++j) take(rec[j]);
        }
    }
    out_xyz[qrow * 3 + 0] = bx;
    out_xyz[qrow * 3 + 1] = by;
    out_xyz[qrow * 3 + 2] = bz;
    out_idx[qrow] = bi;
}

// grid n_clouds, block 256: centre[c] = float32(min + max) / 2 per axis over the cloud's dsm and dem rows
__global__ __launch_bounds__(256) void dsm_centre_kernel(const float* __restrict__ dsm, const float* __restrict__ dem,
                                                        const int32_t* __restrict__ row0, const int32_t* __restrict__ len,
                                                        int32_t max_len, int64_t rows, float* __restrict__ centre) {
    __shared__ float red[6][4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t r0 = row0[c], n64 = len[c];
    const int n = (r0 >= 0 && n64 >= 0 && n64 <= max_len && r0 + n64 <= rows) ? (int)n64 : 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = t; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float a = dsm[(r0 + i) * 3 + k], b = dem[(r0 + i) * 3 + k];
            lo[k] = fminf(lo[k], fminf(a, b));
            hi[k] = fmaxf(hi[k], fmaxf(a, b));
        }
    block_bounds<3>(lo, hi, red);
    if (t >= 3) return;
    float a, b;
    bounds_of<3>(red, t, a, b);
    centre[c * 3 + t] = n > 0 ? (a + b) / 2.0f : 0.0f;
}

// grid (ceil(max_len / 256), n_clouds)
__global__ __launch_bounds__(256) void dsm_rows_kernel(const float* __restrict__ dsm, const float* __restrict__ dem,
                                                      const int32_t* __restrict__ row0, const int32_t* __restrict__ len,
                                                      int32_t max_len, int64_t rows, const float* __restrict__ centre,
                                                      float* __restrict__ out) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int64_t r0 = row0[c], n64 = len[c];
    if (!(r0 >= 0 && n64 >= 0 && n64 <= max_len && r0 + n64 <= rows) || i >= n64) return;
    const int64_t row = r0 + i;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float m = centre[c * 3 + k];
        out[row * 6 + k] = dsm[row * 3 + k] - m;
        out[row * 6 + 3 + k] = dem[row * 3 + k] - m;
    }
}

}  // namespace

extern "C" int64_t scream_dsm_workspace_bytes(int64_t patch_rows_total, int32_t n_clouds, int32_t max_p_len) {
    if (n_clouds < 0 || !rows_ok(patch_rows_total, max_p_len)) return SCREAM_EINVAL;
    return grid_carve<2>(nullptr, patch_rows_total, n_clouds, grid_side(max_p_len)).bytes;
}

extern "C" int scream_dsm_extract(const float* patch, const int32_t* p_row0, const int32_t* p_len, int32_t max_p_len,
                                  int64_t patch_rows_total, const float* dem, const int32_t* d_row0, const int32_t* d_len,
                                  int32_t max_d_len, int64_t dem_rows_total, int32_t n_clouds, float radius, float* out_xyz,
                                  int32_t* out_idx, void* workspace, int64_t workspace_bytes_given, void* stream) {
    SCREAM_REQUIRE(radius > 0.0f && isfinite(radius), SCREAM_EINVAL);
    SCREAM_REQUIRE(n_clouds >= 0 && rows_ok(patch_rows_total, max_p_len) && rows_ok(dem_rows_total, max_d_len), SCREAM_EINVAL);
    if (n_clouds == 0) return 0;
    SCREAM_REQUIRE(n_clouds <= 65535, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(patch && p_row0 && p_len && dem && d_row0 && d_len && out_xyz && out_idx && workspace, SCREAM_EINVAL);
    const int side = grid_side(max_p_len);
    const GridWs<2> ws = grid_carve<2>(workspace, patch_rows_total, n_clouds, side);
    SCREAM_REQUIRE(workspace_bytes_given >= ws.bytes, SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(workspace), SCREAM_EINVAL);
    const double R = (double)radius;
    hipStream_t st = as_stream(stream);
    const int rc = cell_grid_enqueue<2>(patch, p_row0, p_len, max_p_len, patch_rows_total, d_row0, d_len, max_d_len, dem_rows_total, n_clouds,
                                        R, DSM_EDGE_SLACK, side, ws, st);
    if (rc != 0) return rc;
    if (max_d_len > 0) {
        dsm_query_kernel<<<dim3(row_blocks(max_d_len), n_clouds), dim3(256), 0, st>>>(dem, ws.plan, side, ws.cells, ws.recs, R,
                                                                                        out_xyz, out_idx);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int scream_dsm_dem_assemble(const float* dsm, const float* dem, const int32_t* row0, const int32_t* len, int32_t n_clouds,
                                       int32_t max_len, int64_t rows_total, float* out, float* centre, void* stream) {
    SCREAM_REQUIRE(n_clouds >= 0 && rows_ok(rows_total, max_len), SCREAM_EINVAL);
    if (n_clouds == 0) return 0;
    SCREAM_REQUIRE(n_clouds <= 65535, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(dsm && dem && row0 && len && out && centre, SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    dsm_centre_kernel<<<dim3(n_clouds), dim3(256), 0, st>>>(dsm, dem, row0, len, max_len, rows_total, centre);
    SCREAM_LAUNCH_CHECK();
    if (max_len > 0) {
        dsm_rows_kernel<<<dim3(row_blocks(max_len), n_clouds), dim3(256), 0, st>>>(dsm, dem, row0, len, max_len, rows_total, centre,
                                                                                     out);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}
