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
// The grid is a candidate filter only.  Per cloud, a uniform 2-D grid over the exact fp32 xy bounds of its patch:
//   cell edge h = max(R * DSM_EDGE_SLACK, extent_x / side, extent_y / side), side^2 <= DSM_GRID_CELLS cells per cloud (side is
//   fixed per call from max_p_len: about one cell per row of the call's largest patch, so small clouds get small tables) --
//   a large extent makes the cells larger, never refuses the cloud;
//   cell(x) = clamp(floor((float64(x) - origin) * (1 / h)), 0, n - 1), every step monotone non-decreasing in x.
// A query scans the cells  cell(q - Rs) .. cell(q + Rs)  per axis, Rs = R * (1 + 2^-20).  Conservative because: a candidate has
// |float32(p.x - q.x)| <= R, so |p.x - q.x| <= R (1 + 2^-24) in real numbers (half an fp32 ulp of R at most, R being an fp32
// value); q.x + Rs rounded to float64 is then still >= p.x (the slack R (2^-20 - 2^-24) is far above a float64 ulp of any fp32
// coordinate whose fp32 difference to q.x could be as small as R), and cell() is monotone, so cell(p.x) lies inside the scanned
// range whatever the rounding of the cell computation itself.  The clamp keeps queries outside the patch's bounds on the
// border cells, as cell_coord does in icp_grid.h.
//
//   plan     one block per cloud: rows checked against the arrays, fp32 xy bounds of the patch, grid origin / edge / dimensions,
//            the cloud's cell counters zeroed
//   count    one thread per patch row: integer atomic on its cell's counter
//   scan     one block per cloud: exclusive scan of the counters in place (cell order: y * nx + x, so the cells of one grid row
//            that a query touches are ONE contiguous run of records)
//   scatter  one thread per patch row: record {x, y, z, row} at the cell's cursor; afterwards the counter of cell c holds the END
//            of cell c, i.e. the start of cell c + 1 -- one array serves as cursor and as cell table
//   query    one thread per ground point: at most three runs of records (one per grid row), candidates tested four at a time
//   assemble (second entry point) per-cloud fp32 min / max over dsm and dem rows, centre = float32(min + max) / 2, rows
//            float32(dsm - centre) | float32(dem - centre)
// A lone 100 m window is ~10^4 queries = 40 blocks on 256 CUs: latency-bound whatever the block shape.  The design point is the
// batched call (64 windows: 2 500 blocks of 256 queries, ten waves per SIMD's worth of independent loads).
// Non-finite coordinates are outside the contract; every cell index goes through a clamp that maps NaN to 0, every loop is
// bounded by the scanned counters, so such input cannot fault or hang.
#include <math.h>

#include "common.h"

namespace {

constexpr int DSM_GRID_CELLS = 1 << 14;    // cells per cloud at most (128 x 128: a 100 m window at the 0.8 m radius has 125 x 125)
constexpr int DSM_MAX_SIDE = 128;
constexpr int DSM_MIN_SIDE = 8;
constexpr double DSM_EDGE_SLACK = 1.0 + 1.0 / 1024.0;       // cell edge >= R * this: a disc touches at most 3 cells per axis
constexpr double DSM_REACH_SLACK = 1.0 + 1.0 / 1048576.0;   // Rs = R * this (see the header of this file)
static_assert(DSM_MAX_SIDE * DSM_MAX_SIDE <= DSM_GRID_CELLS, "grid cap");

struct DsmPlan {
    double ox, oy, inv_h;
    int32_t nx, ny;
    int32_t p_row0, p_len;  // both 0 for a cloud whose rows are outside the arrays: such a cloud writes nothing
    int32_t d_row0, d_len;
    int32_t pad[2];
};

inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

// cells per axis of every cloud of a call: about one cell per patch row
inline int grid_side(int32_t max_p_len) {
    int s = DSM_MIN_SIDE;
    while (s < DSM_MAX_SIDE && (int64_t)s * s < (int64_t)max_p_len) s *= 2;
    return s;
}

struct Carve {
    DsmPlan* plan;
    int32_t* cells;  // [n_clouds][side * side]
    f32x4* recs;     // [p_rows] records in cell order, per cloud from its own first patch row
};
inline int64_t workspace_bytes(int64_t p_rows, int32_t n_clouds, int32_t max_p_len) {
    const int64_t side = grid_side(max_p_len);
    return align256((int64_t)n_clouds * (int64_t)sizeof(DsmPlan)) + align256((int64_t)n_clouds * side * side * 4) +
           align256(p_rows * 16);
}
inline Carve carve(void* workspace, int64_t p_rows, int32_t n_clouds, int32_t max_p_len) {
    char* w = reinterpret_cast<char*>(workspace);
    auto take = [&](int64_t bytes) { char* r = w; w += align256(bytes); return r; };
    const int64_t side = grid_side(max_p_len);
    Carve c;
    c.plan = reinterpret_cast<DsmPlan*>(take((int64_t)n_clouds * (int64_t)sizeof(DsmPlan)));
    c.cells = reinterpret_cast<int32_t*>(take((int64_t)n_clouds * side * side * 4));
    c.recs = reinterpret_cast<f32x4*>(take(p_rows * 16));
    return c;
}

// floor(v) clamped to [0, n - 1]; NaN -> 0.  Monotone non-decreasing in v.
__device__ __forceinline__ int clamp_cell(double v, int n) {
    double c = floor(v);
    c = c >= 0.0 ? c : 0.0;
    c = c <= (double)(n - 1) ? c : (double)(n - 1);
    return (int)c;
}
__device__ __forceinline__ int cell_x(const DsmPlan& p, double x) { return clamp_cell((x - p.ox) * p.inv_h, p.nx); }
__device__ __forceinline__ int cell_y(const DsmPlan& p, double y) { return clamp_cell((y - p.oy) * p.inv_h, p.ny); }

// grid n_clouds, block 256
__global__ __launch_bounds__(256) void dsm_plan_kernel(const float* __restrict__ patch, const int32_t* __restrict__ p_row0,
                                                      const int32_t* __restrict__ p_len, const int32_t* __restrict__ d_row0,
                                                      const int32_t* __restrict__ d_len, int32_t max_p_len, int32_t max_d_len,
                                                      int64_t p_rows, int64_t d_rows, double R, int side,
                                                      DsmPlan* __restrict__ plan, int32_t* __restrict__ cells) {
    __shared__ float red[4][4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int64_t pr = p_row0[c], pn = p_len[c], dr = d_row0[c], dn = d_len[c];
    const bool ok = pr >= 0 && pn >= 0 && pn <= max_p_len && pr + pn <= p_rows && dr >= 0 && dn >= 0 && dn <= max_d_len &&
                    dr + dn <= d_rows;
    const int n = ok ? (int)pn : 0;
    int32_t* cell = cells + (int64_t)c * side * side;
    for (int i = t; i < side * side; i += 256) cell[i] = 0;
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    for (int i = t; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float v = patch[(pr + i) * 3 + k];
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], m));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m));
        }
    if ((t & 63) == 0)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            red[k][t >> 6] = lo[k];
            red[2 + k][t >> 6] = hi[k];
        }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            lo[k] = fminf(lo[k], red[k][w]);
            hi[k] = fmaxf(hi[k], red[2 + k][w]);
        }
    DsmPlan p = {};
    p.p_row0 = ok ? (int32_t)pr : 0;
    p.p_len = n;
    p.d_row0 = ok ? (int32_t)dr : 0;
    p.d_len = ok ? (int32_t)dn : 0;
    p.nx = p.ny = 1;
    p.inv_h = 0.0;
    if (n > 0) {
        const double ex = (double)hi[0] - (double)lo[0], ey = (double)hi[1] - (double)lo[1];  // exact
        double h = R * DSM_EDGE_SLACK;
        h = fmax(h, fmax(ex, ey) / (double)side);
        p.ox = (double)lo[0];
        p.oy = (double)lo[1];
        p.inv_h = 1.0 / h;
        // the largest coordinate has the largest cell (cell() is monotone): no point lies beyond nx, ny even without the clamp
        p.nx = clamp_cell(ex * p.inv_h, side) + 1;
        p.ny = clamp_cell(ey * p.inv_h, side) + 1;
    }
    plan[c] = p;
}

// grid (ceil(max_p_len / 256), n_clouds)
__global__ __launch_bounds__(256) void dsm_count_kernel(const float* __restrict__ patch, const DsmPlan* __restrict__ plan, int side,
                                                       int32_t* __restrict__ cells) {
    const DsmPlan& p = plan[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.p_len) return;
    const int64_t row = (int64_t)p.p_row0 + i;
    const int cx = cell_x(p, (double)patch[row * 3 + 0]), cy = cell_y(p, (double)patch[row * 3 + 1]);
    atomicAdd(&cells[(int64_t)blockIdx.y * side * side + cy * p.nx + cx], 1);
}

// grid n_clouds, block 1024: in-place exclusive scan of the cloud's nx * ny counters
__global__ __launch_bounds__(1024) void dsm_scan_kernel(const DsmPlan* __restrict__ plan, int side, int32_t* __restrict__ cells) {
    __shared__ int32_t part[1024];
    const DsmPlan& p = plan[blockIdx.x];
    const int t = threadIdx.x;
    int32_t* c = cells + (int64_t)blockIdx.x * side * side;
    const int n = p.nx * p.ny, chunk = (n + 1023) / 1024;
    const int b = min(n, t * chunk), e = min(n, b + chunk);
    int32_t s = 0;
    for (int i = b; i < e; ++i) s += c[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int32_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int32_t run = part[t] - s;
    for (int i = b; i < e; ++i) {
        const int32_t v = c[i];
        c[i] = run;
        run += v;
    }
}

// grid (ceil(max_p_len / 256), n_clouds): afterwards cells[c] = end of cell c
__global__ __launch_bounds__(256) void dsm_scatter_kernel(const float* __restrict__ patch, const DsmPlan* __restrict__ plan, int side,
                                                         int32_t* __restrict__ cells, f32x4* __restrict__ recs) {
    const DsmPlan& p = plan[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.p_len) return;
    const int64_t row = (int64_t)p.p_row0 + i;
    const float x = patch[row * 3 + 0], y = patch[row * 3 + 1], z = patch[row * 3 + 2];
    const int cx = cell_x(p, (double)x), cy = cell_y(p, (double)y);
    const int pos = atomicAdd(&cells[(int64_t)blockIdx.y * side * side + cy * p.nx + cx], 1);
    if (pos >= 0 && pos < p.p_len) {  // always, for counters that match the rows
        f32x4 r = {x, y, z, __int_as_float(i)};
        recs[(int64_t)p.p_row0 + pos] = r;
    }
}

// grid (ceil(max_d_len / 256), n_clouds)
__global__ __launch_bounds__(256) void dsm_query_kernel(const float* __restrict__ dem, const DsmPlan* __restrict__ plan, int side,
                                                       const int32_t* __restrict__ cells, const f32x4* __restrict__ recs,
                                                       double R, float* __restrict__ out_xyz, int32_t* __restrict__ out_idx) {
    const DsmPlan& p = plan[blockIdx.y];
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= p.d_len) return;
    const int64_t qrow = (int64_t)p.d_row0 + qi;
    const float qx = dem[qrow * 3 + 0], qy = dem[qrow * 3 + 1], qz = dem[qrow * 3 + 2];
    const double R2 = R * R, Rs = R * DSM_REACH_SLACK;
    float bx = qx, by = qy, bz = qz;
    int bi = -1;
    if (p.p_len > 0) {
        const int32_t* cell = cells + (int64_t)blockIdx.y * side * side;
        const f32x4* rec = recs + p.p_row0;
        const int x0 = cell_x(p, (double)qx - Rs), x1 = cell_x(p, (double)qx + Rs);
        const int y0 = cell_y(p, (double)qy - Rs), y1 = cell_y(p, (double)qy + Rs);
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
            const int c0 = y * p.nx + x0, c1 = y * p.nx + x1;
            int j = c0 > 0 ? cell[c0 - 1] : 0, je = cell[c1];
            j = max(j, 0);
            je = min(je, p.p_len);
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
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], m));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m));
        }
    if ((t & 63) == 0)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            red[k][t >> 6] = lo[k];
            red[3 + k][t >> 6] = hi[k];
        }
    __syncthreads();
    if (t >= 3) return;
    float a = red[t][0], b = red[3 + t][0];
    for (int w = 1; w < 4; ++w) {
        a = fminf(a, red[t][w]);
        b = fmaxf(b, red[3 + t][w]);
    }
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

inline unsigned row_blocks(int32_t max_len) { return (unsigned)(((int64_t)max_len + 255) / 256); }
inline bool rows_ok(int64_t rows, int32_t max_len) { return rows >= 0 && rows <= INT32_MAX && max_len >= 0 && max_len <= rows; }

}  // namespace

extern "C" int64_t scream_dsm_workspace_bytes(int64_t patch_rows_total, int32_t n_clouds, int32_t max_p_len) {
    if (n_clouds < 0 || !rows_ok(patch_rows_total, max_p_len)) return SCREAM_EINVAL;
    return workspace_bytes(patch_rows_total, n_clouds, max_p_len);
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
    SCREAM_REQUIRE(workspace_bytes_given >= workspace_bytes(patch_rows_total, n_clouds, max_p_len), SCREAM_EINVAL);
    SCREAM_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, SCREAM_EINVAL);
    const Carve cv = carve(workspace, patch_rows_total, n_clouds, max_p_len);
    const int side = grid_side(max_p_len);
    const double R = (double)radius;
    hipStream_t st = as_stream(stream);
    dsm_plan_kernel<<<dim3(n_clouds), dim3(256), 0, st>>>(patch, p_row0, p_len, d_row0, d_len, max_p_len, max_d_len, patch_rows_total,
                                                          dem_rows_total, R, side, cv.plan, cv.cells);
    SCREAM_LAUNCH_CHECK();
    if (max_p_len > 0) {
        const dim3 per_row(row_blocks(max_p_len), n_clouds);
        dsm_count_kernel<<<per_row, dim3(256), 0, st>>>(patch, cv.plan, side, cv.cells);
        SCREAM_LAUNCH_CHECK();
        dsm_scan_kernel<<<dim3(n_clouds), dim3(1024), 0, st>>>(cv.plan, side, cv.cells);
        SCREAM_LAUNCH_CHECK();
        dsm_scatter_kernel<<<per_row, dim3(256), 0, st>>>(patch, cv.plan, side, cv.cells, cv.recs);
        SCREAM_LAUNCH_CHECK();
    }
    if (max_d_len > 0) {
        dsm_query_kernel<<<dim3(row_blocks(max_d_len), n_clouds), dim3(256), 0, st>>>(dem, cv.plan, side, cv.cells, cv.recs, R,
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
