// A dense uniform grid over one cloud of every pair of a packed call, built by a counting sort: the candidate filter of dsm.hip
// (D = 2: the xy plane) and radius.hip (D = 3).  One cloud of the pair is BINNED (the DSM's patch, the search's target), the
// other one QUERIES it.  Everything lives in an anonymous namespace: each file that includes this gets its own kernels.
// Compile with -ffp-contract=off.
//
// Per pair, over the exact fp32 bounds of its binned cloud on the first D axes:
//   cell edge h = max(R * edge_slack, largest extent / side), at most side^D cells (`side` is fixed per call by the op, from the
//   call's longest binned cloud) -- a large extent makes the cells larger, never refuses the cloud;
//   cell_k(v) = clamp(floor((v - origin_k) * (1 / h)), 0, n_k - 1), evaluated in float64 (cell_of below) for the coordinates of
//   BOTH clouds (an fp32 coordinate converts exactly), every step monotone non-decreasing in v.
// The grid only filters: an op's result must not depend on it.  That holds for a query that scans, per axis, the cells
//   cell(lo) .. cell(hi)   with float64 lo <= b_k <= hi for every binned point b its predicate accepts,
// because cell() is the SAME monotone function for both clouds: cell(lo) <= cell(b_k) <= cell(hi) whatever the rounding inside
// cell() itself.  That is why a querying point's cell must not come from a different (say fp32) expression than a binned
// point's: two functions that round differently may disagree about a point on a cell border.  Each op's file proves only the
// step that is its own: that its lo / hi enclose what its predicate accepts.
// h >= R (1 + 2^-10) bounds a scanned range of reach R (1 + 2^-20) at most on either side by three cells per axis: lo and hi
// differ by less than 2 - 2^-10 cell edges, and the float64 roundings of the sums and inside cell() move an unclamped value
// (|value| <= side + 2 <= 130 near the grid; everything beyond clamps to the same border cell) by less than 2^-40.
// The clamp keeps a query outside the binned cloud's bounding box on the border cells: beyond reach its runs hold nobody who
// passes the predicate, just outside it still meets the border cells' points.
//
//   plan     rows checked against the arrays, fp32 bounds of the binned cloud, grid origin / edge / dimensions: block (pair, 0).
//            The launch also ZEROES the counters, for both ops the same way: a pair has one block per 16 KiB of its side^D
//            counters (1 .. 64 blocks), each clears its share with 16-byte stores, and block 0 goes on to plan.  Not a
//            hipMemsetAsync in front: that is one more node per call, and on the MI355X it cost the DSM's packed call 0.4 us
//            at one window and 1 - 2 us at 64, its public call 3 us at one window (profiles/cell_grid_ab.json,
//            "memset_variant"); nor one block per pair looping over up to 1 MiB.
//   count    one thread per binned row: integer atomic on its cell's counter
//   scan     one block per pair: exclusive scan of the counters in place.  Cell order (z * ny + y) * nx + x (D = 2: nz = 1, i.e.
//            y * nx + x), so the cells of one grid row that a query touches are ONE contiguous run of records
//   scatter  one thread per binned row: record {x, y, z, row} at the cell's cursor; afterwards the counter of cell c holds the
//            END of cell c, i.e. the start of cell c + 1 -- one array serves as cursor and as cell table
// No floating-point atomics; the integer atomics only decide the order of the records INSIDE a cell, which no result may depend
// on.  Non-finite coordinates are outside the contract; every cell index goes through a clamp that maps NaN to 0 and every
// store is bounded by the cloud's length, so such input -- or a workspace that held anything -- cannot fault or hang.
#pragma once
#include <math.h>

#include "common.h"

namespace {

template <int D>
struct GridPlan {
    double o[D], inv_h;
    int32_t n[3];            // cells per axis; n[k] = 1 for k >= D
    int32_t b_row0, b_len;   // the binned cloud's rows.  All four are 0 for a pair whose rows leave the arrays: such a pair
    int32_t q_row0, q_len;   // reads and writes nothing
};
static_assert(sizeof(GridPlan<2>) == 56 && sizeof(GridPlan<3>) == 64, "plan layout");

template <int D>
struct GridWs {
    GridPlan<D>* plan;
    int32_t* cells;  // [n_pairs][side^D]
    f32x4* recs;     // [b_rows] records in cell order, per pair from its own first binned row
    int64_t cells_per_pair;
    int64_t bytes;   // of the whole workspace
};
template <int D>
inline GridWs<D> grid_carve(void* workspace, int64_t b_rows, int32_t n_pairs, int side) {
    Carver cv{workspace};
    GridWs<D> w;
    w.cells_per_pair = D == 2 ? (int64_t)side * side : (int64_t)side * side * side;
    w.plan = cv.take<GridPlan<D>>(n_pairs);
    w.cells = cv.take<int32_t>(n_pairs * w.cells_per_pair);
    w.recs = cv.take<f32x4>(b_rows);
    w.bytes = cv.used;
    return w;
}

// floor(v) clamped to [0, n - 1]; NaN -> 0.  Monotone non-decreasing in v.
__device__ __forceinline__ int clamp_cell(double v, int n) {
    double c = floor(v);
    c = c >= 0.0 ? c : 0.0;
    c = c <= (double)(n - 1) ? c : (double)(n - 1);
    return (int)c;
}
// THE cell coordinate on axis k, of binned and querying points alike
template <int D>
__device__ __forceinline__ int cell_of(const GridPlan<D>& p, int k, double v) { return clamp_cell((v - p.o[k]) * p.inv_h, p.n[k]); }

// the cell of a binned row
template <int D>
__device__ __forceinline__ int cell_index(const GridPlan<D>& p, const float* __restrict__ v) {
    int c = cell_of(p, D - 1, (double)v[D - 1]);
#pragma unroll
    for (int k = D - 2; k >= 0; --k) c = c * p.n[k] + cell_of(p, k, (double)v[k]);
    return c;
}

// Block-wide (256 threads) fp32 bounds of A axes: every thread brings the bounds of its own rows; afterwards, for every thread,
// red[k][w] / red[A + k][w] are wave w's bounds of axis k (bounds_of folds the four).  Min and max do not depend on the order.
template <int A>
__device__ __forceinline__ void block_bounds(float (&lo)[A], float (&hi)[A], float (*red)[4]) {
    const int t = threadIdx.x;
    for (int m = 1; m < 64; m <<= 1)
#pragma unroll
        for (int k = 0; k < A; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], m));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m));
        }
    if ((t & 63) == 0)
#pragma unroll
        for (int k = 0; k < A; ++k) {
            red[k][t >> 6] = lo[k];
            red[A + k][t >> 6] = hi[k];
        }
    __syncthreads();
}
template <int A>
__device__ __forceinline__ void bounds_of(const float (*red)[4], int k, float& lo, float& hi) {
    lo = red[k][0];
    hi = red[A + k][0];
    for (int w = 1; w < 4; ++w) {
        lo = fminf(lo, red[k][w]);
        hi = fmaxf(hi, red[A + k][w]);
    }
}

// grid (n_pairs, zero_blocks), block 256
template <int D>
__global__ __launch_bounds__(256) void grid_plan_kernel(const float* __restrict__ pts, const int32_t* __restrict__ b_row0,
                                                       const int32_t* __restrict__ b_len, const int32_t* __restrict__ q_row0,
                                                       const int32_t* __restrict__ q_len, int32_t max_b_len, int32_t max_q_len,
                                                       int64_t b_rows, int64_t q_rows, double R, double edge_slack, int side,
                                                       GridPlan<D>* __restrict__ plan, int64_t cells_per_pair,
                                                       int32_t* __restrict__ cells) {
    __shared__ float red[2 * D][4];
    const int c = blockIdx.x, t = threadIdx.x;
    // cells_per_pair is a multiple of 16 (side >= 4, a power of two) and the table starts at a multiple of 256 bytes
    int4* zero = reinterpret_cast<int4*>(cells + (int64_t)c * cells_per_pair);
    for (int64_t i = (int64_t)blockIdx.y * 256 + t; i < cells_per_pair / 4; i += (int64_t)gridDim.y * 256) zero[i] = make_int4(0, 0, 0, 0);
    if (blockIdx.y != 0) return;
    const int64_t br = b_row0[c], bn = b_len[c], qr = q_row0[c], qn = q_len[c];
    const bool ok = br >= 0 && bn >= 0 && bn <= max_b_len && br + bn <= b_rows && qr >= 0 && qn >= 0 && qn <= max_q_len &&
                    qr + qn <= q_rows;
    const int n = ok ? (int)bn : 0;
    float lo[D], hi[D];
#pragma unroll
    for (int k = 0; k < D; ++k) lo[k] = INFINITY, hi[k] = -INFINITY;
    for (int i = t; i < n; i += 256)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const float v = pts[(br + i) * 3 + k];
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    block_bounds<D>(lo, hi, red);
    if (t != 0) return;
    GridPlan<D> p = {};
    p.b_row0 = ok ? (int32_t)br : 0;
    p.b_len = n;
    p.q_row0 = ok ? (int32_t)qr : 0;
    p.q_len = ok ? (int32_t)qn : 0;
    p.n[0] = p.n[1] = p.n[2] = 1;
    p.inv_h = 0.0;
    if (n > 0) {
        double e[D], h = R * edge_slack;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            bounds_of<D>(red, k, lo[k], hi[k]);
            e[k] = (double)hi[k] - (double)lo[k];  // exact
            h = fmax(h, e[k] / (double)side);
            p.o[k] = (double)lo[k];
        }
        p.inv_h = 1.0 / h;
        // the largest coordinate has the largest cell (cell_of is monotone): no binned point lies beyond n[k] even without the clamp
#pragma unroll
        for (int k = 0; k < D; ++k) p.n[k] = clamp_cell(e[k] * p.inv_h, side) + 1;
    }
    plan[c] = p;
}

// grid (ceil(max_b_len / 256), n_pairs)
template <int D>
__global__ __launch_bounds__(256) void grid_count_kernel(const float* __restrict__ pts, const GridPlan<D>* __restrict__ plan,
                                                        int64_t cells_per_pair, int32_t* __restrict__ cells) {
    const GridPlan<D>& p = plan[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.b_len) return;
    const int64_t row = (int64_t)p.b_row0 + i;
    atomicAdd(&cells[(int64_t)blockIdx.y * cells_per_pair + cell_index(p, pts + row * 3)], 1);
}

// grid n_pairs, block 1024: in-place exclusive scan of the pair's nx * ny * nz counters
template <int D>
__global__ __launch_bounds__(1024) void grid_scan_kernel(const GridPlan<D>* __restrict__ plan, int64_t cells_per_pair,
                                                        int32_t* __restrict__ cells) {
    __shared__ int32_t part[1024];
    const GridPlan<D>& p = plan[blockIdx.x];
    const int t = threadIdx.x;
    int32_t* c = cells + (int64_t)blockIdx.x * cells_per_pair;
    const int n = p.n[0] * p.n[1] * p.n[2], chunk = (n + 1023) / 1024;
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

// grid (ceil(max_b_len / 256), n_pairs): afterwards cells[c] = end of cell c
template <int D>
__global__ __launch_bounds__(256) void grid_scatter_kernel(const float* __restrict__ pts, const GridPlan<D>* __restrict__ plan,
                                                          int64_t cells_per_pair, int32_t* __restrict__ cells,
                                                          f32x4* __restrict__ recs) {
    const GridPlan<D>& p = plan[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.b_len) return;
    const int64_t row = (int64_t)p.b_row0 + i;
    const float x = pts[row * 3 + 0], y = pts[row * 3 + 1], z = pts[row * 3 + 2];
    const float v[3] = {x, y, z};
    const int pos = atomicAdd(&cells[(int64_t)blockIdx.y * cells_per_pair + cell_index(p, v)], 1);
    if (pos >= 0 && pos < p.b_len) {  // always, for counters that match the rows
        f32x4 r = {x, y, z, __int_as_float(i)};
        recs[(int64_t)p.b_row0 + pos] = r;
    }
}

// plan (which zeroes), count, scan, scatter on the stream; n_pairs >= 1.  Returns 0 or the HIP error.
template <int D>
inline int cell_grid_enqueue(const float* pts, const int32_t* b_row0, const int32_t* b_len, int32_t max_b_len, int64_t b_rows,
                             const int32_t* q_row0, const int32_t* q_len, int32_t max_q_len, int64_t q_rows, int32_t n_pairs, double R,
                             double edge_slack, int side, const GridWs<D>& w, hipStream_t st) {
    SCREAM_REQUIRE(w.cells_per_pair % 4 == 0, SCREAM_EINVAL);  // the 16-byte stores of the zeroing
    const unsigned zero_blocks = (unsigned)(w.cells_per_pair * 4 <= 16384 ? 1 : w.cells_per_pair * 4 >= 64 * 16384 ? 64 : w.cells_per_pair * 4 / 16384);
    grid_plan_kernel<D><<<dim3(n_pairs, zero_blocks), dim3(256), 0, st>>>(pts, b_row0, b_len, q_row0, q_len, max_b_len, max_q_len, b_rows,
                                                                          q_rows, R, edge_slack, side, w.plan, w.cells_per_pair, w.cells);
    SCREAM_LAUNCH_CHECK();
    if (max_b_len > 0) {
        const dim3 per_row(row_blocks(max_b_len), n_pairs);
        grid_count_kernel<D><<<per_row, dim3(256), 0, st>>>(pts, w.plan, w.cells_per_pair, w.cells);
        SCREAM_LAUNCH_CHECK();
        grid_scan_kernel<D><<<dim3(n_pairs), dim3(1024), 0, st>>>(w.plan, w.cells_per_pair, w.cells);
        SCREAM_LAUNCH_CHECK();
        grid_scatter_kernel<D><<<per_row, dim3(256), 0, st>>>(pts, w.plan, w.cells_per_pair, w.cells, w.recs);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace
