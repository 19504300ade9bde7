// voxel_down_sample for a batch of packed clouds: open3d's legacy voxel_down_sample as scream_amd/evaluate_open_gf.py restates
// it (process_3d_match.py:30-32, process_kitti.py:55-56, datasets/kitti.py:137-138, datasets/open_gf.py:22,42,62).
//
// Per cloud: origin = min_bound - voxel / 2; voxel index per axis = floor((p - origin) / voxel) in float64 from the fp32
// coordinate (a real division); one output row per occupied voxel = the float64 sum of its points in ASCENDING ORIGINAL ROW
// INDEX, divided in float64 by the count, rounded once to fp32; output rows in ascending (i, j, k), i most significant (the
// order of np.unique(axis=0)).  Every rule is a fixed IEEE sequence, so the result is a pure function of the cloud: bitwise
// repeatable, independent of the other clouds of the launch, and equal bit for bit to a float64 numpy restatement
// (tests/voxel_ref.py).  No floating-point atomics; the integer atomics below (LDS histograms, head counts) are sums whose
// value does not depend on the arrival order.  This file is compiled with -ffp-contract=off.
//
// Dense counting grids (icp_grid.hip) do not fit: a KITTI extent at 0.3 m is tens of millions of cells.  Instead:
//   plan     one block: validates row0 / len of every cloud and lays its VX_TILE-row blocks out in the shared count tables
//   bounds   one block per cloud: exact fp32 min / max per axis, non-finite check, grid origin, the bit width of each axis'
//            largest index and from them the cloud's key layout  key = i << (bj + bk) | j << bk | k  and its number of 8-bit
//            passes -- decided HERE, on the device: the host launches all VX_MAX_PASSES and a cloud's blocks leave at once in
//            the passes it does not need (a cloud with 1000 cells per axis sorts in 4 passes, not 8)
//   keys     (key, row) per point
//   sort     stable LSD radix sort of the pairs inside each cloud, 8 bits per pass: block histograms -> exclusive scan over
//            (digit, block) -> scatter with wave-level ranks (a lane's rank among the lanes of its wave with the same digit
//            comes from eight ballots).  Rows start in index order and every pass is stable, so the row index is the tie-break.
//   heads    run-head flags (key != previous key), counted per block, scanned per cloud, then every head writes its sorted
//            position at its ordinal; the number of heads is the cloud's output length
//   centroid one thread per run sums its rows serially in float64
// A cloud whose grid needs more than 2^21 cells on an axis, that holds a non-finite coordinate or whose voxel is not a
// positive finite number -- and one whose rows do not fit what the caller declared -- gets length -1 and no rows; the
// other clouds of the launch are unaffected.
#include <math.h>

#include "common.h"
#include "voxel_sort.h"  // plan, bounds, keys, the segmented radix sort and the run heads: shared with icp_raw.hip

namespace {

// grid (ceil(max_len / 256), n_clouds): one thread per run; float64 sums in sorted order = ascending original row
__global__ __launch_bounds__(256) void voxel_centroid_kernel(const float* __restrict__ xyz, const CloudPlan* __restrict__ plan,
                                                            const int32_t* __restrict__ rows0, const int32_t* __restrict__ rows1,
                                                            const int32_t* __restrict__ start, float* __restrict__ out_xyz,
                                                            int32_t* __restrict__ out_count) {
    const CloudPlan& p = plan[blockIdx.y];
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (p.status || m >= p.n_out) return;
    const int32_t* rows = ((p.npass & 1) ? rows1 : rows0) + p.row0;
    // the clamps cost nothing and keep every address inside the cloud whatever the workspace held
    const int s0 = min(max(start[p.row0 + m], 0), p.len), s1 = min(m + 1 < p.n_out ? start[p.row0 + m + 1] : p.len, p.len);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int s = s0; s < s1; ++s) {
        const int64_t row = (int64_t)p.row0 + min(max(rows[s], 0), p.len - 1);
        sx += (double)xyz[row * 3 + 0];
        sy += (double)xyz[row * 3 + 1];
        sz += (double)xyz[row * 3 + 2];
    }
    const double cnt = (double)(s1 - s0);
    const int64_t o = (int64_t)p.row0 + m;
    out_xyz[o * 3 + 0] = (float)(sx / cnt);
    out_xyz[o * 3 + 1] = (float)(sy / cnt);
    out_xyz[o * 3 + 2] = (float)(sz / cnt);
    if (out_count) out_count[o] = s1 - s0;
}

}  // namespace

extern "C" int64_t scream_voxel_workspace_bytes(int64_t rows_total, int32_t n_clouds) {
    if (rows_total < 0 || rows_total > INT32_MAX || n_clouds < 0) return SCREAM_EINVAL;
    return voxel_carve_bytes(rows_total, n_clouds);
}

extern "C" int scream_voxel_down_sample(const float* xyz, const int32_t* row0, const int32_t* len, int32_t n_clouds, int32_t max_len,
                                        const double* voxel, float* out_xyz, int32_t* out_len, int32_t* out_count, void* workspace,
                                        int64_t workspace_bytes_given, void* stream) {
    SCREAM_REQUIRE(n_clouds >= 0 && max_len >= 0 && workspace_bytes_given >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(xyz && row0 && len && voxel && out_xyz && out_len && workspace, SCREAM_EINVAL);
    SCREAM_REQUIRE(workspace_bytes_given >= voxel_carve_bytes(max_len, n_clouds), SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(workspace), SCREAM_EINVAL);
    if (n_clouds == 0) return 0;
    SCREAM_REQUIRE(n_clouds <= 65535, SCREAM_EUNSUPPORTED);
    // the rows this workspace was sized for: the largest rows_total whose workspace fits (the size is monotone in rows)
    int64_t rows_cap = max_len, hi = INT32_MAX;
    while (rows_cap < hi) {
        const int64_t mid = rows_cap + (hi - rows_cap + 1) / 2;
        if (voxel_carve_bytes(mid, n_clouds) <= workspace_bytes_given) rows_cap = mid;
        else hi = mid - 1;
    }
    Carver w{workspace};
    const Carve cv = voxel_carve(w, rows_cap, n_clouds);
    hipStream_t st = as_stream(stream);
    const int rc = voxel_sort_enqueue(xyz, row0, len, n_clouds, max_len, voxel, rows_cap, cv, st);
    if (rc != 0) return rc;
    if (max_len > 0) {
        const dim3 per_tile((max_len + VX_TILE - 1) / VX_TILE, n_clouds);
        voxel_heads_count_kernel<<<per_tile, dim3(VX_THREADS), 0, st>>>(cv.plan, cv.keys[0], cv.keys[1], cv.heads);
        SCREAM_LAUNCH_CHECK();
    }
    voxel_heads_scan_kernel<<<dim3(n_clouds), dim3(256), 0, st>>>(cv.plan, cv.heads, out_len);
    SCREAM_LAUNCH_CHECK();
    if (max_len > 0) {
        const dim3 per_row((max_len + 255) / 256, n_clouds), per_tile((max_len + VX_TILE - 1) / VX_TILE, n_clouds);
        voxel_heads_write_kernel<<<per_tile, dim3(VX_THREADS), 0, st>>>(cv.plan, cv.keys[0], cv.keys[1], cv.heads, cv.start);
        SCREAM_LAUNCH_CHECK();
        voxel_centroid_kernel<<<per_row, dim3(256), 0, st>>>(xyz, cv.plan, cv.rows[0], cv.rows[1], cv.start, out_xyz, out_count);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}
