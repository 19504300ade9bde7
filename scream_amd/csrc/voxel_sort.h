// The front half of voxel.hip, shared with icp_raw.hip: the per-cloud plan (row ranges checked, exact bounds, grid origin
// min_bound - voxel / 2, the key layout  key = i << (bj + bk) | j << bk | k  with cell index floor((p - origin) / voxel) per axis
// in float64), the (key, row) pairs, their stable segmented LSD radix sort inside each cloud and the run heads.  voxel.hip's
// header describes every stage; voxel_sort_enqueue() below enqueues plan .. sort.  Everything lives in an anonymous namespace:
// each file that includes this gets its own kernels.  Compile with -ffp-contract=off.
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int VX_THREADS = 256;
constexpr int VX_WAVES = VX_THREADS / 64;
constexpr int VX_ROUNDS = 8;
constexpr int VX_TILE = VX_THREADS * VX_ROUNDS;  // rows per block of the sort and of the head scan
constexpr int VX_MAX_PASSES = 8;                 // 3 x 21 bits in 8-bit digits
constexpr double VX_AXIS_CELLS = 2097152.0;      // 2^21

struct CloudPlan {
    double origin[3];
    double voxel;
    int32_t row0, len;  // len = 0 when status != 0: no kernel below touches a row of such a cloud
    int32_t status;     // 0, or -1: reported as the cloud's output length
    int32_t blk0, nblk;  // the cloud's blocks in the count tables
    int32_t shift_i, shift_j;
    int32_t npass;
    int32_t n_out;
    int32_t bits[3];  // bit width of the largest cell index per axis (i, j, k)
};

struct Carve {
    CloudPlan* plan;
    uint64_t* keys[2];
    int32_t* rows[2];
    int32_t* start;    // sorted position of the head of run m, at row0 + m
    uint32_t* counts;  // per cloud [256][nblk] at blk0 * 256
    int32_t* heads;    // per block
};

inline int64_t blocks_cap(int64_t rows, int32_t n_clouds) { return rows / VX_TILE + n_clouds + 1; }
// THE layout of the sort's buffers, for `rows` rows in `n_clouds` clouds, from wherever `w` stands (voxel.hip: the caller's
// workspace; icp_raw.hip: behind the run's own buffers).  On a Carver with a null base it only measures.
inline Carve voxel_carve(Carver& w, int64_t rows, int32_t n_clouds) {
    Carve c;
    c.plan = w.take<CloudPlan>(n_clouds);
    c.keys[0] = w.take<uint64_t>(rows);
    c.keys[1] = w.take<uint64_t>(rows);
    c.rows[0] = w.take<int32_t>(rows);
    c.rows[1] = w.take<int32_t>(rows);
    c.start = w.take<int32_t>(rows);
    c.counts = w.take<uint32_t>(blocks_cap(rows, n_clouds) * 256);
    c.heads = w.take<int32_t>(blocks_cap(rows, n_clouds));
    return c;
}
inline int64_t voxel_carve_bytes(int64_t rows, int32_t n_clouds) {
    Carver w{nullptr};
    voxel_carve(w, rows, n_clouds);
    return w.used;
}

// grid 1, block 256: every cloud's row range checked against what the host declared (the kernels below trust the plan, not
// the caller's arrays) and its blocks placed in the count tables by a prefix sum over the clouds
__global__ __launch_bounds__(256) void voxel_plan_kernel(const int32_t* __restrict__ row0, const int32_t* __restrict__ len,
                                                        int32_t n_clouds, int32_t max_len, int64_t rows_cap, int64_t blk_cap,
                                                        CloudPlan* __restrict__ plan) {
    __shared__ int64_t part[256];
    const int t = threadIdx.x;
    const int chunk = (n_clouds + 255) / 256;
    const int b = min(n_clouds, t * chunk), e = min(n_clouds, b + chunk);
    auto blocks_of = [&](int c) -> int64_t {
        const int64_t r0 = row0[c], n = len[c];
        return (r0 >= 0 && n >= 0 && n <= max_len && r0 + n <= rows_cap) ? (n + VX_TILE - 1) / VX_TILE : -1;
    };
    int64_t s = 0;
    for (int c = b; c < e; ++c) s += max(blocks_of(c), (int64_t)0);
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int64_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int64_t run = part[t] - s;
    for (int c = b; c < e; ++c) {
        const int64_t nb = blocks_of(c);
        const bool ok = nb >= 0 && run + nb <= blk_cap;  // beyond the table only when clouds overlap
        CloudPlan p = {};
        p.status = ok ? 0 : -1;
        p.row0 = ok ? row0[c] : 0;
        p.len = ok ? len[c] : 0;
        p.blk0 = ok ? (int32_t)run : 0;
        p.nblk = ok ? (int32_t)nb : 0;
        plan[c] = p;
        run += max(nb, (int64_t)0);
    }
}

// grid n_clouds, block 1024
__global__ __launch_bounds__(1024) void voxel_bounds_kernel(const float* __restrict__ xyz, const double* __restrict__ voxel,
                                                           CloudPlan* __restrict__ plan) {
    __shared__ float red[6][16];
    __shared__ int red_bad[16];
    const int c = blockIdx.x, t = threadIdx.x, n = plan[c].len;
    if (n == 0) return;  // empty, or already refused: nothing to bound (uniform over the block)
    const int64_t r0 = plan[c].row0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
    for (int i = t; i < n; i += 1024)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = xyz[(r0 + i) * 3 + k];
            bad |= !isfinite(v);
            lo[k] = fminf(lo[k], v);
            hi[k] = fmaxf(hi[k], v);
        }
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], m));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m));
        }
        bad |= __shfl_xor(bad, m);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            red[k][t >> 6] = lo[k];
            red[3 + k][t >> 6] = hi[k];
        }
        red_bad[t >> 6] = bad;
    }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < 16; ++w) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], red[k][w]);
            hi[k] = fmaxf(hi[k], red[3 + k][w]);
        }
        bad |= red_bad[w];
    }
    const double vx = voxel[c];
    bool ok = !bad && vx > 0.0 && isfinite(vx);
    int bits[3] = {0, 0, 0};
    double origin[3] = {0.0, 0.0, 0.0};
    if (ok)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            origin[k] = (double)lo[k] - vx * 0.5;
            // p -> floor((p - origin) / voxel) never decreases with p: the largest coordinate has the largest index
            const double top = floor(((double)hi[k] - origin[k]) / vx);
            if (!(top >= 0.0 && top < VX_AXIS_CELLS)) ok = false;  // also an overflowed or NaN quotient
            else bits[k] = top == 0.0 ? 0 : 64 - __clzll((long long)top);
        }
    CloudPlan p = plan[c];
    if (!ok) {
        p.status = -1;
        p.len = 0;
        p.nblk = 0;
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) p.origin[k] = origin[k];
        p.voxel = vx;
#pragma unroll
        for (int k = 0; k < 3; ++k) p.bits[k] = bits[k];
        p.shift_j = bits[2];
        p.shift_i = bits[2] + bits[1];
        p.npass = (bits[0] + bits[1] + bits[2] + 7) / 8;
    }
    plan[c] = p;
}

// grid (ceil(max_len / 256), n_clouds)
__global__ __launch_bounds__(256) void voxel_keys_kernel(const float* __restrict__ xyz, const CloudPlan* __restrict__ plan,
                                                        uint64_t* __restrict__ keys, int32_t* __restrict__ rows) {
    const CloudPlan& p = plan[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.len) return;
    const int64_t row = (int64_t)p.row0 + i;
    const double vx = p.voxel;
    const uint64_t ci = (uint64_t)floor(((double)xyz[row * 3 + 0] - p.origin[0]) / vx);
    const uint64_t cj = (uint64_t)floor(((double)xyz[row * 3 + 1] - p.origin[1]) / vx);
    const uint64_t ck = (uint64_t)floor(((double)xyz[row * 3 + 2] - p.origin[2]) / vx);
    keys[row] = (ci << p.shift_i) | (cj << p.shift_j) | ck;
    rows[row] = i;
}

// grid (ceil(max_len / VX_TILE), n_clouds): counts[digit][block] of this pass' digit
__global__ __launch_bounds__(VX_THREADS) void voxel_hist_kernel(const CloudPlan* __restrict__ plan, const uint64_t* __restrict__ keys0,
                                                               const uint64_t* __restrict__ keys1, int pass,
                                                               uint32_t* __restrict__ counts) {
    __shared__ uint32_t h[256];
    const CloudPlan& p = plan[blockIdx.y];
    const int b = blockIdx.x, t = threadIdx.x;
    if (pass >= p.npass || b >= p.nblk) return;
    const uint64_t* keys = ((pass & 1) ? keys1 : keys0) + p.row0;
    h[t] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VX_ROUNDS; ++r) {
        const int i = b * VX_TILE + r * VX_THREADS + t;
        if (i < p.len) atomicAdd(&h[(keys[i] >> (8 * pass)) & 255], 1u);
    }
    __syncthreads();
    counts[(int64_t)p.blk0 * 256 + (int64_t)t * p.nblk + b] = h[t];
}

// grid n_clouds, block 1024: in-place exclusive scan of the cloud's counts in (digit, block) order
__global__ __launch_bounds__(1024) void voxel_scan_kernel(const CloudPlan* __restrict__ plan, int pass, uint32_t* __restrict__ counts) {
    __shared__ uint32_t part[1024];
    const CloudPlan& p = plan[blockIdx.x];
    if (pass >= p.npass) return;
    const int t = threadIdx.x;
    uint32_t* c = counts + (int64_t)p.blk0 * 256;
    const int n = p.nblk * 256, chunk = (n + 1023) / 1024;
    const int b = min(n, t * chunk), e = min(n, b + chunk);
    uint32_t s = 0;
    for (int i = b; i < e; ++i) s += c[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int i = b; i < e; ++i) {
        const uint32_t v = c[i];
        c[i] = run;
        run += v;
    }
}

// grid (ceil(max_len / VX_TILE), n_clouds): stable scatter.  Element order inside a block is (round, wave, lane) = ascending
// position; an element's place is  the scanned start of (digit, block)  +  the same-digit elements of earlier rounds (folded
// into base[] after every round)  +  those of the lower waves of this round (wc[])  +  those of the lower lanes of its wave.
__global__ __launch_bounds__(VX_THREADS) void voxel_scatter_kernel(const CloudPlan* __restrict__ plan, uint64_t* __restrict__ keys0,
                                                                  uint64_t* __restrict__ keys1, int32_t* __restrict__ rows0,
                                                                  int32_t* __restrict__ rows1, int pass,
                                                                  const uint32_t* __restrict__ counts) {
    __shared__ uint32_t base[256];
    __shared__ uint32_t wc[VX_WAVES][256];
    const CloudPlan& p = plan[blockIdx.y];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (pass >= p.npass || b >= p.nblk) return;
    const uint64_t* kin = ((pass & 1) ? keys1 : keys0) + p.row0;
    const int32_t* rin = ((pass & 1) ? rows1 : rows0) + p.row0;
    uint64_t* kout = ((pass & 1) ? keys0 : keys1) + p.row0;
    int32_t* rout = ((pass & 1) ? rows0 : rows1) + p.row0;
    const int len = p.len;
    base[t] = counts[(int64_t)p.blk0 * 256 + (int64_t)t * p.nblk + b];
#pragma unroll
    for (int k = 0; k < VX_WAVES; ++k) wc[k][t] = 0;
    __syncthreads();
    for (int r = 0; r < VX_ROUNDS; ++r) {
        const int i0 = b * VX_TILE + r * VX_THREADS;
        if (i0 >= len) break;  // uniform over the block
        const int i = i0 + t;
        const bool valid = i < len;
        uint64_t key = 0;
        int32_t row = 0;
        if (valid) {
            key = kin[i];
            row = rin[i];
        }
        const uint32_t d = (uint32_t)(key >> (8 * pass)) & 255u;
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const uint64_t m = __ballot(valid && one);
            peers &= one ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wc[w][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = base[d] + rank;
            for (int k = 0; k < w; ++k) pos += wc[k][d];
            if (pos < (uint32_t)len) {  // always, for counts that match the keys
                kout[pos] = key;
                rout[pos] = row;
            }
        }
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < VX_WAVES; ++k) {
            s += wc[k][t];
            wc[k][t] = 0;
        }
        base[t] += s;
        __syncthreads();
    }
}

__device__ __forceinline__ bool run_head(const uint64_t* __restrict__ keys, int i, int len) {
    return i < len && (i == 0 || keys[i] != keys[i - 1]);
}

// grid (ceil(max_len / VX_TILE), n_clouds): run heads per block
__global__ __launch_bounds__(VX_THREADS) void voxel_heads_count_kernel(const CloudPlan* __restrict__ plan,
                                                                      const uint64_t* __restrict__ keys0,
                                                                      const uint64_t* __restrict__ keys1,
                                                                      int32_t* __restrict__ heads) {
    __shared__ int32_t total;
    const CloudPlan& p = plan[blockIdx.y];
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= p.nblk) return;
    const uint64_t* keys = ((p.npass & 1) ? keys1 : keys0) + p.row0;
    if (t == 0) total = 0;
    __syncthreads();
    int32_t n = 0;
#pragma unroll
    for (int r = 0; r < VX_ROUNDS; ++r) n += run_head(keys, b * VX_TILE + r * VX_THREADS + t, p.len);
    for (int m = 1; m < 64; m <<= 1) n += __shfl_xor(n, m);
    if ((t & 63) == 0) atomicAdd(&total, n);
    __syncthreads();
    if (t == 0) heads[p.blk0 + b] = total;
}

// grid n_clouds, block 256: in-place exclusive scan of the cloud's head counts; the total is the cloud's output length
__global__ __launch_bounds__(256) void voxel_heads_scan_kernel(CloudPlan* __restrict__ plan, int32_t* __restrict__ heads,
                                                              int32_t* __restrict__ out_len) {
    __shared__ int32_t part[256];
    CloudPlan& p = plan[blockIdx.x];
    const int t = threadIdx.x;
    int32_t* c = heads + p.blk0;
    const int n = p.nblk, chunk = (n + 255) / 256;
    const int b = min(n, t * chunk), e = min(n, b + chunk);
    int32_t s = 0;
    for (int i = b; i < e; ++i) s += c[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
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
    if (t == 255) {
        p.n_out = part[255];
        out_len[blockIdx.x] = p.status ? -1 : part[255];
    }
}

// grid (ceil(max_len / VX_TILE), n_clouds): the head of run m writes its sorted position to start[row0 + m]
__global__ __launch_bounds__(VX_THREADS) void voxel_heads_write_kernel(const CloudPlan* __restrict__ plan,
                                                                      const uint64_t* __restrict__ keys0,
                                                                      const uint64_t* __restrict__ keys1,
                                                                      const int32_t* __restrict__ heads,
                                                                      int32_t* __restrict__ start) {
    __shared__ int32_t wc[VX_WAVES];
    const CloudPlan& p = plan[blockIdx.y];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (b >= p.nblk) return;
    const uint64_t* keys = ((p.npass & 1) ? keys1 : keys0) + p.row0;
    int32_t* out = start + p.row0;
    int32_t run = heads[p.blk0 + b];
    for (int r = 0; r < VX_ROUNDS; ++r) {
        const int i = b * VX_TILE + r * VX_THREADS + t;
        const bool head = run_head(keys, i, p.len);
        const uint64_t m = __ballot(head);
        if (lane == 0) wc[w] = (int32_t)__popcll(m);
        __syncthreads();
        int32_t ord = run + (int32_t)__popcll(m & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
        for (int k = 0; k < VX_WAVES; ++k) {
            ord += k < w ? wc[k] : 0;
            all += wc[k];
        }
        if (head && ord < p.len) out[ord] = i;
        run += all;
        __syncthreads();
    }
}


// plan, bounds, keys and all VX_MAX_PASSES passes of the sort (a cloud's blocks leave at once in the passes it does not need).
// Afterwards cloud c's sorted keys / rows are keys[npass & 1] / rows[npass & 1] at row0 .. + len of its plan.
inline int voxel_sort_enqueue(const float* xyz, const int32_t* row0, const int32_t* len, int32_t n_clouds, int32_t max_len,
                              const double* voxel, int64_t rows_cap, const Carve& cv, hipStream_t st) {
    voxel_plan_kernel<<<dim3(1), dim3(256), 0, st>>>(row0, len, n_clouds, max_len, rows_cap, blocks_cap(rows_cap, n_clouds), cv.plan);
    SCREAM_LAUNCH_CHECK();
    voxel_bounds_kernel<<<dim3(n_clouds), dim3(1024), 0, st>>>(xyz, voxel, cv.plan);
    SCREAM_LAUNCH_CHECK();
    if (max_len > 0) {
        const dim3 per_row((max_len + 255) / 256, n_clouds), per_tile((max_len + VX_TILE - 1) / VX_TILE, n_clouds);
        voxel_keys_kernel<<<per_row, dim3(256), 0, st>>>(xyz, cv.plan, cv.keys[0], cv.rows[0]);
        SCREAM_LAUNCH_CHECK();
        for (int pass = 0; pass < VX_MAX_PASSES; ++pass) {
            voxel_hist_kernel<<<per_tile, dim3(VX_THREADS), 0, st>>>(cv.plan, cv.keys[0], cv.keys[1], pass, cv.counts);
            SCREAM_LAUNCH_CHECK();
            voxel_scan_kernel<<<dim3(n_clouds), dim3(1024), 0, st>>>(cv.plan, pass, cv.counts);
            SCREAM_LAUNCH_CHECK();
            voxel_scatter_kernel<<<per_tile, dim3(VX_THREADS), 0, st>>>(cv.plan, cv.keys[0], cv.keys[1], cv.rows[0], cv.rows[1], pass,
                                                                        cv.counts);
            SCREAM_LAUNCH_CHECK();
        }
    }
    return 0;
}

}  // namespace
