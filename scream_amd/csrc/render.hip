// Depth renderer of the training-time GAN loss (models/render.py:8-73, RegistrationRender): for every (pair, view, side) the
// image img[p] = max_k pv_k g_kp over the side's points, g_kp = exp(-rho^2/2 |X_k,xy - c_p|^2), pv_k = 1 - (z_k - dmin) / (dmax
// - dmin), and its backward.  The reference materialises [n+m, 4096, 2] per view and reads dmin / dmax back to the host; here the
// depth range, the scan and the merge stay on the device (four launches, no host synchronisation).
//
// Arithmetic (include/scream_hip.h states the rules):
//   X = R p as fma(R2, pz, fma(R1, py, R0 px)) per row; c_p = (j - w/2 + 0.5) / (w/2) (IEEE divide);
//   pv = 1 - (z - dmin) / (dmax - dmin) (IEEE divide); d2 = fma(dy, dy, dx dx);
//   g = exp2(d2 * cexp), cexp = fp32(-rho^2 / 2 * log2(e)) (one v_exp_f32); value = pv g.
// The scan visits a block's points in ascending index order and keeps (best, index) with a strict '>' starting from (0, -1): the
// lowest index wins a tie and a pixel whose maximum is exactly 0 keeps index -1.  Blocks that split a point range merge with an
// integer atomicMax of 64-bit (value bits, ~index) keys (values are >= +0, so their bits order like the values): the result does
// not depend on how the range is split.
//
// Culling: a block stages only the points whose exponent is below -160 for NO pixel of its 32 x 32 tile.  The exponent of the
// tile's nearest pixel is computed with the same (monotone) roundings as the scan's, so every skipped point has t < -160 at every
// pixel of the tile, where exp2 is exactly 0 (2^-149 is the smallest fp32): skipping it changes nothing.
// This file is compiled with -ffp-contract=off: the forward, the range pass and the backward recompute X and pv with the same
// explicitly rounded operations.
#include <math.h>
#include <stdint.h>

#include "common.h"

namespace {

constexpr int TILE = 32;                       // pixel tile edge of a splat block (w % 64 == 0: tiles never straddle the edge)
constexpr int THREADS = 256;
constexpr int PPT = TILE * TILE / THREADS;     // pixels per lane: one column, rows 8 apart
constexpr int SUB = THREADS;                   // points tested against the tile per staging step (one per lane)
constexpr int CAP = 1024;                      // staged points in LDS (16 KiB)
constexpr float CULL_T = -160.0f;              // exp2 argument below which a point is skipped
constexpr int BWD_THREADS = 128;
constexpr int BWD_LDS_MAX_W = 128;             // the backward keeps the view's argmax map in LDS up to w = 128 (64 KiB)

__device__ __forceinline__ uint32_t f32_orderable(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float f32_from_orderable(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__device__ __forceinline__ void rotate(const float* __restrict__ R, float px, float py, float pz, float& x, float& y, float& z) {
    x = __fmaf_rn(R[2], pz, __fmaf_rn(R[1], py, __fmul_rn(R[0], px)));
    y = __fmaf_rn(R[5], pz, __fmaf_rn(R[4], py, __fmul_rn(R[3], px)));
    z = __fmaf_rn(R[8], pz, __fmaf_rn(R[7], py, __fmul_rn(R[6], px)));
}

// pixel-centre coordinate of column (or row) j: (j - w/2 + 0.5) / (w/2), as the reference's pix_xy (render.py:14-16)
__device__ __forceinline__ float centre(int j, int half) {
    return __fdiv_rn(__fadd_rn(__fsub_rn((float)j, (float)half), 0.5f), (float)half);
}

// depth range slots of (pair, view): [0] = ~orderable(min), [1] = orderable(max), both merged with atomicMax from 0
__device__ __forceinline__ void load_range(const uint32_t* __restrict__ range, int pv, float& dmin, float& span) {
    dmin = f32_from_orderable(~range[2 * pv]);
    const float dmax = f32_from_orderable(range[2 * pv + 1]);
    span = __fsub_rn(dmax, dmin);
}

__device__ __forceinline__ float pix_value(float z, float dmin, float span) {
    return __fsub_rn(1.0f, __fdiv_rn(__fsub_rn(z, dmin), span));
}

// grid (ceil(n_zero / 256)): zero the range slots and the merge keys
__global__ __launch_bounds__(256) void render_setup_kernel(uint32_t* __restrict__ range, int64_t n_range, uint64_t* __restrict__ keys,
                                                           int64_t n_keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_range) range[i] = 0u;
    if (i < n_keys) keys[i] = 0ull;
}

__device__ __forceinline__ float wave_min(float v) {
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// grid (ceil(max_len / 256), 2 sides, n_pairs): min / max of the rotated z over BOTH clouds of the pair, per view
__global__ __launch_bounds__(256) void render_range_kernel(const float* __restrict__ src, const int32_t* __restrict__ s_row0,
                                                           const int32_t* __restrict__ s_len, const float* __restrict__ tgt,
                                                           const int32_t* __restrict__ t_row0, const int32_t* __restrict__ t_len,
                                                           const float* __restrict__ rot, int V, uint32_t* __restrict__ range) {
    __shared__ float red[2][THREADS / 64];
    const int p = blockIdx.z, side = blockIdx.y;
    const int n = side ? t_len[p] : s_len[p];
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if ((int)(blockIdx.x * THREADS) >= n) return;  // block-uniform
    const float* pts = (side ? tgt : src) + (int64_t)(side ? t_row0[p] : s_row0[p]) * 3;
    const bool has = k < n;
    const float px = has ? pts[(int64_t)k * 3 + 0] : 0.0f, py = has ? pts[(int64_t)k * 3 + 1] : 0.0f,
                pz = has ? pts[(int64_t)k * 3 + 2] : 0.0f;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int v = 0; v < V; ++v) {
        float x, y, z;
        rotate(rot + v * 9, px, py, pz, x, y, z);
        const float lo = wave_min(has ? z : __builtin_inff()), hi = wave_max(has ? z : -__builtin_inff());
        if (lane == 0) {
            red[0][wv] = lo;
            red[1][wv] = hi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float a = red[0][0], b = red[1][0];
            for (int i = 1; i < THREADS / 64; ++i) {
                a = fminf(a, red[0][i]);
                b = fmaxf(b, red[1][i]);
            }
            atomicMax(range + 2 * ((int64_t)p * V + v), ~f32_orderable(a));
            atomicMax(range + 2 * ((int64_t)p * V + v) + 1, f32_orderable(b));
        }
        __syncthreads();
    }
}

// grid (tiles per image, splits, n_pairs * V * 2); blockIdx.z = (pair * V + view) * 2 + side
__global__ __launch_bounds__(THREADS) void render_splat_kernel(const float* __restrict__ src, const int32_t* __restrict__ s_row0,
                                                               const int32_t* __restrict__ s_len, const float* __restrict__ tgt,
                                                               const int32_t* __restrict__ t_row0, const int32_t* __restrict__ t_len,
                                                               const float* __restrict__ rot, int V, int w, float cexp, int per_split,
                                                               const uint32_t* __restrict__ range, uint64_t* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) f32x4 buf[CAP];
    __shared__ int wave_cnt[THREADS / 64];
    const int side = blockIdx.z & 1, pv_id = blockIdx.z >> 1;
    const int p = pv_id / V, v = pv_id % V;
    const int n = side ? t_len[p] : s_len[p];
    const int j_begin = blockIdx.y * per_split;
    const int j_end = min(n, j_begin + per_split);
    if (j_begin >= j_end) return;  // block-uniform
    float dmin, span;
    load_range(range, pv_id, dmin, span);
    if (!(span > 0.0f)) return;  // flat view: the finalize writes NaN
    const float* pts = (side ? tgt : src) + (int64_t)(side ? t_row0[p] : s_row0[p]) * 3;
    const float* R = rot + v * 9;
    const int half = w >> 1, tiles_x = w / TILE;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = tx * TILE + (tid & 31);
    const int row0 = ty * TILE + (tid >> 5);
    const float cx = centre(col, half);
    float cy[PPT], best[PPT];
    int bi[PPT];
#pragma unroll
    for (int u = 0; u < PPT; ++u) {
        cy[u] = centre(row0 + 8 * u, half);
        best[u] = 0.0f;
        bi[u] = -1;
    }
    const float x_lo = centre(tx * TILE, half), x_hi = centre(tx * TILE + TILE - 1, half);
    const float y_lo = centre(ty * TILE, half), y_hi = centre(ty * TILE + TILE - 1, half);

    int cnt = 0;  // staged points (block-uniform)
    for (int c = j_begin; c < j_end; c += SUB) {
        const int k = c + tid;
        bool keep = false;
        f32x4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        if (k < j_end) {
            float x, y, z;
            rotate(R, pts[(int64_t)k * 3 + 0], pts[(int64_t)k * 3 + 1], pts[(int64_t)k * 3 + 2], x, y, z);
            // distance to the tile's nearest pixel centre, with the scan's roundings (every one of them monotone)
            const float ddx = fmaxf(fmaxf(__fsub_rn(x_lo, x), __fsub_rn(x, x_hi)), 0.0f);
            const float ddy = fmaxf(fmaxf(__fsub_rn(y_lo, y), __fsub_rn(y, y_hi)), 0.0f);
            const float t = __fmul_rn(__fmaf_rn(ddy, ddy, __fmul_rn(ddx, ddx)), cexp);
            keep = t >= CULL_T;  // (NaN coordinates: never staged)
            q = f32x4{x, y, pix_value(z, dmin, span), __int_as_float(k)};
        }
        // order-preserving compaction: lanes in index order within a wave, waves in index order within the block
        const uint64_t m = __ballot(keep);
        if (lane == 0) wave_cnt[wv] = __popcll(m);
        __syncthreads();
        int off = cnt, total = 0;
#pragma unroll
        for (int i = 0; i < THREADS / 64; ++i) {
            off += i < wv ? wave_cnt[i] : 0;
            total += wave_cnt[i];
        }
        if (keep) buf[off + __popcll(m & ((1ull << lane) - 1ull))] = q;
        cnt += total;
        __syncthreads();
        if (cnt > CAP - SUB || c + SUB >= j_end) {
            for (int i = 0; i < cnt; ++i) {
                const f32x4 b = buf[i];  // wave-uniform address: broadcast
                const float dx = __fsub_rn(b[0], cx);
                const float dx2 = __fmul_rn(dx, dx);
#pragma unroll
                for (int u = 0; u < PPT; ++u) {
                    const float dy = __fsub_rn(b[1], cy[u]);
                    const float g = __builtin_amdgcn_exp2f(__fmul_rn(__fmaf_rn(dy, dy, dx2), cexp));
                    const float val = __fmul_rn(b[2], g);
                    if (val > best[u]) {
                        best[u] = val;
                        bi[u] = __float_as_int(b[3]);
                    }
                }
            }
            cnt = 0;
            __syncthreads();
        }
    }
    uint64_t* kp = keys + ((int64_t)blockIdx.z * w) * w;
#pragma unroll
    for (int u = 0; u < PPT; ++u) {
        if (bi[u] >= 0) {
            const uint64_t key = ((uint64_t)__float_as_uint(best[u]) << 32) | (uint64_t)(~(uint32_t)bi[u]);
            atomicMax(reinterpret_cast<unsigned long long*>(kp + (int64_t)(row0 + 8 * u) * w + col), (unsigned long long)key);
        }
    }
}

// grid (ceil(n_pix / 256)): keys -> images ((v - 0.5) / 0.5, render.py:69) and the argmax map
__global__ __launch_bounds__(256) void render_finalize_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ range,
                                                              int64_t n_pix, int w, float* __restrict__ imgs,
                                                              int32_t* __restrict__ argmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pix) return;
    const int pv_id = (int)(i / ((int64_t)w * w) >> 1);
    float dmin, span;
    load_range(range, pv_id, dmin, span);
    if (!(span > 0.0f)) {  // flat view: 0 / 0 in the reference, every pixel NaN
        imgs[i] = __builtin_nanf("");
        argmax[i] = -1;
        return;
    }
    const uint64_t key = keys[i];
    const float val = __uint_as_float((uint32_t)(key >> 32));  // key 0: value +0, no point
    imgs[i] = __fdiv_rn(__fsub_rn(val, 0.5f), 0.5f);
    argmax[i] = key ? (int32_t)~(uint32_t)key : -1;
}

// grid (ceil(max_s_len / 128), V, n_pairs): per source point and view, the gradient of the view's source image in the point's
// own coordinates, summed over the pixels whose argmax it is, in raster order over the window that holds every pixel where its g
// can be > 0; written to partial[v][row][3]
template <bool LDS>
__global__ __launch_bounds__(BWD_THREADS) void render_bwd_kernel(const float* __restrict__ src, const int32_t* __restrict__ s_row0,
                                                                 const int32_t* __restrict__ s_len, const float* __restrict__ rot, int V,
                                                                 int w, float cexp, float two_rho2, float reach,
                                                                 const uint32_t* __restrict__ range, const float* __restrict__ dimgs,
                                                                 const int32_t* __restrict__ argmax, int64_t rows_total,
                                                                 float* __restrict__ partial) {
    extern __shared__ int amap_lds[];
    const int p = blockIdx.z, v = blockIdx.y;
    const int n = s_len[p];
    if ((int)(blockIdx.x * BWD_THREADS) >= n) return;  // block-uniform
    const int64_t img0 = (((int64_t)p * V + v) * 2) * w * w;  // the source channel of (pair, view)
    const int32_t* amap = argmax + img0;
    if (LDS) {
        for (int i = threadIdx.x; i < w * w; i += BWD_THREADS) amap_lds[i] = amap[i];
        __syncthreads();
        amap = amap_lds;
    }
    const int k = blockIdx.x * BWD_THREADS + threadIdx.x;
    if (k >= n) return;
    const int64_t row = (int64_t)s_row0[p] + k;
    float* out = partial + ((int64_t)v * rows_total + row) * 3;
    float dmin, span;
    load_range(range, p * V + v, dmin, span);
    float x, y, z;
    const float* R = rot + v * 9;
    rotate(R, src[row * 3 + 0], src[row * 3 + 1], src[row * 3 + 2], x, y, z);
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (span > 0.0f && fabsf(x) <= 1e6f && fabsf(y) <= 1e6f) {
        const float pv = pix_value(z, dmin, span);
        const int half = w >> 1;
        // pixel j has its centre at (j - half + 0.5) / half: columns within `reach` of x, one pixel of margin on each side
        auto lo_of = [&](float c) { return (int)fminf(fmaxf(floorf((c - reach) * half + half - 0.5f) - 1.0f, 0.0f), (float)(w - 1)); };
        auto hi_of = [&](float c) { return (int)fminf(fmaxf(ceilf((c + reach) * half + half - 0.5f) + 1.0f, -1.0f), (float)(w - 1)); };
        const int j0 = lo_of(x), j1 = hi_of(x), i0 = lo_of(y), i1 = hi_of(y);
        const float* dimg = dimgs + img0;
        for (int i = i0; i <= i1; ++i) {
            const float dy = __fsub_rn(y, centre(i, half));
            for (int j = j0; j <= j1; ++j) {
                if (amap[i * w + j] != k) continue;
                const float dx = __fsub_rn(x, centre(j, half));
                const float g = __builtin_amdgcn_exp2f(__fmul_rn(__fmaf_rn(dy, dy, __fmul_rn(dx, dx)), cexp));
                const float f = __fmul_rn(dimg[i * w + j], g);  // dL/do g
                const float fp = __fmul_rn(f, pv);
                gx = __fmaf_rn(fp, dx, gx);
                gy = __fmaf_rn(fp, dy, gy);
                gz = __fadd_rn(gz, f);
            }
        }
        // do/dx = -2 rho^2 pv g (x - cx), do/dz = -2 g / (dmax - dmin)
        gx = __fmul_rn(gx, -two_rho2);
        gy = __fmul_rn(gy, -two_rho2);
        gz = __fdiv_rn(__fmul_rn(gz, -2.0f), span);
    }
    // d/dp = R^T d/dX
    out[0] = __fmaf_rn(R[6], gz, __fmaf_rn(R[3], gy, __fmul_rn(R[0], gx)));
    out[1] = __fmaf_rn(R[7], gz, __fmaf_rn(R[4], gy, __fmul_rn(R[1], gx)));
    out[2] = __fmaf_rn(R[8], gz, __fmaf_rn(R[5], gy, __fmul_rn(R[2], gx)));
}

// grid (ceil(max_s_len / 256), n_pairs): dsrc[row] = sum over views (ascending) of partial[v][row]
__global__ __launch_bounds__(256) void render_bwd_reduce_kernel(const float* __restrict__ partial, const int32_t* __restrict__ s_row0,
                                                                const int32_t* __restrict__ s_len, int V, int64_t rows_total,
                                                                float* __restrict__ dsrc) {
    const int p = blockIdx.y;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= s_len[p]) return;
    const int64_t row = (int64_t)s_row0[p] + k;
    float a = 0.0f, b = 0.0f, c = 0.0f;
    for (int v = 0; v < V; ++v) {
        const float* q = partial + ((int64_t)v * rows_total + row) * 3;
        a = __fadd_rn(a, q[0]);
        b = __fadd_rn(b, q[1]);
        c = __fadd_rn(c, q[2]);
    }
    dsrc[row * 3 + 0] = a;
    dsrc[row * 3 + 1] = b;
    dsrc[row * 3 + 2] = c;
}

// THE layout of the workspace: range [n_pairs][V][2], which the backward reads where the forward left it, then the forward's keys
// [n_pairs][V][2][w][w] or the backward's partial [V][src_rows_total][3].  From a null base it only measures.
struct RenderWs {
    uint32_t* range;
    uint64_t* keys;
    float* partial;
    int64_t bytes;
};
RenderWs render_carve(void* base, int32_t n_pairs, int32_t V, int32_t w, int64_t src_rows_total, bool backward) {
    Carver cv{base};
    RenderWs r = {};
    r.range = cv.take<uint32_t>((int64_t)n_pairs * V * 2);
    if (backward) r.partial = cv.take<float>((int64_t)V * src_rows_total * 3);
    else r.keys = cv.take<uint64_t>((int64_t)n_pairs * V * 2 * w * w);
    r.bytes = cv.used;
    return r;
}

float exp2_scale(float rho) { return (float)(-0.5 * (double)rho * (double)rho * 1.4426950408889634); }

bool bad_geometry(int32_t n_pairs, int32_t V, int32_t w, int64_t src_rows_total) {
    return n_pairs < 0 || V < 1 || w < 64 || w % 64 != 0 || w > 4096 || src_rows_total < 0;
}

}  // namespace

extern "C" int64_t scream_render_workspace_bytes(int32_t n_pairs, int32_t n_views, int32_t w, int64_t src_rows_total) {
    if (bad_geometry(n_pairs, n_views, w, src_rows_total)) return SCREAM_EINVAL;
    const int64_t fwd = render_carve(nullptr, n_pairs, n_views, w, src_rows_total, false).bytes;
    const int64_t bwd = render_carve(nullptr, n_pairs, n_views, w, src_rows_total, true).bytes;
    return fwd > bwd ? fwd : bwd;
}

extern "C" int scream_render_depth(const float* src, const int32_t* s_row0, const int32_t* s_len, const float* tgt,
                                   const int32_t* t_row0, const int32_t* t_len, int32_t n_pairs, int32_t max_s_len,
                                   int32_t max_t_len, int64_t src_rows_total, const float* rot, int32_t n_views, int32_t w,
                                   float rho, float* imgs, int32_t* argmax, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
    SCREAM_REQUIRE(src && s_row0 && s_len && tgt && t_row0 && t_len && rot && imgs && argmax && workspace, SCREAM_EINVAL);
    SCREAM_REQUIRE(!bad_geometry(n_pairs, n_views, w, src_rows_total) && max_s_len >= 0 && max_t_len >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(isfinite(rho), SCREAM_EINVAL);
    SCREAM_REQUIRE(workspace_bytes >= scream_render_workspace_bytes(n_pairs, n_views, w, src_rows_total), SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(workspace), SCREAM_EINVAL);
    if (n_pairs == 0) return 0;
    SCREAM_REQUIRE((int64_t)n_pairs * n_views * 2 <= 65535, SCREAM_EUNSUPPORTED);
    hipStream_t st = as_stream(stream);
    const RenderWs ws = render_carve(workspace, n_pairs, n_views, w, src_rows_total, false);
    uint32_t* range = ws.range;
    uint64_t* keys = ws.keys;
    const int64_t n_range = (int64_t)n_pairs * n_views * 2, n_pix = n_range * w * w;
    SCREAM_REQUIRE((n_pix + 255) / 256 < (1ll << 31), SCREAM_EUNSUPPORTED);
    render_setup_kernel<<<dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st>>>(range, n_range, keys, n_pix);
    SCREAM_LAUNCH_CHECK();
    const int max_len = max_s_len > max_t_len ? max_s_len : max_t_len;
    if (max_len > 0) {
        render_range_kernel<<<dim3((max_len + THREADS - 1) / THREADS, 2, n_pairs), dim3(THREADS), 0, st>>>(src, s_row0, s_len, tgt,
                                                                                                        t_row0, t_len, rot, n_views, range);
        SCREAM_LAUNCH_CHECK();
        // split each point range so that the launch has ~2 048 blocks when the images alone give fewer (B = 1: 48 blocks of
        // 1 024 pixels at w = 64), but never below 256 points per block; the merge makes the result independent of the split
        // (restated line for line as split_plan() in tests/render_ref.py, by which the tests know that a shape reaches the
        // mid-range scan of the splat block: change both together)
        const int64_t tiles = (int64_t)(w / TILE) * (w / TILE);
        const int64_t base = tiles * n_range;
        int64_t splits = (2048 + base - 1) / base;
        const int64_t max_splits = (max_len + SUB - 1) / SUB;
        splits = splits < max_splits ? splits : max_splits;
        splits = splits < 1 ? 1 : splits;
        const int per_split = (int)((max_len + splits - 1) / splits);
        splits = (max_len + per_split - 1) / per_split;
        SCREAM_REQUIRE(tiles < (1ll << 31), SCREAM_EUNSUPPORTED);
        render_splat_kernel<<<dim3((unsigned)tiles, (unsigned)splits, (unsigned)n_range), dim3(THREADS), 0, st>>>(
            src, s_row0, s_len, tgt, t_row0, t_len, rot, n_views, w, exp2_scale(rho), per_split, range, keys);
        SCREAM_LAUNCH_CHECK();
    }
    render_finalize_kernel<<<dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st>>>(keys, range, n_pix, w, imgs, argmax);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_render_depth_bwd(const float* src, const int32_t* s_row0, const int32_t* s_len, int32_t n_pairs,
                                       int32_t max_s_len, int64_t src_rows_total, const float* rot, int32_t n_views, int32_t w,
                                       float rho, const float* dimgs, const int32_t* argmax, void* workspace,
                                       int64_t workspace_bytes, float* dsrc, void* stream) {
    SCREAM_REQUIRE(src && s_row0 && s_len && rot && dimgs && argmax && workspace && dsrc, SCREAM_EINVAL);
    SCREAM_REQUIRE(!bad_geometry(n_pairs, n_views, w, src_rows_total) && max_s_len >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(isfinite(rho), SCREAM_EINVAL);
    SCREAM_REQUIRE(workspace_bytes >= scream_render_workspace_bytes(n_pairs, n_views, w, src_rows_total), SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(workspace), SCREAM_EINVAL);
    if (n_pairs == 0 || max_s_len == 0) return 0;
    SCREAM_REQUIRE(n_views <= 65535 && n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    hipStream_t st = as_stream(stream);
    const RenderWs ws = render_carve(workspace, n_pairs, n_views, w, src_rows_total, true);
    const uint32_t* range = ws.range;
    float* partial = ws.partial;
    const float cexp = exp2_scale(rho);
    // g > 0 needs d^2 cexp >= -150 or so; the window reaches sqrt(160 / |cexp|) (all of the image when rho == 0)
    const float reach = cexp < 0.0f ? (float)sqrt(160.0 / -(double)cexp) : 4.0f;
    const float two_rho2 = (float)(2.0 * (double)rho * (double)rho);
    const dim3 grid((max_s_len + BWD_THREADS - 1) / BWD_THREADS, n_views, n_pairs);
    if (w <= BWD_LDS_MAX_W) {
        render_bwd_kernel<true><<<grid, dim3(BWD_THREADS), (size_t)w * w * 4, st>>>(src, s_row0, s_len, rot, n_views, w, cexp, two_rho2,
                                                                                    reach, range, dimgs, argmax, src_rows_total, partial);
    } else {
        render_bwd_kernel<false><<<grid, dim3(BWD_THREADS), 0, st>>>(src, s_row0, s_len, rot, n_views, w, cexp, two_rho2, reach, range,
                                                                     dimgs, argmax, src_rows_total, partial);
    }
    SCREAM_LAUNCH_CHECK();
    render_bwd_reduce_kernel<<<dim3((max_s_len + 255) / 256, n_pairs), dim3(256), 0, st>>>(partial, s_row0, s_len, n_views,
                                                                                            src_rows_total, dsrc);
    SCREAM_LAUNCH_CHECK();
    return 0;
}
