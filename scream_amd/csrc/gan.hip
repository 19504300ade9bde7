// The adversarial loss in HIP: the reference's NLayerDiscriminator(input_nc, ndf, n_layers=3) (models/gan.py:15-65), its
// backward, and the two hinge losses of loss.py:31-35,53-66.  Contract: include/scream_hip.h.
//
// Layout.  Every activation stays NCHW fp32, as the renderer writes its images and as torch holds the weights [Cout,Cin,4,4]:
// with the contraction index ordered (ci, kh, kw) a weight row IS a row of the GEMM's operand, and so is a row of the weight
// gradient, so no weight image is ever packed and no activation is ever transposed.
//
// Convolutions.  Forward, data gradient and weight gradient are three instances of one implicit GEMM on v_mfma_f32_32x32x2_f32
// (fp32 in, fp32 accumulate, a k-ordered fma chain: the arithmetic of train_backend="f32").  One wave owns one 32 x 32 tile
// of   rows x cols  and walks the contraction in steps of 8: lane (r, half) supplies elements 4 half + i (i = 0..3) of operand
// row r for both operands, gathered straight from global memory with the padding and the stride folded into the address
// (out-of-image taps are zeros, never loads).  The weight gradient, whose contraction runs along the pixels, loads 32 pixels
// with the lanes along them, one load ahead in registers, and turns them into the operand layout through 8 KiB of LDS.
//              rows        cols                 contraction
//   forward    co          pixel (n, oh, ow)    (ci, kh, kw)          y  = W . im2col(x)
//   dgrad      ci          pixel (n, ih, iw)    (co, kh, kw)          dx = W^T . col2im taps of dy
//   wgrad      co          (ci, kh, kw)         pixel (n, oh, ow)     dW = dy . im2col(x)^T
// The contraction is cut into z equal ranges (make_plan: a pure function of the shape); range z's tile goes to partial[z], whose
// columns are padded to whole tiles and whose rows are the true ones (a padded row of a tile is computed and dropped).  A second launch (finish_kernel) adds the partials of an element in
// ascending z from partial[0], then applies the epilogue (bias; LeakyReLU; the leaky mask of the layer below) and writes the
// true shape.  No float atomics: a result depends on the shape alone, two identical calls give identical bits.
// What the padding costs: rows and cols are padded to 32, so the last layer (Cout = 1) spends 31 of 32 matrix rows on zeros
// (0.1 GFLOP of padding per 6 images, spread over 64 contraction ranges), and the first layer's dgrad (Cin <= 4) likewise; the
// first layer's contraction 16 Cin is a multiple of 8 and is not padded at all.  The stride-2 data gradients evaluate all 16
// taps although 4 land on a pixel: three quarters of their matrix work multiplies zeros.
//
// BatchNorm + LeakyReLU, losses: per-channel and whole-tensor sums are float64, one block per channel: thread t of 256 adds
// its elements t, t + 256, ... (in the order n-major, pixel-minor) from 0.0, then the tree v[t] += v[t + 128], + 64, ... + 1.
#include "common.h"

namespace {

constexpr float LEAK = 0.2f;
constexpr int FWD = 0, DGRAD = 1, WGRAD = 2;
constexpr int64_t MAX_PARTIAL = (int64_t)1 << 24;  // floats of partial tiles beyond which the contraction is not cut further

struct Geo {
    int N, Cin, H, W, Cout, Ho, Wo, s;
};

bool make_geo(int n, int cin, int cout, int h, int w, int stride, Geo& g) {
    if (n <= 0 || cin <= 0 || cout <= 0 || h < 2 || w < 2 || (stride != 1 && stride != 2)) return false;
    g = Geo{n, cin, h, w, cout, (h - 2) / stride + 1, (w - 2) / stride + 1, stride};
    const int64_t lim = INT32_MAX / 2;  // every element index and every padded tile count stays an int32
    return (int64_t)n * cin * h * w < lim && (int64_t)n * cout * g.Ho * g.Wo < lim && (int64_t)cout * cin * 16 < lim &&
           (int64_t)n * h * w < lim;
}

struct Plan {
    int rows, cols, rpad, cpad, steps, spz, z;
    // only the true rows of a range are kept: the padded rows of a tile (31 of 32 where Cout = 1 or Cin <= 4) are never stored
    int64_t floats() const { return (int64_t)z * rows * cpad; }
};

int pad32(int v) { return (v + 31) / 32 * 32; }

// The cut of one GEMM: enough waves to occupy the machine (about 1024; 8192 for the weight gradient), at least 16 steps per
// range, at most 64 ranges, and the partial tiles within MAX_PARTIAL floats where one range already fits.
Plan make_plan(int mode, const Geo& g) {
    Plan p;
    const int M = g.N * g.Ho * g.Wo;
    int red;
    if (mode == FWD) p.rows = g.Cout, p.cols = M, red = 16 * g.Cin;
    else if (mode == DGRAD) p.rows = g.Cin, p.cols = g.N * g.H * g.W, red = 16 * g.Cout;
    else p.rows = g.Cout, p.cols = 16 * g.Cin, red = M;
    p.rpad = pad32(p.rows), p.cpad = pad32(p.cols);
    p.steps = (red + 7) / 8;
    const int64_t tiles = (int64_t)p.rpad * p.cpad / 1024, tile_floats = (int64_t)p.rows * p.cpad;  // matrix work | floats kept
    // the weight gradient has few tiles and a long, latency-bound contraction: it wants eight waves per SIMD to hide its loads
    int64_t z = (mode == WGRAD ? 8192 : 1024) / tiles;
    if (z > p.steps / 16) z = p.steps / 16;
    if (z > MAX_PARTIAL / tile_floats) z = MAX_PARTIAL / tile_floats;
    if (z > 64) z = 64;
    if (z < 1) z = 1;
    p.spz = (int)((p.steps + z - 1) / z);
    if (mode == WGRAD) p.spz = (p.spz + 3) / 4 * 4;  // whole 32-pixel loads
    p.z = (p.steps + p.spz - 1) / p.spz;
    return p;
}

// P / Q: forward (w, x), dgrad (w, dy), wgrad (dy, x)
template <int MODE>
__global__ __launch_bounds__(64) void conv_mfma_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                       float* __restrict__ partial, Geo g, int steps, int spz, int rows, int cpad) {
    __shared__ float lds[MODE == WGRAD ? 2 * 32 * 33 : 1];  // the weight gradient's two operand tiles of 32 pixels
    const int lane = threadIdx.x, r = lane & 31, half = lane >> 5;
    const int row = blockIdx.y * 32 + r, col = blockIdx.x * 32 + r;  // this lane's operand row / operand column
    const int s0 = blockIdx.z * spz, s1 = min(steps, s0 + spz);
    const int HoWo = g.Ho * g.Wo;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    if (MODE == FWD) {
        const int K = 16 * g.Cin, M = g.N * HoWo;
        const bool rowok = row < g.Cout, colok = col < M;
        const int n = col / HoWo, p = col - n * HoWo, oh = p / g.Wo, ow = p - oh * g.Wo;
        const int ih0 = oh * g.s - 1, iw0 = ow * g.s - 1;
        const float* wrow = P + (int64_t)row * K;
        for (int st = s0; st < s1; ++st) {
            const int kk = st * 8 + 4 * half, ci = kk >> 4, ih = ih0 + ((kk >> 2) & 3);
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (rowok) a = ld4(wrow + kk);
            if (colok && (unsigned)ih < (unsigned)g.H) {
                const float* xr = Q + (((int64_t)n * g.Cin + ci) * g.H + ih) * g.W;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if ((unsigned)(iw0 + i) < (unsigned)g.W) b[i] = xr[iw0 + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
        }
    } else if (MODE == DGRAD) {
        const int HW = g.H * g.W, M = g.N * HW, sh = g.s - 1;
        const bool rowok = row < g.Cin, colok = col < M;
        const int n = col / HW, p = col - n * HW, ih = p / g.W, iw = p - ih * g.W;
        for (int st = s0; st < s1; ++st) {
            const int kk = st * 8 + 4 * half, co = kk >> 4, kh = (kk >> 2) & 3;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (rowok) a = ld4(P + ((int64_t)co * g.Cin + row) * 16 + kh * 4);
            const int th = ih + 1 - kh, oh = th >> sh;
            if (colok && th >= 0 && (th & sh) == 0 && oh < g.Ho) {
                const float* dyr = Q + (((int64_t)n * g.Cout + co) * g.Ho + oh) * g.Wo;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int tw = iw + 1 - i, ow = tw >> sh;
                    if (tw >= 0 && (tw & sh) == 0 && ow < g.Wo) b[i] = dyr[ow];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[i], acc, 0, 0, 0);
        }
    } else {
        // The contraction runs over pixels, which are contiguous in memory for a fixed operand row (a channel of dy, a tap of
        // x): 32 pixels at a time are loaded with the lanes along the pixels (lane (r, half) loads pixel r of operand rows
        // 2 j + half) and turned through LDS into the operand layout (lane r = operand row).  The sum order is unchanged:
        // pixel 8 step + 4 half + i in instruction i of the step.
        const int K = 16 * g.Cin, M = g.N * HoWo;
        const int m1 = min(M, s1 * 8);
        float* la = lds;
        float* lb = lds + 32 * 33;
        float va[16], vb[16];
        auto load = [&](int mb) {  // the 32 pixels from mb on, into registers: they land under the previous 32 pixels' MFMAs
            const int m = mb + r;
            const bool ok = m < m1;
            const int n = m / HoWo, p = m - n * HoWo, oh = p / g.Wo, ow = p - oh * g.Wo;
            const int ih0 = oh * g.s - 1, iw0 = ow * g.s - 1;
            const float* dyp = P + (int64_t)n * g.Cout * HoWo + p;
            const float* xp = Q + (int64_t)n * g.Cin * g.H * g.W;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int t = 2 * j + half, co = blockIdx.y * 32 + t, k = blockIdx.x * 32 + t;
                const int ih = ih0 + ((k >> 2) & 3), iw = iw0 + (k & 3);
                va[j] = 0.f, vb[j] = 0.f;
                if (ok && co < g.Cout) va[j] = dyp[(int64_t)co * HoWo];
                if (ok && k < K && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)
                    vb[j] = xp[((int64_t)(k >> 4) * g.H + ih) * g.W + iw];
            }
        };
        if (s0 * 8 < m1) load(s0 * 8);
        for (int mb = s0 * 8; mb < m1; mb += 32) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                la[(2 * j + half) * 33 + r] = va[j];
                lb[(2 * j + half) * 33 + r] = vb[j];
            }
            __syncthreads();
            if (mb + 32 < m1) load(mb + 32);
#pragma unroll
            for (int e = 0; e < 32; e += 8)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(la[r * 33 + e + 4 * half + i], lb[r * 33 + e + 4 * half + i], acc, 0, 0, 0);
            __syncthreads();
        }
    }
    // partial[z] is [rows, cpad]: cpad is whole tiles, so every column has its place; rows past the true count are dropped
    float* tile = partial + (int64_t)blockIdx.z * rows * cpad + blockIdx.x * 32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int tr = blockIdx.y * 32 + mfma32_row(e, half);
        if (tr < rows) tile[(int64_t)tr * cpad] = acc[e];
    }
}

// out[idx] = epilogue(partial[0] + partial[1] + ... of its element).  FWD / DGRAD: out is NCHW [N, rows, hw], the element's
// column is n hw + pixel; WGRAD: out is [rows, cols].
template <int MODE>
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ partial, int z, int cpad, int rows, int hw,
                                                     int64_t total, const float* __restrict__ bias, int leaky,
                                                     const float* __restrict__ mask, float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int row, col;
    if (MODE == WGRAD) {
        row = (int)(idx / hw), col = (int)(idx - (int64_t)row * hw);  // hw: the true column count 16 Cin
    } else {
        const int nc = (int)(idx / hw), p = (int)(idx - (int64_t)nc * hw), n = nc / rows;
        row = nc - n * rows, col = n * hw + p;
    }
    const float* src = partial + (int64_t)row * cpad + col;
    const int64_t zs = (int64_t)rows * cpad;
    float v = src[0];
    for (int k = 1; k < z; ++k) v += src[k * zs];
    if (bias) v += bias[row];
    if (leaky) v = v > 0.f ? v : LEAK * v;
    if (mask) v = mask[idx] > 0.f ? v : LEAK * v;
    out[idx] = v;
}

int conv_run(int mode, const Geo& g, const float* P, const float* Q, float* out, const float* bias, int leaky, const float* mask,
             float* scratch, int64_t scratch_floats, hipStream_t st) {
    const Plan p = make_plan(mode, g);
    SCREAM_REQUIRE(scratch && scratch_floats >= p.floats(), SCREAM_EINVAL);
    SCREAM_REQUIRE(p.rpad / 32 <= 65535, SCREAM_EUNSUPPORTED);
    const dim3 grid(p.cpad / 32, p.rpad / 32, p.z);
    int64_t total;
    int hw;
    if (mode == FWD) {
        conv_mfma_kernel<FWD><<<grid, 64, 0, st>>>(P, Q, scratch, g, p.steps, p.spz, p.rows, p.cpad);
        hw = g.Ho * g.Wo, total = (int64_t)g.N * g.Cout * hw;
    } else if (mode == DGRAD) {
        conv_mfma_kernel<DGRAD><<<grid, 64, 0, st>>>(P, Q, scratch, g, p.steps, p.spz, p.rows, p.cpad);
        hw = g.H * g.W, total = (int64_t)g.N * g.Cin * hw;
    } else {
        conv_mfma_kernel<WGRAD><<<grid, 64, 0, st>>>(P, Q, scratch, g, p.steps, p.spz, p.rows, p.cpad);
        hw = 16 * g.Cin, total = (int64_t)g.Cout * hw;
    }
    SCREAM_LAUNCH_CHECK();
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (mode == FWD) finish_kernel<FWD><<<blocks, 256, 0, st>>>(scratch, p.z, p.cpad, p.rows, hw, total, bias, leaky, mask, out);
    else if (mode == DGRAD) finish_kernel<DGRAD><<<blocks, 256, 0, st>>>(scratch, p.z, p.cpad, p.rows, hw, total, bias, leaky, mask, out);
    else finish_kernel<WGRAD><<<blocks, 256, 0, st>>>(scratch, p.z, p.cpad, p.rows, hw, total, bias, leaky, mask, out);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

// ---- float64 block sums ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// BatchNorm statistics of channel blockIdx.x over [N, C, hw].  training: batch statistics, running update; otherwise the
// running statistics become mean / invstd.
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, int N, int C, int hw, int training,
                                                       float* __restrict__ running_mean, float* __restrict__ running_var,
                                                       int64_t* __restrict__ nbt, float* __restrict__ mean, float* __restrict__ invstd) {
    __shared__ double sh[256];
    const int c = blockIdx.x, t = threadIdx.x;
    if (!training) {
        if (t == 0) {
            mean[c] = running_mean[c];
            invstd[c] = (float)(1.0 / sqrt((double)running_var[c] + 1e-5));
        }
        return;
    }
    const int total = N * hw;
    double s1 = 0.0, s2 = 0.0;
    for (int e = t; e < total; e += 256) {
        const int n = e / hw, p = e - n * hw;
        const double v = (double)x[((int64_t)n * C + c) * hw + p];
        s1 += v;
        s2 += v * v;
    }
    s1 = block_sum(s1, sh);
    s2 = block_sum(s2, sh);
    if (t == 0) {
        const double cnt = (double)total, m = s1 / cnt;
        double var = s2 / cnt - m * m;
        if (var < 0.0) var = 0.0;
        mean[c] = (float)m;
        invstd[c] = (float)(1.0 / sqrt(var + 1e-5));
        running_mean[c] = (float)(0.9 * (double)running_mean[c] + 0.1 * m);
        running_var[c] = (float)(0.9 * (double)running_var[c] + 0.1 * (var * (cnt / (cnt - 1.0))));
        if (c == 0 && nbt) nbt[0] += 1;
    }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, int C, int hw, int64_t total,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       float* __restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)((idx / hw) % C);
    const float v = ((x[idx] - mean[c]) * invstd[c]) * gamma[c] + beta[c];
    y[idx] = v > 0.f ? v : LEAK * v;
}

// sums[2c] = sum dz, sums[2c + 1] = sum dz xhat, dz = dy (y > 0 ? 1 : 0.2), xhat = (x - mean) invstd as the forward rounds it
__global__ __launch_bounds__(256) void bn_bwd_sums_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                          const float* __restrict__ x, int N, int C, int hw,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          double* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sh[256];
    const int c = blockIdx.x, t = threadIdx.x, total = N * hw;
    const float mu = mean[c], is = invstd[c];
    double s1 = 0.0, s2 = 0.0;
    for (int e = t; e < total; e += 256) {
        const int n = e / hw, p = e - n * hw;
        const int64_t idx = ((int64_t)n * C + c) * hw + p;
        const float g = dy[idx], dz = y[idx] > 0.f ? g : LEAK * g;
        s1 += (double)dz;
        s2 += (double)dz * (double)((x[idx] - mu) * is);
    }
    s1 = block_sum(s1, sh);
    s2 = block_sum(s2, sh);
    if (t == 0) {
        sums[2 * c] = s1, sums[2 * c + 1] = s2;
        if (dbeta) dbeta[c] = (float)s1;
        if (dgamma) dgamma[c] = (float)s2;
    }
}

// (dx may be dy: an element is read before it is written, by its own thread)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* dy, const float* __restrict__ y,
                                                           const float* __restrict__ x, int C, int hw, int64_t total, double cnt,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const double* __restrict__ sums,
                                                           float* dx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)((idx / hw) % C);
    const float g = dy[idx], dz = y[idx] > 0.f ? g : LEAK * g;
    const double xhat = (double)((x[idx] - mean[c]) * invstd[c]);
    const double k = (double)gamma[c] * (double)invstd[c];
    dx[idx] = (float)(k * (((double)dz - sums[2 * c] / cnt) - xhat * (sums[2 * c + 1] / cnt)));
}

// db[c] = sum over n and pixels of dy[n, c, .]
__global__ __launch_bounds__(256) void bias_sum_kernel(const float* __restrict__ dy, int N, int C, int hw, float* __restrict__ db) {
    __shared__ double sh[256];
    const int c = blockIdx.x, t = threadIdx.x, total = N * hw;
    double s = 0.0;
    for (int e = t; e < total; e += 256) {
        const int n = e / hw, p = e - n * hw;
        s += (double)dy[((int64_t)n * C + c) * hw + p];
    }
    s = block_sum(s, sh);
    if (t == 0) db[c] = (float)s;
}

// ---- losses (one block each) -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void loss_g_kernel(const float* __restrict__ logits, int64_t cnt, float* __restrict__ loss) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < cnt; e += 256) s += (double)logits[e];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) loss[0] = (float)(-(s / (double)cnt));
}

__global__ __launch_bounds__(256) void loss_g_bwd_kernel(const float* __restrict__ dout, int64_t cnt, float* __restrict__ dlogits) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < cnt) dlogits[idx] = (float)(-((double)dout[0] / (double)cnt));
}

__global__ __launch_bounds__(256) void loss_d_kernel(const float* __restrict__ real, int64_t cnt_r, const float* __restrict__ fake,
                                                     int64_t cnt_f, float* __restrict__ loss) {
    __shared__ double sh[256];
    double sr = 0.0, sf = 0.0;
    for (int64_t e = threadIdx.x; e < cnt_r; e += 256) sr += (double)fmaxf(1.f - real[e], 0.f);
    for (int64_t e = threadIdx.x; e < cnt_f; e += 256) sf += (double)fmaxf(1.f + fake[e], 0.f);
    sr = block_sum(sr, sh);
    sf = block_sum(sf, sh);
    if (threadIdx.x == 0) loss[0] = (float)(0.5 * (sr / (double)cnt_r + sf / (double)cnt_f));
}

__global__ __launch_bounds__(256) void loss_d_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ real, int64_t cnt_r,
                                                         const float* __restrict__ fake, int64_t cnt_f, float* __restrict__ dreal,
                                                         float* __restrict__ dfake) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const double h = 0.5 * (double)dout[0];
    if (idx < cnt_r) dreal[idx] = (1.f - real[idx]) > 0.f ? (float)(-(h / (double)cnt_r)) : 0.f;
    if (idx < cnt_f) dfake[idx] = (1.f + fake[idx]) > 0.f ? (float)(h / (double)cnt_f) : 0.f;
}

// the ground-truth source rows of the `real` images: out = R_p x + t_p on every packed source row, p the pair of the row's tile
__global__ __launch_bounds__(256) void pairs_transform_kernel(const float* __restrict__ xyz, const float* __restrict__ rot,
                                                              const float* __restrict__ trans, const int32_t* __restrict__ tile_cloud,
                                                              int n_pairs, int64_t rows, float* __restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const int p = tile_cloud[row / SCREAM_ROW_TILE];
    const float x = xyz[3 * row], y = xyz[3 * row + 1], z = xyz[3 * row + 2];
    if (p < 0 || p >= n_pairs) {
        out[3 * row] = x, out[3 * row + 1] = y, out[3 * row + 2] = z;
        return;
    }
    const float* R = rot + 9 * p;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * row + k] = ((R[3 * k] * x + R[3 * k + 1] * y) + R[3 * k + 2] * z) + trans[3 * p + k];
}

unsigned blocks_of(int64_t total) { return (unsigned)((total + 255) / 256); }

int bn_fwd_run(const float* x, const float* gamma, const float* beta, float* rm, float* rv, int64_t* nbt, int n, int c, int hw,
               int training, float* y, float* mean, float* invstd, hipStream_t st) {
    bn_stats_kernel<<<c, 256, 0, st>>>(x, n, c, hw, training, rm, rv, nbt, mean, invstd);
    SCREAM_LAUNCH_CHECK();
    const int64_t total = (int64_t)n * c * hw;
    bn_apply_kernel<<<blocks_of(total), 256, 0, st>>>(x, c, hw, total, gamma, beta, mean, invstd, y);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

int bn_bwd_run(const float* dy, const float* y, const float* x, const float* gamma, const float* mean, const float* invstd, int n,
               int c, int hw, double* sums, float* dx, float* dgamma, float* dbeta, hipStream_t st) {
    bn_bwd_sums_kernel<<<c, 256, 0, st>>>(dy, y, x, n, c, hw, mean, invstd, sums, dgamma, dbeta);
    SCREAM_LAUNCH_CHECK();
    const int64_t total = (int64_t)n * c * hw;
    bn_bwd_apply_kernel<<<blocks_of(total), 256, 0, st>>>(dy, y, x, c, hw, total, (double)n * hw, gamma, mean, invstd, sums, dx);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

// ---- the whole network -------------------------------------------------------------------------------------------------------
struct Net {
    Geo L[5];
};

bool make_net(int n, int cin, int ndf, int h, int w, Net& net) {
    if (n <= 0 || cin < 1 || cin > 4 || ndf <= 0 || ndf % 32 || h < 24 || w < 24) return false;
    const int ch[6] = {cin, ndf, 2 * ndf, 4 * ndf, 8 * ndf, 1}, stride[5] = {2, 2, 2, 1, 1};
    for (int l = 0; l < 5; ++l) {
        if (!make_geo(n, ch[l], ch[l + 1], h, w, stride[l], net.L[l])) return false;
        h = net.L[l].Ho, w = net.L[l].Wo;
    }
    return true;
}

int64_t out_floats(const Geo& g) { return (int64_t)g.N * g.Cout * g.Ho * g.Wo; }

// The one carve of a pass.  The forward fills a1 .. invstd; the backward reads them and works in the rest.
struct NetWs {
    float* a1;             // leaky(conv1 + b)
    float *x[3], *a[3];    // conv output and leaky(bn(.)) of layers 2 .. 4
    float *mean[3], *invstd[3];
    double* sums;          // [2 * 8 ndf] of the BatchNorm backward
    float *ga, *gb;        // two gradient buffers, each the size of the largest activation
    float* scratch;        // partial tiles of the convolution in flight
    int64_t scratch_floats;
};

NetWs carve_net(void* base, const Net& net, int64_t* bytes) {
    Carver cv{base};
    NetWs ws;
    int64_t big = out_floats(net.L[0]), scratch = 0;
    ws.a1 = cv.take<float>(big);
    for (int l = 1; l < 4; ++l) {
        const int64_t f = out_floats(net.L[l]);
        big = f > big ? f : big;
        ws.x[l - 1] = cv.take<float>(f);
        ws.a[l - 1] = cv.take<float>(f);
        ws.mean[l - 1] = cv.take<float>(net.L[l].Cout);
        ws.invstd[l - 1] = cv.take<float>(net.L[l].Cout);
    }
    ws.sums = cv.take<double>(2 * (int64_t)net.L[3].Cout);
    ws.ga = cv.take<float>(big);
    ws.gb = cv.take<float>(big);
    for (int l = 0; l < 5; ++l)
        for (int mode = 0; mode < 3; ++mode) {
            const int64_t f = make_plan(mode, net.L[l]).floats();
            scratch = f > scratch ? f : scratch;
        }
    ws.scratch = cv.take<float>(scratch);
    ws.scratch_floats = scratch;
    *bytes = cv.used;
    return ws;
}

}  // namespace

extern "C" int64_t scream_gan_conv_workspace_bytes(int32_t mode, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w,
                                                   int32_t stride) {
    Geo g;
    if (mode < 0 || mode > 2 || !make_geo(n, cin, cout, h, w, stride, g)) return -1;
    return make_plan(mode, g).floats() * 4;
}

#define GAN_CONV_ARGS()                                                     \
    Geo g;                                                                  \
    SCREAM_REQUIRE(make_geo(n, cin, cout, h, w, stride, g), SCREAM_EINVAL); \
    SCREAM_REQUIRE(workspace && aligned16(workspace), SCREAM_EINVAL)

extern "C" int scream_gan_conv_fwd(const float* x, const float* wt, const float* bias, int32_t n, int32_t cin, int32_t cout,
                                   int32_t h, int32_t w, int32_t stride, int32_t leaky, float* y, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    GAN_CONV_ARGS();
    SCREAM_REQUIRE(x && y && wt && aligned16(wt), SCREAM_EINVAL);
    return conv_run(FWD, g, wt, x, y, bias, leaky, nullptr, (float*)workspace, workspace_bytes / 4, as_stream(stream));
}

extern "C" int scream_gan_conv_dgrad(const float* dy, const float* wt, const float* mask, int32_t n, int32_t cin, int32_t cout,
                                     int32_t h, int32_t w, int32_t stride, float* dx, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
    GAN_CONV_ARGS();
    SCREAM_REQUIRE(dy && dx && wt && aligned16(wt), SCREAM_EINVAL);
    return conv_run(DGRAD, g, wt, dy, dx, nullptr, 0, mask, (float*)workspace, workspace_bytes / 4, as_stream(stream));
}

extern "C" int scream_gan_conv_wgrad(const float* x, const float* dy, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w,
                                     int32_t stride, float* dw, float* dbias, void* workspace, int64_t workspace_bytes,
                                     void* stream) {
    GAN_CONV_ARGS();
    SCREAM_REQUIRE(x && dy && dw, SCREAM_EINVAL);
    if (int rc = conv_run(WGRAD, g, dy, x, dw, nullptr, 0, nullptr, (float*)workspace, workspace_bytes / 4, as_stream(stream))) return rc;
    if (dbias) {
        bias_sum_kernel<<<cout, 256, 0, as_stream(stream)>>>(dy, n, cout, g.Ho * g.Wo, dbias);
        SCREAM_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int scream_gan_bn_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, int32_t n, int32_t c, int32_t hw, int32_t training, float* y,
                                 float* mean, float* invstd, void* stream) {
    SCREAM_REQUIRE(x && gamma && beta && running_mean && running_var && y && mean && invstd, SCREAM_EINVAL);
    SCREAM_REQUIRE(n > 0 && c > 0 && hw > 0 && (int64_t)n * c * hw < INT32_MAX, SCREAM_EINVAL);
    SCREAM_REQUIRE(!training || (int64_t)n * hw > 1, SCREAM_EINVAL);
    return bn_fwd_run(x, gamma, beta, running_mean, running_var, num_batches_tracked, n, c, hw, training, y, mean, invstd,
                      as_stream(stream));
}

extern "C" int scream_gan_bn_bwd(const float* dy, const float* y, const float* x, const float* gamma, const float* mean,
                                 const float* invstd, int32_t n, int32_t c, int32_t hw, double* sums, float* dx, float* dgamma,
                                 float* dbeta, void* stream) {
    SCREAM_REQUIRE(dy && y && x && gamma && mean && invstd && sums && aligned8(sums) && dx, SCREAM_EINVAL);
    SCREAM_REQUIRE(n > 0 && c > 0 && hw > 0 && (int64_t)n * c * hw < INT32_MAX, SCREAM_EINVAL);
    return bn_bwd_run(dy, y, x, gamma, mean, invstd, n, c, hw, sums, dx, dgamma, dbeta, as_stream(stream));
}

extern "C" int scream_gan_loss_g(const float* logits, int64_t cnt, float* loss, void* stream) {
    SCREAM_REQUIRE(logits && loss && cnt > 0, SCREAM_EINVAL);
    loss_g_kernel<<<1, 256, 0, as_stream(stream)>>>(logits, cnt, loss);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_gan_loss_g_bwd(const float* dout, int64_t cnt, float* dlogits, void* stream) {
    SCREAM_REQUIRE(dout && dlogits && cnt > 0, SCREAM_EINVAL);
    loss_g_bwd_kernel<<<blocks_of(cnt), 256, 0, as_stream(stream)>>>(dout, cnt, dlogits);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_gan_loss_d(const float* real, int64_t cnt_r, const float* fake, int64_t cnt_f, float* loss, void* stream) {
    SCREAM_REQUIRE(real && fake && loss && cnt_r > 0 && cnt_f > 0, SCREAM_EINVAL);
    loss_d_kernel<<<1, 256, 0, as_stream(stream)>>>(real, cnt_r, fake, cnt_f, loss);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_gan_loss_d_bwd(const float* dout, const float* real, int64_t cnt_r, const float* fake, int64_t cnt_f,
                                     float* dreal, float* dfake, void* stream) {
    SCREAM_REQUIRE(dout && real && fake && dreal && dfake && cnt_r > 0 && cnt_f > 0, SCREAM_EINVAL);
    loss_d_bwd_kernel<<<blocks_of(cnt_r > cnt_f ? cnt_r : cnt_f), 256, 0, as_stream(stream)>>>(dout, real, cnt_r, fake, cnt_f, dreal, dfake);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_pairs_transform(const float* xyz, const float* rot, const float* trans, const int32_t* tile_cloud,
                                      int32_t n_pairs, int64_t rows_src, float* out, void* stream) {
    SCREAM_REQUIRE(xyz && rot && trans && tile_cloud && out && n_pairs > 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(rows_src > 0 && rows_src % SCREAM_ROW_TILE == 0 && rows_src <= INT32_MAX, SCREAM_EINVAL);
    pairs_transform_kernel<<<blocks_of(rows_src), 256, 0, as_stream(stream)>>>(xyz, rot, trans, tile_cloud, n_pairs, rows_src, out);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t scream_gan_workspace_bytes(int32_t n, int32_t cin, int32_t ndf, int32_t h, int32_t w) {
    Net net;
    if (!make_net(n, cin, ndf, h, w, net)) return -1;
    int64_t bytes;
    carve_net(nullptr, net, &bytes);
    return bytes;
}

static bool params_ok(const scream_gan_params_t* p) {
    if (!p || !p->b0 || !p->b4) return false;
    for (int l = 0; l < 5; ++l)
        if (!p->w[l] || !aligned16(p->w[l])) return false;
    for (int l = 0; l < 3; ++l)
        if (!p->gamma[l] || !p->beta[l] || !p->running_mean[l] || !p->running_var[l]) return false;
    return true;
}

extern "C" int scream_gan_forward(const float* x, const scream_gan_params_t* p, int32_t n, int32_t cin, int32_t ndf, int32_t h,
                                  int32_t w, int32_t training, float* logits, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    Net net;
    SCREAM_REQUIRE(make_net(n, cin, ndf, h, w, net), SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(x && logits && params_ok(p) && workspace && aligned16(workspace), SCREAM_EINVAL);
    int64_t bytes;
    const NetWs ws = carve_net(workspace, net, &bytes);
    SCREAM_REQUIRE(workspace_bytes >= bytes, SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    if (int rc = conv_run(FWD, net.L[0], p->w[0], x, ws.a1, p->b0, 1, nullptr, ws.scratch, ws.scratch_floats, st)) return rc;
    const float* in = ws.a1;
    for (int l = 1; l < 4; ++l) {
        const Geo& g = net.L[l];
        if (int rc = conv_run(FWD, g, p->w[l], in, ws.x[l - 1], nullptr, 0, nullptr, ws.scratch, ws.scratch_floats, st)) return rc;
        if (int rc = bn_fwd_run(ws.x[l - 1], p->gamma[l - 1], p->beta[l - 1], p->running_mean[l - 1], p->running_var[l - 1],
                                p->num_batches_tracked[l - 1], g.N, g.Cout, g.Ho * g.Wo, training, ws.a[l - 1], ws.mean[l - 1],
                                ws.invstd[l - 1], st))
            return rc;
        in = ws.a[l - 1];
    }
    return conv_run(FWD, net.L[4], p->w[4], in, logits, p->b4, 0, nullptr, ws.scratch, ws.scratch_floats, st);
}

extern "C" int scream_gan_backward(const float* dlogits, const float* x, const scream_gan_params_t* p, int32_t n, int32_t cin,
                                   int32_t ndf, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, float* dx,
                                   const scream_gan_grads_t* grads, void* stream) {
    Net net;
    SCREAM_REQUIRE(make_net(n, cin, ndf, h, w, net), SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(dlogits && x && params_ok(p) && workspace && aligned16(workspace), SCREAM_EINVAL);
    if (grads) {
        SCREAM_REQUIRE(grads->b0 && grads->b4, SCREAM_EINVAL);
        for (int l = 0; l < 5; ++l) SCREAM_REQUIRE(grads->w[l], SCREAM_EINVAL);
        for (int l = 0; l < 3; ++l) SCREAM_REQUIRE(grads->gamma[l] && grads->beta[l], SCREAM_EINVAL);
    }
    int64_t bytes;
    const NetWs ws = carve_net(workspace, net, &bytes);
    SCREAM_REQUIRE(workspace_bytes >= bytes, SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    float* S = ws.scratch;
    const int64_t SF = ws.scratch_floats;
    // layer 5: dlogits -> d a4
    if (grads) {
        if (int rc = conv_run(WGRAD, net.L[4], dlogits, ws.a[2], grads->w[4], nullptr, 0, nullptr, S, SF, st)) return rc;
        bias_sum_kernel<<<1, 256, 0, st>>>(dlogits, n, 1, net.L[4].Ho * net.L[4].Wo, grads->b4);
        SCREAM_LAUNCH_CHECK();
    }
    if (int rc = conv_run(DGRAD, net.L[4], p->w[4], dlogits, ws.ga, nullptr, 0, nullptr, S, SF, st)) return rc;
    // layers 4 .. 2: BatchNorm + leaky backward in place (ga), weight gradient, data gradient (ga -> gb), swap
    float *cur = ws.ga, *other = ws.gb;
    for (int l = 3; l >= 1; --l) {
        const Geo& g = net.L[l];
        if (int rc = bn_bwd_run(cur, ws.a[l - 1], ws.x[l - 1], p->gamma[l - 1], ws.mean[l - 1], ws.invstd[l - 1], g.N, g.Cout,
                                g.Ho * g.Wo, ws.sums, cur, grads ? grads->gamma[l - 1] : nullptr, grads ? grads->beta[l - 1] : nullptr, st))
            return rc;
        const float* in = l == 1 ? ws.a1 : ws.a[l - 2];
        if (grads)
            if (int rc = conv_run(WGRAD, g, cur, in, grads->w[l], nullptr, 0, nullptr, S, SF, st)) return rc;
        // the first layer's LeakyReLU rides in the finish of the second layer's data gradient
        if (int rc = conv_run(DGRAD, g, p->w[l], cur, other, nullptr, 0, l == 1 ? ws.a1 : nullptr, S, SF, st)) return rc;
        float* t = cur;
        cur = other, other = t;
    }
    if (grads) {
        if (int rc = conv_run(WGRAD, net.L[0], cur, x, grads->w[0], nullptr, 0, nullptr, S, SF, st)) return rc;
        bias_sum_kernel<<<ndf, 256, 0, st>>>(cur, n, ndf, net.L[0].Ho * net.L[0].Wo, grads->b0);
        SCREAM_LAUNCH_CHECK();
    }
    if (dx)
        if (int rc = conv_run(DGRAD, net.L[0], p->w[0], cur, dx, nullptr, 0, nullptr, S, SF, st)) return rc;
    return 0;
}
