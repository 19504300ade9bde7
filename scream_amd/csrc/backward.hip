// Backward pass of PointTransformer (training).  scream_amd/train.py composes these with the forward's GEMMs (data gradients
// dX = dY W run on transposed weights) into the gradient of every parameter.  Everything here is fp32 arithmetic; the weight
// gradient exists twice: on the fp32-input MFMA (train_backend "f32") and, fp32-accurate by operand splitting (split.h), on the
// bf16 matrix cores (train_backend "split").
//
// Every reduction here is deterministic: a kernel writes fixed-order partial sums into a slab with ordinary vector
// stores, and a second launch adds the slab's entries in index order.  No float atomics, so two identical calls give
// bitwise identical gradients.  Padded rows (clouds start on 128-row boundaries) carry zero gradient: the attention
// backward writes zeros there, and everything else is row-wise, so zeros propagate.
#include "common.h"
#include "split.h"
#include "wgrad.h"

namespace {

constexpr int D = SCREAM_D_MODEL;         // 256
constexpr int HD = SCREAM_HEAD_DIM;       // 32
constexpr int NH = SCREAM_NHEAD;          // 8
constexpr int KV_ELEMS = (HD + 1) * HD;   // 1056 floats per head: 32 x 32 and a row of 32
constexpr int CHUNK = SCREAM_KV_CHUNK;    // 256 query tokens per partial of the attention reduction

__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// ------------------------------------------------------------------------------------------------ weight gradient
// dW[N,K] = sum_r dY[r,:]^T X[r,:].  Block tile 128 (N) x 128 (K), 4 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32);
// blockIdx.y is a slice of rows.  Per 32-row chunk both operands are staged TRANSPOSED in LDS ([column][row], rows
// padded to 36), so that with the row as the MFMA's contraction index lane (i, half) reads rows 4 half .. 4 half + 3 of
// an 8-row group as one ds_read_b128 for its column i: four reads feed sixteen v_mfma_f32_32x32x2_f32.  The next chunk's
// global loads are issued before the current chunk's MFMAs.  Each slice writes its 128 x 128 partial; wgrad_reduce adds
// the slices in order.
constexpr int WG_LD = WG_R + 4;

__global__ __launch_bounds__(256) void wgrad_partial_kernel(const float* __restrict__ dY, int64_t ldy,
                                                            const float* __restrict__ X, int64_t ldx, int64_t rows,
                                                            int N, int K, int64_t slice_rows, float* __restrict__ part,
                                                            float* __restrict__ colpart) {
    __shared__ __attribute__((aligned(16))) float sA[WG_T * WG_LD];
    __shared__ __attribute__((aligned(16))) float sB[WG_T * WG_LD];
    const int kt = K / WG_T;
    const int n0 = (blockIdx.x / kt) * WG_T, k0 = (blockIdx.x % kt) * WG_T;
    const int64_t r_begin = (int64_t)blockIdx.y * slice_rows;
    const int64_t r_end = min(rows, r_begin + slice_rows);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wk = wave & 1, i = lane & 31, half = lane >> 5;
    const bool do_col = colpart != nullptr && k0 == 0;

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    float csum = 0.f;

    // loads: float4 f = tid + 256 u of a 32 x 128 chunk -> row f >> 5, columns 4 (f & 31) .. + 3
    f32x4 ra[4], rb[4];
    auto load = [&](int64_t r0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + 256 * u;
            const int64_t row = r0 + (f >> 5);
            const int c = (f & 31) * 4;
            const bool ok = row < r_end;
            ra[u] = ok ? ld4(dY + row * ldy + n0 + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[u] = ok ? ld4(X + row * ldx + k0 + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    if (r_begin < r_end) load(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += WG_R) {
        __syncthreads();  // the previous chunk's reads are done
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = tid + 256 * u;
            const int rr = f >> 5, c = (f & 31) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sA[(c + j) * WG_LD + rr] = ra[u][j];
                sB[(c + j) * WG_LD + rr] = rb[u][j];
            }
        }
        __syncthreads();
        if (r0 + WG_R < r_end) load(r0 + WG_R);
        if (do_col && tid < WG_T) {
#pragma unroll
            for (int rr = 0; rr < WG_R; rr += 4) {
                const f32x4 v = ld4(sA + tid * WG_LD + rr);
                csum += ((v[0] + v[1]) + (v[2] + v[3]));
            }
        }
#pragma unroll
        for (int g = 0; g < WG_R / 8; ++g) {
            f32x4 fa[2], fb[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[t] = ld4(sA + (wn * 64 + t * 32 + i) * WG_LD + g * 8 + half * 4);
                fb[t] = ld4(sB + (wk * 64 + t * 32 + i) * WG_LD + g * 8 + half * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a][j], fb[b][j], acc[a][b], 0, 0, 0);
        }
    }
    // acc[a][b][e] = dW[n0 + 64 wn + 32 a + mfma32_row(e, half)][k0 + 64 wk + 32 b + i]
    float* out = part + (int64_t)blockIdx.y * N * K;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                out[(int64_t)(n0 + wn * 64 + a * 32 + mfma32_row(e, half)) * K + k0 + wk * 64 + b * 32 + i] = acc[a][b][e];
    if (do_col && tid < WG_T) colpart[(int64_t)blockIdx.y * N + n0 + tid] = csum;
}

// ------------------------------------------------------------------------------------------------ LayerNorm
// One wave per row, lane owns features 4 lane .. 4 lane + 3 (as scream_pe_embed_ln).
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ y, float* __restrict__ mean_out,
                                                     float* __restrict__ rstd_out, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int f0 = 4 * lane;
    f32x4 v = ld4(a + row * D + f0);
    if (b) v += ld4(b + row * D + f0);
    const float mean = wave_sum((v[0] + v[1]) + (v[2] + v[3])) * (1.0f / D);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) q += (v[k] - mean) * (v[k] - mean);
    const float rstd = 1.0f / sqrtf(wave_sum(q) * (1.0f / D) + 1e-5f);
    const f32x4 g = ld4(gamma + f0), be = ld4(beta + f0);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (v[k] - mean) * rstd * g[k] + be[k];
    st4(y + row * D + f0, o);
    if (lane == 0) {
        mean_out[row] = mean;
        rstd_out[row] = rstd;
    }
}

constexpr int LN_ROWS = 512;  // rows per block of the LayerNorm backward (one partial of dgamma / dbeta each)

// dz = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy, xhat = (a + b - mean) rstd recomputed from the inputs.
// dz is written; dsum (optional) receives dsum += dz.  part[block] = { sum dy xhat [256], sum dy [256] } over the block's
// rows in a fixed order (per wave in row order, then the four waves in order).
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ a,
                                                     const float* __restrict__ b, const float* __restrict__ mean_in,
                                                     const float* __restrict__ rstd_in, const float* __restrict__ gamma,
                                                     float* __restrict__ dz, float* __restrict__ dsum, int64_t rows,
                                                     float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[4][2 * D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f0 = 4 * lane;
    const f32x4 g = ld4(gamma + f0);
    f32x4 sgx = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f};
    const int64_t r_begin = (int64_t)blockIdx.x * LN_ROWS;
    const int64_t r_end = min(rows, r_begin + LN_ROWS);
    for (int64_t row = r_begin + wave; row < r_end; row += 4) {
        f32x4 v = ld4(a + row * D + f0);
        if (b) v += ld4(b + row * D + f0);
        const f32x4 d = ld4(dy + row * D + f0);
        const float mean = mean_in[row], rstd = rstd_in[row];
        f32x4 xh, gg;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xh[k] = (v[k] - mean) * rstd;
            gg[k] = g[k] * d[k];
            s1 += gg[k];
            s2 += gg[k] * xh[k];
            sgx[k] += d[k] * xh[k];
            sg[k] += d[k];
        }
        const float mg = wave_sum(s1) * (1.0f / D), mgx = wave_sum(s2) * (1.0f / D);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = rstd * ((gg[k] - mg) - xh[k] * mgx);
        st4(dz + row * D + f0, o);
        if (dsum) st4(dsum + row * D + f0, ld4(dsum + row * D + f0) + o);
    }
    st4(&red[wave][f0], sgx);
    st4(&red[wave][D + f0], sg);
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * D; c += 256)
        part[(int64_t)blockIdx.x * 2 * D + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// dgamma / dbeta (+)= sum of the blocks' partials in block order.  One block of 512 threads.
__global__ __launch_bounds__(512) void ln_param_reduce_kernel(const float* __restrict__ part, int n_blocks,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              int accumulate) {
    const int c = threadIdx.x;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int q = 0;
    for (; q + 4 <= n_blocks; q += 4)
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += part[(int64_t)(q + u) * 2 * D + c];
    for (int u = 0; q + u < n_blocks; ++u) s[u] += part[(int64_t)(q + u) * 2 * D + c];
    const float t = (s[0] + s[1]) + (s[2] + s[3]);
    float* o = c < D ? dgamma + c : dbeta + (c - D);
    *o = accumulate ? *o + t : t;
}

// ------------------------------------------------------------------------------------------------ linear attention
// Forward (scream_kv_reduce / scream_attn_apply): Q' = elu(q) + 1, K', V; S = key cloud length; KV = K'^T (V / S),
// ks = sum K'; Z_l = 1 / (Q'_l . ks + 1e-6); O_l = S Z_l Q'_l KV.  Backward, per (query cloud, head):
//   dKV = sum_l S Z_l Q'_l^T dO_l,   dks = -sum_l Z_l (dO_l . O_l) Q'_l                          (phase 1, reduction)
//   dQ'_l = S Z_l dO_l KV^T - Z_l (dO_l . O_l) ks,   dK'_s = (V_s / S) dKV^T + dks,   dV_s = K'_s dKV / S   (phase 2)
//   dq = dQ' min(Q', 1), dk = dK' min(K', 1)  (elu + 1 backward from its output).

// Phase 1: grid (max_chunks, n_q), block 512 = one wave per head; lane = (d, half), two tokens per MFMA as in
// kv_partial_kernel.  part [n_q][max_chunks][8][1056]: dKV as [d][v], then dks[d].
__global__ __launch_bounds__(512) void attn_bwd_partial_kernel(const float* __restrict__ Qf, int64_t ldq, int64_t q_row_base,
                                                               const float* __restrict__ O, const float* __restrict__ dO,
                                                               const float* __restrict__ kv, const int32_t* __restrict__ cloud_row0,
                                                               const int32_t* __restrict__ cloud_len, int q_cloud_begin,
                                                               int kv_cloud_offset, int max_chunks, float* __restrict__ part) {
    const int qc = q_cloud_begin + blockIdx.y, kvc = qc + kv_cloud_offset;
    const int len = cloud_len[qc];
    const int t0 = blockIdx.x * CHUNK;
    float* out = part + (((int64_t)blockIdx.y * max_chunks + blockIdx.x) * NH + (threadIdx.x >> 6)) * KV_ELEMS;
    const int lane = threadIdx.x & 63, h = threadIdx.x >> 6;
    const int d = lane & 31, half = lane >> 5;
    if (t0 >= len) {  // block-uniform: an empty chunk of a shorter cloud writes nothing; attn_bwd_final_kernel reads only the real chunks
        return;
    }
    const int t1 = min(len, t0 + CHUNK);
    const float S = (float)cloud_len[kvc];
    const float ksd = kv[((int64_t)kvc * NH + h) * KV_ELEMS + HD * HD + d];
    const int64_t r0 = (int64_t)cloud_row0[qc] - q_row_base;
    const float* qp = Qf + r0 * ldq + h * HD + d;
    const float* op = O + r0 * D + h * HD + d;
    const float* gp = dO + r0 * D + h * HD + d;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float dks = 0.f;
    for (int t = t0; t < t1; t += 8) {
        float q[4], o[4], g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tok = t + 2 * u + half;
            const bool ok = tok < t1;
            q[u] = ok ? qp[(int64_t)tok * ldq] : 0.f;
            o[u] = ok ? op[(int64_t)tok * D] : 0.f;
            g[u] = ok ? gp[(int64_t)tok * D] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float Z = 1.0f / (half_wave_sum(q[u] * ksd) + 1e-6f);
            const float go = half_wave_sum(g[u] * o[u]);
            // A[i = d][k = half] = S Z Q'[tok][d], B[k = half][j = v] = dO[tok][v]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32((S * Z) * q[u], g[u], acc, 0, 0, 0);
            dks -= (Z * go) * q[u];
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) out[mfma32_row(e, half) * HD + d] = acc[e];
    dks += __shfl_xor(dks, 32);
    if (half == 0) out[HD * HD + d] = dks;
}

// grid n_q * 8; block 256.  dkv[i][h] = sum of the cloud's chunks in chunk order.
__global__ __launch_bounds__(256) void attn_bwd_final_kernel(const float* __restrict__ part, const int32_t* __restrict__ cloud_len,
                                                             int q_cloud_begin, int max_chunks, float* __restrict__ dkv) {
    const int qi = blockIdx.x / NH, h = blockIdx.x % NH;
    const int n_chunks = (cloud_len[q_cloud_begin + qi] + CHUNK - 1) / CHUNK;
    const float* p = part + ((int64_t)qi * max_chunks * NH + h) * KV_ELEMS;
    float* o = dkv + ((int64_t)qi * NH + h) * KV_ELEMS;
    for (int i = threadIdx.x; i < KV_ELEMS; i += 256) {
        float s = 0.f;
        for (int c = 0; c < n_chunks; ++c) s += p[(int64_t)c * NH * KV_ELEMS + i];
        o[i] = s;
    }
}

// Phase 2, query rows: grid = query rows / 128, block 256, thread c = (h, d).  The 32 dO rows of a sub-tile are staged in
// LDS and read back as broadcasts (all lanes of a head read the same row segment).
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float* __restrict__ Qf, int64_t ldq, int64_t q_row_base,
                                                         const float* __restrict__ O, const float* __restrict__ dO,
                                                         const float* __restrict__ kv, const int32_t* __restrict__ tile_cloud,
                                                         const int32_t* __restrict__ cloud_row0,
                                                         const int32_t* __restrict__ cloud_len, int kv_cloud_offset,
                                                         float* __restrict__ dq, int64_t lddq) {
    __shared__ __attribute__((aligned(16))) float sg[32 * D];
    const int c = threadIdx.x, h = c >> 5, d = c & 31;
    const int qc = tile_cloud[blockIdx.x], kvc = qc + kv_cloud_offset;
    const int64_t tile_row = (int64_t)blockIdx.x * SCREAM_ROW_TILE;  // relative to q_row_base
    const int64_t first_pad = (int64_t)cloud_row0[qc] + cloud_len[qc] - q_row_base;
    const float S = (float)cloud_len[kvc];
    const float* kvh = kv + ((int64_t)kvc * NH + h) * KV_ELEMS;
    float KVd[HD];  // KV[d][v] (stored [v][d])
#pragma unroll
    for (int v = 0; v < HD; ++v) KVd[v] = kvh[v * HD + d];
    const float ksd = kvh[HD * HD + d];
    for (int sub = 0; sub < SCREAM_ROW_TILE; sub += 32) {
        __syncthreads();
        for (int rr = 0; rr < 32; ++rr) sg[rr * D + c] = dO[(tile_row + sub + rr) * D + c];
        __syncthreads();
        for (int rr = 0; rr < 32; ++rr) {
            const int64_t row = tile_row + sub + rr;
            const float q = Qf[row * ldq + c], o = O[row * D + c], g = sg[rr * D + c];
            const float Z = 1.0f / (half_wave_sum(q * ksd) + 1e-6f);
            const float go = half_wave_sum(g * o);
            float dot = 0.f;
#pragma unroll
            for (int v4 = 0; v4 < HD; v4 += 4) {
                const f32x4 gv = ld4(sg + rr * D + h * HD + v4);
                dot += gv[0] * KVd[v4] + gv[1] * KVd[v4 + 1] + gv[2] * KVd[v4 + 2] + gv[3] * KVd[v4 + 3];
            }
            const float dqp = (S * Z) * dot - (Z * go) * ksd;
            dq[row * lddq + c] = row < first_pad ? dqp * fminf(q, 1.0f) : 0.f;
        }
    }
}

// Phase 2, key rows: grid = key rows / 128, block 256, thread c = (h, j).  dKV row j and column j of the head in registers;
// K' and V rows staged in LDS.
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float* __restrict__ Kf, const float* __restrict__ Vf, int64_t ldkv,
                                                          int64_t kv_row_base, const float* __restrict__ dkv,
                                                          const int32_t* __restrict__ tile_cloud,
                                                          const int32_t* __restrict__ cloud_row0,
                                                          const int32_t* __restrict__ cloud_len, int q_cloud_begin,
                                                          int kv_cloud_offset, float* __restrict__ dk, float* __restrict__ dv,
                                                          int64_t lddkv) {
    __shared__ __attribute__((aligned(16))) float sk[32 * D];
    __shared__ __attribute__((aligned(16))) float sv[32 * D];
    const int c = threadIdx.x, h = c >> 5, j = c & 31;
    const int kc = tile_cloud[blockIdx.x];
    const int qi = kc - kv_cloud_offset - q_cloud_begin;
    const int64_t tile_row = (int64_t)blockIdx.x * SCREAM_ROW_TILE;
    const int64_t first_pad = (int64_t)cloud_row0[kc] + cloud_len[kc] - kv_row_base;
    const float inv_S = 1.0f / (float)cloud_len[kc];
    const float* g = dkv + ((int64_t)qi * NH + h) * KV_ELEMS;  // dKV [d][v], then dks[d]
    float rowj[HD], colj[HD];
#pragma unroll
    for (int t = 0; t < HD; ++t) {
        rowj[t] = g[j * HD + t];  // dKV[j][v = t]
        colj[t] = g[t * HD + j];  // dKV[d = t][j]
    }
    const float dksj = g[HD * HD + j];
    for (int sub = 0; sub < SCREAM_ROW_TILE; sub += 32) {
        __syncthreads();
        for (int rr = 0; rr < 32; ++rr) {
            const int64_t row = tile_row + sub + rr;
            sk[rr * D + c] = Kf[row * ldkv + c];
            sv[rr * D + c] = Vf[row * ldkv + c];
        }
        __syncthreads();
        for (int rr = 0; rr < 32; ++rr) {
            const int64_t row = tile_row + sub + rr;
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int t4 = 0; t4 < HD; t4 += 4) {
                const f32x4 vv = ld4(sv + rr * D + h * HD + t4), kk = ld4(sk + rr * D + h * HD + t4);
                a += vv[0] * rowj[t4] + vv[1] * rowj[t4 + 1] + vv[2] * rowj[t4 + 2] + vv[3] * rowj[t4 + 3];
                b += kk[0] * colj[t4] + kk[1] * colj[t4 + 1] + kk[2] * colj[t4 + 2] + kk[3] * colj[t4 + 3];
            }
            const bool real = row < first_pad;
            const float kp = sk[rr * D + c];
            dk[row * lddkv + c] = real ? (a * inv_S + dksj) * fminf(kp, 1.0f) : 0.f;
            dv[row * lddkv + c] = real ? b * inv_S : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ small kernels
// dy[i] = y[i] > 0 ? dy[i] : 0 (relu backward from the relu's output)
__global__ __launch_bounds__(256) void relu_bwd_kernel(float* __restrict__ dy, const float* __restrict__ y, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 g = ld4(dy + 4 * i);
        const f32x4 v = ld4(y + 4 * i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = v[k] > 0.f ? g[k] : 0.f;
        st4(dy + 4 * i, g);
    }
}

__global__ __launch_bounds__(256) void add_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        st4(y + 4 * i, ld4(y + 4 * i) + ld4(x + 4 * i));
}

// out[C][R] = in[R][C] through a 32 x 33 LDS tile; grid (ceil(C / 32), ceil(R / 32)), block 32 x 8.
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int R, int C, float* __restrict__ out) {
    __shared__ float t[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = y; k < 32; k += 8)
        if (r0 + k < R && c0 + x < C) t[k][x] = in[(int64_t)(r0 + k) * C + c0 + x];
    __syncthreads();
    for (int k = y; k < 32; k += 8)
        if (c0 + k < C && r0 + x < R) out[(int64_t)(c0 + k) * R + r0 + x] = t[x][k];
}

// coor_mlp head backward (data): dH[r,k] = (H[r,k] > 0) sum_j dOut[r,j] W[j,k] -- the relu of coor_mlp.3 folded in.
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ W,
                                                       const float* __restrict__ H, float* __restrict__ dH, int64_t rows) {
    const int lane = threadIdx.x & 63;
    const int f0 = 4 * lane;
    const f32x4 w0 = ld4(W + f0), w1 = ld4(W + D + f0), w2 = ld4(W + 2 * D + f0);
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
        const float g0 = dout[row * 3], g1 = dout[row * 3 + 1], g2 = dout[row * 3 + 2];
        const f32x4 hv = ld4(H + row * D + f0);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = hv[k] > 0.f ? (g0 * w0[k] + g1 * w1[k]) + g2 * w2[k] : 0.f;
        st4(dH + row * D + f0, o);
    }
}

constexpr int SK_ROWS = 512;                // rows per block of the 3-wide gradient reductions
constexpr int SK_PART = 3 * D + D + 4;      // per block: P[3][256], colsum of the wide operand [256], of the narrow one [3] (+1)

// P[j][k] = sum_r s[r][j] w[r][k] for a 256-wide operand w and a 3-wide operand s, plus both column sums.  The narrow
// operand is either given ([rows, 3]) or, for the embedding, xyz - center[cloud of the row].  Thread k owns column k.
__global__ __launch_bounds__(256) void skinny_partial_kernel(const float* __restrict__ w, const float* __restrict__ s,
                                                             const float* __restrict__ center,
                                                             const int32_t* __restrict__ tile_cloud, int64_t rows,
                                                             float* __restrict__ part) {
    const int k = threadIdx.x;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, cw = 0.f;
    // The narrow operand's column sums in double: for coor_mlp.4.bias they add the L1 loss's gradient, +-1/N per row, and where
    // the prediction lies to one side of its target every term is the same number: a running fp32 sum then rounds the same
    // way at every step (5.3e-6 relative over 512 rows of 1/2000, measured) instead of averaging out.
    double cs0 = 0.0, cs1 = 0.0, cs2 = 0.0;
    const int64_t r_begin = (int64_t)blockIdx.x * SK_ROWS;
    const int64_t r_end = min(rows, r_begin + SK_ROWS);
    for (int64_t r = r_begin; r < r_end; ++r) {
        float s0 = s[r * 3], s1 = s[r * 3 + 1], s2 = s[r * 3 + 2];
        if (center) {
            const int cl = tile_cloud[r / SCREAM_ROW_TILE];
            s0 -= center[cl * 3];
            s1 -= center[cl * 3 + 1];
            s2 -= center[cl * 3 + 2];
        }
        const float x = w[r * D + k];
        p0 += s0 * x;
        p1 += s1 * x;
        p2 += s2 * x;
        cw += x;
        cs0 += s0;
        cs1 += s1;
        cs2 += s2;
    }
    float* o = part + (int64_t)blockIdx.x * SK_PART;
    o[k] = p0;
    o[D + k] = p1;
    o[2 * D + k] = p2;
    o[3 * D + k] = cw;
    if (k == 0) {
        o[4 * D] = (float)cs0;
        o[4 * D + 1] = (float)cs1;
        o[4 * D + 2] = (float)cs2;
    }
}

// Sum of the blocks' partials in block order.  transpose_w: write P as [256][3] (the embedding's weight) instead of [3][256].
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* __restrict__ part, int n_blocks, float* __restrict__ dW,
                                                            int transpose_w, float* __restrict__ col_w,
                                                            float* __restrict__ col_s, int accumulate) {
    for (int i = threadIdx.x + blockIdx.x * 256; i < 4 * D + 3; i += gridDim.x * 256) {
        float t = 0.f;
        if (i < 4 * D) {
            for (int q = 0; q < n_blocks; ++q) t += part[(int64_t)q * SK_PART + i];
        } else {  // col_s: equal partials round one way too (skinny_partial_kernel); still a fixed-order sum
            double td = 0.0;
            for (int q = 0; q < n_blocks; ++q) td += (double)part[(int64_t)q * SK_PART + i];
            t = (float)td;
        }
        float* o = nullptr;
        if (i < 3 * D) o = dW ? dW + (transpose_w ? (i % D) * 3 + i / D : i) : nullptr;
        else if (i < 4 * D) o = col_w ? col_w + (i - 3 * D) : nullptr;
        else o = col_s ? col_s + (i - 4 * D) : nullptr;
        if (o) *o = accumulate ? *o + t : t;
    }
}

unsigned grid_for(int64_t n, int64_t per_block, int64_t cap) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

// THE workspace of the attention backward, a head block per entry: part [n_q_clouds][max_chunks][NH][KV_ELEMS], the chunk
// partials, then dkv [n_q_clouds][NH][KV_ELEMS], their sums.  Returns the bytes; from a null base it only measures.
int64_t attn_bwd_carve(void* base, int32_t n_q_clouds, int32_t max_chunks, float** part, float** dkv) {
    Carver cv{base};
    *part = cv.take<float>((int64_t)n_q_clouds * max_chunks * NH * KV_ELEMS);
    *dkv = cv.take<float>((int64_t)n_q_clouds * NH * KV_ELEMS);
    return cv.used;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int64_t scream_wgrad_workspace_bytes(int64_t rows, int32_t N, int32_t K) {
    if (rows < 0 || N <= 0 || K <= 0 || N % WG_T || K % WG_T) return -1;
    return wgrad_carve(nullptr, rows, N, K).bytes;
}

extern "C" int scream_gemm_wgrad_f32(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N,
                                     int32_t K, float* dW, int32_t accumulate, float* colsum, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
    return wgrad_run<wgrad_partial_kernel>(dY, ldy, X, ldx, rows, N, K, dW, accumulate, colsum, workspace, workspace_bytes, stream);
}

extern "C" int64_t scream_wgrad_split_workspace_bytes(int64_t rows, int32_t N, int32_t K) {
    return scream_wgrad_workspace_bytes(rows, N, K);  // the same row slices and slabs
}

extern "C" int scream_gemm_wgrad_split_f32(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N,
                                           int32_t K, float* dW, int32_t accumulate, float* colsum, int32_t split,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(split_valid(split) && !split_fp16(split), SCREAM_EINVAL);  // built for bf16 x 3 only
    return wgrad_run<wgrad_split_partial_kernel<SplitBf3>>(dY, ldy, X, ldx, rows, N, K, dW, accumulate, colsum, workspace,
                                                           workspace_bytes, stream);
}

extern "C" int scream_ln_fwd(const float* a, const float* b, const float* gamma, const float* beta, float* y, float* mean,
                             float* rstd, int64_t rows, void* stream) {
    SCREAM_REQUIRE(a && gamma && beta && y && mean && rstd, SCREAM_EINVAL);
    SCREAM_REQUIRE(rows >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(a) && (!b || aligned16(b)) && aligned16(y) && aligned16(gamma) && aligned16(beta), SCREAM_EINVAL);
    if (rows == 0) return 0;
    SCREAM_REQUIRE((rows + 3) / 4 < (1ll << 31), SCREAM_EUNSUPPORTED);
    ln_fwd_kernel<<<dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, as_stream(stream)>>>(a, b, gamma, beta, y, mean, rstd, rows);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t scream_ln_bwd_workspace_bytes(int64_t rows) {
    if (rows < 0) return -1;
    return ((rows + LN_ROWS - 1) / LN_ROWS) * 2 * D * (int64_t)sizeof(float);
}

extern "C" int scream_ln_bwd(const float* dy, const float* a, const float* b, const float* mean, const float* rstd,
                             const float* gamma, float* dz, float* dsum, float* dgamma, float* dbeta, int32_t accumulate,
                             int64_t rows, void* workspace, int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(dy && a && mean && rstd && gamma && dz && dgamma && dbeta, SCREAM_EINVAL);
    SCREAM_REQUIRE(rows >= 0, SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(dy) && aligned16(a) && (!b || aligned16(b)) && aligned16(dz) && (!dsum || aligned16(dsum)) &&
                       aligned16(gamma), SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    const int64_t blocks = (rows + LN_ROWS - 1) / LN_ROWS;
    if (blocks == 0) {
        if (!accumulate) {
            if (hipMemsetAsync(dgamma, 0, D * sizeof(float), st) != hipSuccess) return SCREAM_EINVAL;
            if (hipMemsetAsync(dbeta, 0, D * sizeof(float), st) != hipSuccess) return SCREAM_EINVAL;
        }
        return 0;
    }
    SCREAM_REQUIRE(workspace && workspace_bytes >= scream_ln_bwd_workspace_bytes(rows) && aligned16(workspace), SCREAM_EINVAL);
    SCREAM_REQUIRE(blocks < (1ll << 31), SCREAM_EUNSUPPORTED);
    float* part = static_cast<float*>(workspace);
    ln_bwd_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(dy, a, b, mean, rstd, gamma, dz, dsum, rows, part);
    SCREAM_LAUNCH_CHECK();
    ln_param_reduce_kernel<<<dim3(1), dim3(512), 0, st>>>(part, (int)blocks, dgamma, dbeta, accumulate);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t scream_attn_bwd_workspace_bytes(int32_t n_q_clouds, int32_t max_chunks) {
    if (n_q_clouds < 0 || max_chunks < 1) return -1;
    float *part, *dkv;
    return attn_bwd_carve(nullptr, n_q_clouds, max_chunks, &part, &dkv);
}

extern "C" int scream_attn_bwd(const float* Qf, int64_t ldq, int64_t q_rows, int64_t q_row_base, const float* O,
                               const float* dO, const float* Kf, const float* Vf, int64_t ldkv, int64_t kv_rows,
                               int64_t kv_row_base, const float* kv, const int32_t* tile_cloud, const int32_t* cloud_row0,
                               const int32_t* cloud_len, int32_t q_cloud_begin, int32_t n_q_clouds, int32_t kv_cloud_offset,
                               int32_t max_chunks, float* dq, int64_t lddq, float* dk, float* dv, int64_t lddkv,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(Qf && O && dO && Kf && Vf && kv && tile_cloud && cloud_row0 && cloud_len && dq && dk && dv, SCREAM_EINVAL);
    SCREAM_REQUIRE(q_rows >= 0 && kv_rows >= 0 && q_rows % SCREAM_ROW_TILE == 0 && kv_rows % SCREAM_ROW_TILE == 0 &&
                       q_row_base % SCREAM_ROW_TILE == 0 && kv_row_base % SCREAM_ROW_TILE == 0, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(ldq >= D && ldkv >= D && lddq >= D && lddkv >= D && n_q_clouds >= 0 && q_cloud_begin >= 0 && max_chunks >= 1,
                   SCREAM_EINVAL);
    SCREAM_REQUIRE(n_q_clouds <= 65535, SCREAM_EUNSUPPORTED);
    if (n_q_clouds == 0) return 0;
    float *part, *dkv;
    const int64_t need = attn_bwd_carve(workspace, n_q_clouds, max_chunks, &part, &dkv);
    SCREAM_REQUIRE(workspace && aligned16(workspace) && workspace_bytes >= need, SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    attn_bwd_partial_kernel<<<dim3(max_chunks, n_q_clouds), dim3(512), 0, st>>>(Qf, ldq, q_row_base, O, dO, kv, cloud_row0, cloud_len,
                                                                                q_cloud_begin, kv_cloud_offset, max_chunks, part);
    SCREAM_LAUNCH_CHECK();
    attn_bwd_final_kernel<<<dim3(n_q_clouds * NH), dim3(256), 0, st>>>(part, cloud_len, q_cloud_begin, max_chunks, dkv);
    SCREAM_LAUNCH_CHECK();
    if (q_rows)
        attn_bwd_q_kernel<<<dim3((unsigned)(q_rows / SCREAM_ROW_TILE)), dim3(256), 0, st>>>(
            Qf, ldq, q_row_base, O, dO, kv, tile_cloud + q_row_base / SCREAM_ROW_TILE, cloud_row0, cloud_len, kv_cloud_offset, dq, lddq);
    SCREAM_LAUNCH_CHECK();
    if (kv_rows)
        attn_bwd_kv_kernel<<<dim3((unsigned)(kv_rows / SCREAM_ROW_TILE)), dim3(256), 0, st>>>(
            Kf, Vf, ldkv, kv_row_base, dkv, tile_cloud + kv_row_base / SCREAM_ROW_TILE, cloud_row0, cloud_len, q_cloud_begin,
            kv_cloud_offset, dk, dv, lddkv);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_relu_bwd(float* dy, const float* y, int64_t n, void* stream) {
    SCREAM_REQUIRE(dy && y && n >= 0 && n % 4 == 0 && aligned16(dy) && aligned16(y), SCREAM_EINVAL);
    if (n == 0) return 0;
    relu_bwd_kernel<<<dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, as_stream(stream)>>>(dy, y, n / 4);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_add_f32(float* y, const float* x, int64_t n, void* stream) {
    SCREAM_REQUIRE(y && x && n >= 0 && n % 4 == 0 && aligned16(y) && aligned16(x), SCREAM_EINVAL);
    if (n == 0) return 0;
    add_kernel<<<dim3(grid_for(n / 4, 256, 4096)), dim3(256), 0, as_stream(stream)>>>(y, x, n / 4);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_transpose_f32(const float* in, int32_t R, int32_t C, float* out, void* stream) {
    SCREAM_REQUIRE(in && out && R >= 0 && C >= 0, SCREAM_EINVAL);
    if (R == 0 || C == 0) return 0;
    transpose_kernel<<<dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, as_stream(stream)>>>(in, R, C, out);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_coor_head_bwd(const float* dout, const float* W, const float* H, float* dH, int64_t rows, void* stream) {
    SCREAM_REQUIRE(dout && W && H && dH && rows >= 0 && aligned16(W) && aligned16(H) && aligned16(dH), SCREAM_EINVAL);
    if (rows == 0) return 0;
    head_bwd_kernel<<<dim3(grid_for(rows, 4, 2048)), dim3(256), 0, as_stream(stream)>>>(dout, W, H, dH, rows);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t scream_grad3_workspace_bytes(int64_t rows) {
    if (rows < 0) return -1;
    return ((rows + SK_ROWS - 1) / SK_ROWS) * SK_PART * (int64_t)sizeof(float);
}

extern "C" int scream_grad3(const float* w, const float* s, const float* center, const int32_t* tile_cloud, int64_t rows,
                            float* dW, int32_t transpose_w, float* col_w, float* col_s, int32_t accumulate, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(w && s && (!center || tile_cloud) && rows >= 0, SCREAM_EINVAL);
    const int64_t blocks = (rows + SK_ROWS - 1) / SK_ROWS;
    SCREAM_REQUIRE(blocks > 0, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(blocks < (1ll << 31), SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(workspace && workspace_bytes >= scream_grad3_workspace_bytes(rows), SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    float* part = static_cast<float*>(workspace);
    skinny_partial_kernel<<<dim3((unsigned)blocks), dim3(256), 0, st>>>(w, s, center, tile_cloud, rows, part);
    SCREAM_LAUNCH_CHECK();
    skinny_reduce_kernel<<<dim3(5), dim3(256), 0, st>>>(part, (int)blocks, dW, transpose_w, col_w, col_s, accumulate);
    SCREAM_LAUNCH_CHECK();
    return 0;
}
