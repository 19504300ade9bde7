// Training-batch preparation and the packed L1 loss: what the reference does per pair on the host between the files and the
// model (datasets/three_d_match.py:129-153,175-192, datasets/kitti.py:233-273) and after it (models/pointnet.py:93-99,
// 163-167), for B pairs per launch.  include/scream_hip.h states the contract; tests/prep_ref.py restates it in numpy.
//
// Every step is ONE IEEE float64 operation on the stated operands (-ffp-contract=off), fp32 inputs are widened first, and every
// sum has a fixed order:
//   chunk sum   the rows of a cloud in 256-row chunks; inside a chunk  s = v[0]; s += v[1]; ...  in ascending row order
//   cloud sum   acc = chunk[0]; acc += chunk[1]; ...  in ascending chunk order (a union: source chunks first, then target chunks)
// One block per chunk writes its partial into the workspace; every block of the NEXT launch begins by summing its pair's partials
// in that order (the pattern of icp_iter_kernel).  No float atomics, no synchronisation between blocks inside a launch: a
// result depends on its own pair alone -- not on scheduling, not on what else is in the batch.
//
// 3x3 products, each element (x*y + x*y) + x*y in ascending inner index; a matrix applied to a point adds the translation last:
//   apply(R, t, x)_k = ((R[k][0]*x0 + R[k][1]*x1) + R[k][2]*x2) + t_k
//   m        = mean of the perturbed side's RAW cloud (cloud sum / n)
//   P'.R     = P.R;   P'.t_k = (P.t_k + m_k) - ((P.R[k][0]*m0 + P.R[k][1]*m1) + P.R[k][2]*m2)              (= C^-1 P C)
//   side 0   q_k = -((P.R[0][k]*P'.t0 + P.R[1][k]*P'.t1) + P.R[2][k]*P'.t2)                                 (P'^-1 = [P.R^T | q])
//            T'.R[i][j] = (T.R[i][0]*P.R[j][0] + T.R[i][1]*P.R[j][1]) + T.R[i][2]*P.R[j][2];  T'.t = apply(T.R, T.t, q)
//            a = apply(P.R, P'.t, x) on source rows, a = x on target rows
//   side 1   T'.R[i][j] = (P.R[i][0]*T.R[0][j] + P.R[i][1]*T.R[1][j]) + P.R[i][2]*T.R[2][j];  T'.t = apply(P.R, P'.t, T.t)
//            a = apply(P.R, P'.t, x) on target rows, a = x on source rows
//   noise    a_k = a_k + noise_std * z_k  on both clouds when noise_std > 0 (gauss3 below)
//   reg      = apply(T'.R, T'.t, a) on source rows, a on target rows
//   ball     c = union sum of reg / (N + M);  d = reg - c;  s = 1 / sqrt(max (d0*d0 + d1*d1) + d2*d2)
//   bbox     c = (lo + hi) / 2;  s = 1 / (max_k (hi_k - lo_k) / 2)
//   xyz      = fp32(s * (a - c));   rot = fp32(T'.R)
//   trans_k  = fp32(s * ((T'.t_k - c_k) + ((T'.R[k][0]*c0 + T'.R[k][1]*c1) + T'.R[k][2]*c2)))
// The augmented points are parked in the workspace as float64 [raw rows, 3] between the launches, so that the logarithm and
// the sine / cosine of the noise are evaluated once per coordinate.
// Non-finite coordinates and a union of zero extent (s is not finite) are outside the contract; nothing here looks for them.
#include <math.h>

#include "common.h"

namespace {

constexpr int PREP_CHUNK = 256;
constexpr int ROW_TILE = 128;  // a packed cloud is zero padded to this (scream_amd/packing.py)

inline int32_t n_chunks(int32_t max_len) { return (int32_t)(((int64_t)max_len + PREP_CHUNK - 1) / PREP_CHUNK); }

struct PrepWs {
    double* part_mean;  // [B][nchunk][3]   chunk sums of the perturbed side's raw cloud
    double* part_reg;   // [2B][nchunk][3]  chunk sums of reg
    double* part_lo;    // [2B][nchunk][3]  chunk bounds of reg
    double* part_hi;
    double* part_max;   // [2B][nchunk]     chunk maxima of |reg - c|^2
    double* part_cen;   // [B][nchunk][3]   chunk sums of the normalised source (centre rule 0)
    double* aug;        // [raw_rows][3]    the augmented points
};
// THE layout of a call, each piece with the element count stated above.  From a null base it only measures: *bytes is what
// scream_prep_pairs_workspace_bytes reports and what scream_prep_pairs asks for.
inline PrepWs prep_carve(void* workspace, int64_t raw_rows, int32_t n_pairs, int32_t max_len, int64_t* bytes) {
    const int64_t per_pair = (int64_t)n_pairs * n_chunks(max_len), per_cloud = 2 * per_pair;
    Carver w{workspace};
    PrepWs ws;
    ws.part_mean = w.take<double>(per_pair * 3);
    ws.part_reg = w.take<double>(per_cloud * 3);
    ws.part_lo = w.take<double>(per_cloud * 3);
    ws.part_hi = w.take<double>(per_cloud * 3);
    ws.part_max = w.take<double>(per_cloud);
    ws.part_cen = w.take<double>(per_pair * 3);
    ws.aug = w.take<double>(raw_rows * 3);
    *bytes = w.used;
    return ws;
}

struct PrepArgs {
    const void* raw;
    int32_t raw_is_f64;
    int64_t raw_rows;
    const int32_t* raw_row0;  // [2B] sources, then targets
    const int32_t* raw_len;
    int32_t max_len;
    const double* T;
    const double* perturb;
    const int32_t* side;
    double noise_std;
    uint64_t seed;
    const int64_t* sample_id;
    int32_t mode;  // 0 ball, 1 bbox
    int32_t center_rule;
    const int32_t* cloud_row0;  // [2B] packed
    int32_t n_pairs;
    int64_t rows_total;
    int32_t nchunk;
    PrepWs ws;
};

// the rows of pair p; a pair whose rows leave the arrays (or exceed max_len) has n = 0 on both sides: it reads and writes no row
struct Geo {
    int64_t raw0[2], pk0[2];
    int32_t n[2];
};
__device__ __forceinline__ int64_t pad_tile(int64_t n) { return (n + ROW_TILE - 1) / ROW_TILE * ROW_TILE; }
__device__ __forceinline__ Geo pair_geo(const PrepArgs& A, int p) {
    Geo g;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int cl = c * A.n_pairs + p;
        g.raw0[c] = A.raw_row0[cl];
        g.n[c] = A.raw_len[cl];
        g.pk0[c] = A.cloud_row0[cl];
        ok = ok && g.raw0[c] >= 0 && g.n[c] >= 0 && g.n[c] <= A.max_len && g.raw0[c] + g.n[c] <= A.raw_rows && g.pk0[c] >= 0 &&
             g.pk0[c] + pad_tile(g.n[c]) <= A.rows_total;
    }
    if (!ok) g.n[0] = g.n[1] = 0;
    return g;
}

__device__ __forceinline__ void load_raw(const PrepArgs& A, int64_t row, double x[3]) {
    if (A.raw_is_f64) {
        const double* r = reinterpret_cast<const double*>(A.raw) + row * 3;
        x[0] = r[0], x[1] = r[1], x[2] = r[2];
    } else {
        const float* r = reinterpret_cast<const float*>(A.raw) + row * 3;
        x[0] = (double)r[0], x[1] = (double)r[1], x[2] = (double)r[2];
    }
}

// THE chunk sum: out[k] = ((v_0[k] + v_1[k]) + ...) + v_{cnt-1}[k] over the block's first cnt threads (cnt >= 1); one wave per axis
__device__ __forceinline__ void chunk_sum3(double (*sh)[PREP_CHUNK], const double v[3], int cnt, double* out) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[0][t] = v[0], sh[1][t] = v[1], sh[2][t] = v[2];
    __syncthreads();
    if ((t & 63) == 0 && t < 192) {
        const int k = t >> 6;
        double s = sh[k][0];
        for (int i = 1; i < cnt; ++i) s += sh[k][i];
        out[k] = s;
    }
}
__device__ __forceinline__ void chunk_sum1(double (*sh)[PREP_CHUNK], double v, int cnt, double* out) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[0][t] = v;
    __syncthreads();
    if (t == 0) {
        double s = sh[0][0];
        for (int i = 1; i < cnt; ++i) s += sh[0][i];
        out[0] = s;
    }
}
// THE cloud sum of axis k over the first nc chunk partials, continuing from acc when cont is set
__device__ __forceinline__ double cloud_sum(const double* part, int nc, int k, int stride, double acc, bool cont) {
    for (int j = 0; j < nc; ++j) {
        const double v = part[(int64_t)j * stride + k];
        acc = (cont || j > 0) ? acc + v : v;
    }
    return acc;
}
__device__ __forceinline__ int chunks_of(int n) { return (n + PREP_CHUNK - 1) / PREP_CHUNK; }

__device__ __forceinline__ double apply_k(const double* R, const double* t, const double* x, int k) {
    return ((R[k * 3 + 0] * x[0] + R[k * 3 + 1] * x[1]) + R[k * 3 + 2] * x[2]) + t[k];
}
__device__ __forceinline__ double dot3_k(const double* R, const double* x, int k) {
    return (R[k * 3 + 0] * x[0] + R[k * 3 + 1] * x[1]) + R[k * 3 + 2] * x[2];
}

// ---- Philox4x32-10 (Salmon et al., SC'11) and the Box-Muller normals of the contract
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ void gauss3(uint64_t seed, int64_t sample_id, int cloud, int row, double z[3]) {
    uint32_t w[4] = {(uint32_t)row, (uint32_t)cloud, (uint32_t)(uint64_t)sample_id, (uint32_t)((uint64_t)sample_id >> 32)};
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double TWO_PI = 6.283185307179586, SCALE = 1.0 / 4294967296.0;
    const double u1 = ((double)w[0] + 0.5) * SCALE, u2 = ((double)w[1] + 0.5) * SCALE;
    const double u3 = ((double)w[2] + 0.5) * SCALE, u4 = ((double)w[3] + 0.5) * SCALE;
    const double r = sqrt(-2.0 * log(u1)), th = TWO_PI * u2;
    z[0] = r * cos(th);
    z[1] = r * sin(th);
    z[2] = sqrt(-2.0 * log(u3)) * cos(TWO_PI * u4);
}

// grid (nchunk, B): chunk sums of the perturbed side's raw cloud
__global__ __launch_bounds__(PREP_CHUNK) void prep_mean_kernel(PrepArgs A) {
    __shared__ double sh[3][PREP_CHUNK];
    const int p = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    const Geo g = pair_geo(A, p);
    const int c = A.side[p] != 0 ? 1 : 0;
    const int i = chunk * PREP_CHUNK + t, cnt = min(PREP_CHUNK, g.n[c] - chunk * PREP_CHUNK);
    if (cnt <= 0) return;
    double x[3] = {0.0, 0.0, 0.0};
    if (i < g.n[c]) load_raw(A, g.raw0[c] + i, x);
    chunk_sum3(sh, x, cnt, A.ws.part_mean + ((int64_t)p * A.nchunk + chunk) * 3);
}

struct Pose {
    double PR[9], Pt[3], TR[9], Tt[3];  // P' and T'
};

// grid (nchunk, 2B): perturb, add noise, park a, chunk sums / bounds of reg; the first source block of a pair writes T_aug
__global__ __launch_bounds__(PREP_CHUNK) void prep_augment_kernel(PrepArgs A, double* __restrict__ T_aug) {
    __shared__ double sh[3][PREP_CHUNK];
    __shared__ double m[3];
    __shared__ Pose pose;
    const int B = A.n_pairs, cl = blockIdx.y, c = cl >= B ? 1 : 0, p = cl - c * B, chunk = blockIdx.x, t = threadIdx.x;
    const Geo g = pair_geo(A, p);
    const int i = chunk * PREP_CHUNK + t, cnt = min(PREP_CHUNK, g.n[c] - chunk * PREP_CHUNK);
    if (cnt <= 0) return;
    const int sd = A.side[p] != 0 ? 1 : 0;
    if (t < 3) m[t] = cloud_sum(A.ws.part_mean + (int64_t)p * A.nchunk * 3, chunks_of(g.n[sd]), t, 3, 0.0, false) / (double)g.n[sd];
    __syncthreads();
    if (t == 0) {
        const double* T = A.T + (int64_t)p * 16;
        const double* P = A.perturb + (int64_t)p * 16;
        double TR[9], Tt[3], PR[9], Pt[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) TR[a * 3 + b] = T[a * 4 + b], PR[a * 3 + b] = P[a * 4 + b];
            Tt[a] = T[a * 4 + 3];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) Pt[k] = (P[k * 4 + 3] + m[k]) - dot3_k(PR, m, k);
        if (sd == 0) {
            double q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = -((PR[0 + k] * Pt[0] + PR[3 + k] * Pt[1]) + PR[6 + k] * Pt[2]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    pose.TR[a * 3 + b] = (TR[a * 3 + 0] * PR[b * 3 + 0] + TR[a * 3 + 1] * PR[b * 3 + 1]) + TR[a * 3 + 2] * PR[b * 3 + 2];
                pose.Tt[a] = apply_k(TR, Tt, q, a);
            }
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    pose.TR[a * 3 + b] = (PR[a * 3 + 0] * TR[0 + b] + PR[a * 3 + 1] * TR[3 + b]) + PR[a * 3 + 2] * TR[6 + b];
                pose.Tt[a] = apply_k(PR, Pt, Tt, a);
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) pose.PR[k] = PR[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) pose.Pt[k] = Pt[k];
        if (chunk == 0 && c == 0) {
            double* o = T_aug + (int64_t)p * 16;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) o[a * 4 + b] = pose.TR[a * 3 + b];
                o[a * 4 + 3] = pose.Tt[a];
            }
            o[12] = 0.0, o[13] = 0.0, o[14] = 0.0, o[15] = 1.0;
        }
    }
    __syncthreads();
    double reg[3] = {0.0, 0.0, 0.0};
    if (i < g.n[c]) {
        double x[3], a[3];
        load_raw(A, g.raw0[c] + i, x);
#pragma unroll
        for (int k = 0; k < 3; ++k) a[k] = c == sd ? apply_k(pose.PR, pose.Pt, x, k) : x[k];
        if (A.noise_std > 0.0) {
            double z[3];
            gauss3(A.seed, A.sample_id[p], c, i, z);
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = a[k] + A.noise_std * z[k];
        }
        double* o = A.ws.aug + (g.raw0[c] + i) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = a[k];
            reg[k] = c == 0 ? apply_k(pose.TR, pose.Tt, a, k) : a[k];
        }
    }
    const int64_t slot = ((int64_t)cl * A.nchunk + chunk) * 3;
    if (A.mode == 0) {
        chunk_sum3(sh, reg, cnt, A.ws.part_reg + slot);
    } else {
        __syncthreads();
        sh[0][t] = reg[0], sh[1][t] = reg[1], sh[2][t] = reg[2];
        __syncthreads();
        if ((t & 63) == 0 && t < 192) {
            const int k = t >> 6;
            double lo = sh[k][0], hi = sh[k][0];
            for (int j = 1; j < cnt; ++j) lo = fmin(lo, sh[k][j]), hi = fmax(hi, sh[k][j]);
            A.ws.part_lo[slot + k] = lo;
            A.ws.part_hi[slot + k] = hi;
        }
    }
}

// the registered point of a parked row
__device__ __forceinline__ void reg_of(const PrepArgs& A, const double* T4, int c, int64_t raw_row, double a[3], double reg[3]) {
    const double* o = A.ws.aug + raw_row * 3;
    a[0] = o[0], a[1] = o[1], a[2] = o[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        reg[k] = c == 0 ? ((T4[k * 4 + 0] * a[0] + T4[k * 4 + 1] * a[1]) + T4[k * 4 + 2] * a[2]) + T4[k * 4 + 3] : a[k];
}

// ball: c of pair p, by threads 0..2 into cs[0..2] (call with all threads; ends with a barrier)
__device__ __forceinline__ void ball_centre(const PrepArgs& A, const Geo& g, int p, double* cs) {
    const int t = threadIdx.x;
    if (t < 3) {
        double acc = cloud_sum(A.ws.part_reg + (int64_t)p * A.nchunk * 3, chunks_of(g.n[0]), t, 3, 0.0, false);
        acc = cloud_sum(A.ws.part_reg + (int64_t)(A.n_pairs + p) * A.nchunk * 3, chunks_of(g.n[1]), t, 3, acc, g.n[0] > 0);
        cs[t] = acc / (double)(g.n[0] + g.n[1]);
    }
    __syncthreads();
}

// grid (nchunk, 2B), ball only: chunk maxima of |reg - c|^2
__global__ __launch_bounds__(PREP_CHUNK) void prep_radius_kernel(PrepArgs A, const double* __restrict__ T_aug) {
    __shared__ double cs[3];
    __shared__ double red[4];
    const int B = A.n_pairs, cl = blockIdx.y, c = cl >= B ? 1 : 0, p = cl - c * B, chunk = blockIdx.x, t = threadIdx.x;
    const Geo g = pair_geo(A, p);
    const int i = chunk * PREP_CHUNK + t;
    if (chunk * PREP_CHUNK >= g.n[c]) return;
    ball_centre(A, g, p, cs);
    double d2 = 0.0;  // neutral: every |reg - c|^2 is >= 0
    if (i < g.n[c]) {
        double a[3], reg[3];
        reg_of(A, T_aug + (int64_t)p * 16, c, g.raw0[c] + i, a, reg);
        const double d0 = reg[0] - cs[0], d1 = reg[1] - cs[1], dz = reg[2] - cs[2];
        d2 = (d0 * d0 + d1 * d1) + dz * dz;
    }
    for (int msk = 1; msk < 64; msk <<= 1) d2 = fmax(d2, __shfl_xor(d2, msk));
    if ((t & 63) == 0) red[t >> 6] = d2;
    __syncthreads();
    if (t == 0) A.ws.part_max[(int64_t)cl * A.nchunk + chunk] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// c and s of pair p into cs[0..3] (all threads call; ends with a barrier)
__device__ __forceinline__ void pair_cs(const PrepArgs& A, const Geo& g, int p, double* cs) {
    const int t = threadIdx.x, B = A.n_pairs;
    const int nc[2] = {chunks_of(g.n[0]), chunks_of(g.n[1])};
    if (A.mode == 0) {
        ball_centre(A, g, p, cs);
        if (t == 0) {
            double mx = 0.0;
            for (int c = 0; c < 2; ++c)
                for (int j = 0; j < nc[c]; ++j) mx = fmax(mx, A.ws.part_max[(int64_t)(c * B + p) * A.nchunk + j]);
            cs[3] = 1.0 / sqrt(mx);
        }
    } else {
        if (t < 3) {
            double lo = INFINITY, hi = -INFINITY;
            for (int c = 0; c < 2; ++c)
                for (int j = 0; j < nc[c]; ++j) {
                    const int64_t slot = ((int64_t)(c * B + p) * A.nchunk + j) * 3 + t;
                    lo = fmin(lo, A.ws.part_lo[slot]);
                    hi = fmax(hi, A.ws.part_hi[slot]);
                }
            cs[t] = (lo + hi) / 2.0;
            cs[4 + t] = hi - lo;
        }
        __syncthreads();
        if (t == 0) cs[3] = 1.0 / (fmax(fmax(cs[4], cs[5]), cs[6]) / 2.0);
    }
    __syncthreads();
}

// grid (nchunk, 2B): the packed rows of a cloud, padding included; chunk sums of the normalised source for centre rule 0
__global__ __launch_bounds__(PREP_CHUNK) void prep_write_kernel(PrepArgs A, float* __restrict__ xyz) {
    __shared__ double sh[3][PREP_CHUNK];
    __shared__ double cs[8];
    const int B = A.n_pairs, cl = blockIdx.y, c = cl >= B ? 1 : 0, p = cl - c * B, chunk = blockIdx.x, t = threadIdx.x;
    const Geo g = pair_geo(A, p);
    const int i = chunk * PREP_CHUNK + t, cnt = min(PREP_CHUNK, g.n[c] - chunk * PREP_CHUNK);
    if (cnt <= 0) return;  // the padding of a cloud ends inside its last chunk: 128 divides 256
    pair_cs(A, g, p, cs);
    double v[3] = {0.0, 0.0, 0.0};
    if (i < pad_tile(g.n[c])) {
        float* o = xyz + (g.pk0[c] + i) * 3;
        if (i < g.n[c]) {
            const double* a = A.ws.aug + (g.raw0[c] + i) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[k] = (float)(cs[3] * (a[k] - cs[k]));
                v[k] = (double)o[k];
            }
        } else {
            o[0] = 0.0f, o[1] = 0.0f, o[2] = 0.0f;
        }
    }
    if (A.center_rule == 0 && c == 0) chunk_sum3(sh, v, cnt, A.ws.part_cen + ((int64_t)p * A.nchunk + chunk) * 3);
}

// grid B, block 64: the per-pair outputs
__global__ __launch_bounds__(64) void prep_finalize_kernel(PrepArgs A, const double* __restrict__ T_aug, float* __restrict__ center,
                                                           float* __restrict__ rot, float* __restrict__ trans, double* __restrict__ s_out,
                                                           double* __restrict__ c_out) {
    __shared__ double cs[8];
    __shared__ double tr[3];
    const int p = blockIdx.x, t = threadIdx.x, B = A.n_pairs;
    const Geo g = pair_geo(A, p);
    pair_cs(A, g, p, cs);
    const double* T4 = T_aug + (int64_t)p * 16;
    if (t < 3) {
        const double Rc = (T4[t * 4 + 0] * cs[0] + T4[t * 4 + 1] * cs[1]) + T4[t * 4 + 2] * cs[2];
        tr[t] = cs[3] * ((T4[t * 4 + 3] - cs[t]) + Rc);
        trans[p * 3 + t] = (float)tr[t];
        c_out[p * 3 + t] = cs[t];
        center[(B + p) * 3 + t] = 0.0f;
    }
    if (t < 9) rot[p * 9 + t] = (float)T4[(t / 3) * 4 + t % 3];
    if (t == 0) s_out[p] = cs[3];
    __syncthreads();
    if (t < 3) {
        double v;
        if (A.center_rule == 0)
            v = cloud_sum(A.ws.part_cen + (int64_t)p * A.nchunk * 3, chunks_of(g.n[0]), t, 3, 0.0, false) / (double)g.n[0];
        else if (A.center_rule == 1)
            v = tr[t];
        else
            v = -((T4[0 + t] * tr[0] + T4[4 + t] * tr[1]) + T4[8 + t] * tr[2]);
        center[p * 3 + t] = (float)v;
    }
}

// ---- the packed L1 loss

struct LossArgs {
    const float* pred;    // [rows_src,3]
    const float* xyz;     // packed; rows 0 .. rows_src are read
    const float* rot;     // [B,9]
    const float* trans;   // [B,3]
    const float* target;  // [rows_src,3] or null
    const int32_t* cloud_row0;
    const int32_t* cloud_len;
    int32_t n_pairs, max_len, nchunk;
    int64_t rows_src;
};

// rows of the source of pair p inside [0, rows_src), padding included; n = 0 otherwise
__device__ __forceinline__ int loss_geo(const LossArgs& A, int p, int64_t& row0) {
    row0 = A.cloud_row0[p];
    const int n = A.cloud_len[p];
    const bool ok = row0 >= 0 && n >= 0 && n <= A.max_len && row0 + pad_tile(n) <= A.rows_src;
    return ok ? n : 0;
}
// pred - g of a row, float64
__device__ __forceinline__ void loss_diff(const LossArgs& A, int p, int64_t row, double d[3]) {
    const float* q = A.pred + row * 3;
    if (A.target) {
        const float* g = A.target + row * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = (double)q[k] - (double)g[k];
    } else {
        const float* xr = A.xyz + row * 3;
        const float* R = A.rot + p * 9;
        const float* tt = A.trans + p * 3;
        const double x0 = (double)xr[0], x1 = (double)xr[1], x2 = (double)xr[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double g = (((double)R[k * 3 + 0] * x0 + (double)R[k * 3 + 1] * x1) + (double)R[k * 3 + 2] * x2) + (double)tt[k];
            d[k] = (double)q[k] - g;
        }
    }
}

// grid (nchunk, B): chunk sums of (|d0| + |d1|) + |d2|
__global__ __launch_bounds__(PREP_CHUNK) void l1_partial_kernel(LossArgs A, double* __restrict__ part) {
    __shared__ double sh[1][PREP_CHUNK];
    const int p = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    int64_t row0;
    const int n = loss_geo(A, p, row0);
    const int i = chunk * PREP_CHUNK + t, cnt = min(PREP_CHUNK, n - chunk * PREP_CHUNK);
    if (cnt <= 0) return;
    double r = 0.0;
    if (i < n) {
        double d[3];
        loss_diff(A, p, row0 + i, d);
        r = (fabs(d[0]) + fabs(d[1])) + fabs(d[2]);
    }
    chunk_sum1(sh, r, cnt, part + (int64_t)p * A.nchunk + chunk);
}

// one block: loss_pair[p] = cloud sum / N_p;  loss = fp32((loss_pair[0] + loss_pair[1] + ...) / B)
__global__ __launch_bounds__(PREP_CHUNK) void l1_final_kernel(LossArgs A, const double* __restrict__ part, double* __restrict__ loss_pair,
                                                              float* __restrict__ loss) {
    for (int p = threadIdx.x; p < A.n_pairs; p += PREP_CHUNK) {
        int64_t row0;
        const int n = loss_geo(A, p, row0);
        loss_pair[p] = cloud_sum(part + (int64_t)p * A.nchunk, chunks_of(n), 0, 1, 0.0, false) / (double)n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = loss_pair[0];
        for (int p = 1; p < A.n_pairs; ++p) acc += loss_pair[p];
        loss[0] = (float)(acc / (double)A.n_pairs);
    }
}

// grid (nchunk, B): dpred rows of a source, padding included
__global__ __launch_bounds__(PREP_CHUNK) void l1_bwd_kernel(LossArgs A, const float* __restrict__ dout, float* __restrict__ dpred) {
    const int p = blockIdx.y, i = blockIdx.x * PREP_CHUNK + threadIdx.x;
    int64_t row0;
    const int n = loss_geo(A, p, row0);
    if (i >= pad_tile(n)) return;
    float* o = dpred + (row0 + i) * 3;
    if (i >= n) {
        o[0] = 0.0f, o[1] = 0.0f, o[2] = 0.0f;
        return;
    }
    double d[3];
    loss_diff(A, p, row0 + i, d);
    const double go = (double)dout[0], den = (double)n * (double)A.n_pairs;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double sg = d[k] > 0.0 ? 1.0 : (d[k] < 0.0 ? -1.0 : 0.0);
        o[k] = (float)((go * sg) / den);
    }
}

inline bool loss_call_ok(const float* pred, const float* xyz, const float* rot, const float* trans, const float* target,
                         const int32_t* cloud_row0, const int32_t* cloud_len, int32_t n_pairs, int32_t max_len, int64_t rows_src) {
    return pred && cloud_row0 && cloud_len && (target || (xyz && rot && trans)) && n_pairs > 0 && max_len > 0 && rows_src > 0 &&
           rows_src <= INT32_MAX && max_len <= rows_src;
}

}  // namespace

extern "C" int64_t scream_prep_pairs_workspace_bytes(int64_t raw_rows, int32_t n_pairs, int32_t max_len) {
    if (raw_rows < 0 || raw_rows > INT32_MAX || n_pairs < 0 || max_len < 0 || max_len > raw_rows) return SCREAM_EINVAL;
    int64_t bytes;
    prep_carve(nullptr, raw_rows, n_pairs, max_len, &bytes);
    return bytes;
}

extern "C" int scream_prep_pairs(const void* raw, int32_t raw_is_f64, int64_t raw_rows, const int32_t* raw_row0, const int32_t* raw_len,
                                 int32_t max_len, const double* T, const double* perturb, const int32_t* side, double noise_std,
                                 uint64_t seed, const int64_t* sample_id, int32_t mode, int32_t center_rule, const int32_t* cloud_row0,
                                 int32_t n_pairs, int64_t rows_total, float* xyz, float* center, float* rot, float* trans, double* s,
                                 double* c, double* T_aug, void* workspace, int64_t workspace_bytes, void* stream) {
    SCREAM_REQUIRE(n_pairs >= 0 && raw_rows >= 0 && raw_rows <= INT32_MAX && rows_total >= 0 && rows_total <= INT32_MAX, SCREAM_EINVAL);
    SCREAM_REQUIRE(max_len >= 0 && max_len <= raw_rows, SCREAM_EINVAL);
    SCREAM_REQUIRE((mode == 0 || mode == 1) && center_rule >= 0 && center_rule <= 2 && noise_std >= 0.0 && isfinite(noise_std),
                   SCREAM_EINVAL);
    if (n_pairs == 0) return 0;
    SCREAM_REQUIRE(n_pairs <= 32767, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(max_len > 0 && raw && raw_row0 && raw_len && T && perturb && side && sample_id && cloud_row0 && xyz && center && rot &&
                       trans && s && c && T_aug && workspace,
                   SCREAM_EINVAL);
    PrepArgs A;
    int64_t need;
    A.ws = prep_carve(workspace, raw_rows, n_pairs, max_len, &need);
    SCREAM_REQUIRE(workspace_bytes >= need && aligned16(workspace), SCREAM_EINVAL);
    A.raw = raw, A.raw_is_f64 = raw_is_f64 != 0, A.raw_rows = raw_rows, A.raw_row0 = raw_row0, A.raw_len = raw_len, A.max_len = max_len;
    A.T = T, A.perturb = perturb, A.side = side, A.noise_std = noise_std, A.seed = seed, A.sample_id = sample_id;
    A.mode = mode, A.center_rule = center_rule, A.cloud_row0 = cloud_row0, A.n_pairs = n_pairs, A.rows_total = rows_total;
    A.nchunk = n_chunks(max_len);
    hipStream_t st = as_stream(stream);
    const dim3 blk(PREP_CHUNK), per_pair(A.nchunk, n_pairs), per_cloud(A.nchunk, 2 * n_pairs);
    prep_mean_kernel<<<per_pair, blk, 0, st>>>(A);
    SCREAM_LAUNCH_CHECK();
    prep_augment_kernel<<<per_cloud, blk, 0, st>>>(A, T_aug);
    SCREAM_LAUNCH_CHECK();
    if (mode == 0) {
        prep_radius_kernel<<<per_cloud, blk, 0, st>>>(A, T_aug);
        SCREAM_LAUNCH_CHECK();
    }
    prep_write_kernel<<<per_cloud, blk, 0, st>>>(A, xyz);
    SCREAM_LAUNCH_CHECK();
    prep_finalize_kernel<<<dim3(n_pairs), dim3(64), 0, st>>>(A, T_aug, center, rot, trans, s, c);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t scream_l1_pairs_workspace_bytes(int32_t n_pairs, int32_t max_len) {
    if (n_pairs < 0 || max_len < 0) return SCREAM_EINVAL;
    Carver w{nullptr};
    w.take<double>((int64_t)n_pairs * n_chunks(max_len));  // one piece: the chunk sums
    return w.used;
}

extern "C" int scream_l1_pairs_fwd(const float* pred, const float* xyz, const float* rot, const float* trans, const float* target,
                                   const int32_t* cloud_row0, const int32_t* cloud_len, int32_t n_pairs, int32_t max_len,
                                   int64_t rows_src, double* loss_pair, float* loss, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
    SCREAM_REQUIRE(loss_call_ok(pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len, rows_src), SCREAM_EINVAL);
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(loss_pair && loss && workspace && workspace_bytes >= scream_l1_pairs_workspace_bytes(n_pairs, max_len), SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned8(workspace), SCREAM_EINVAL);
    LossArgs A = {pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len, n_chunks(max_len), rows_src};
    double* part = reinterpret_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    l1_partial_kernel<<<dim3(A.nchunk, n_pairs), dim3(PREP_CHUNK), 0, st>>>(A, part);
    SCREAM_LAUNCH_CHECK();
    l1_final_kernel<<<dim3(1), dim3(PREP_CHUNK), 0, st>>>(A, part, loss_pair, loss);
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_l1_pairs_bwd(const float* dout, const float* pred, const float* xyz, const float* rot, const float* trans,
                                   const float* target, const int32_t* cloud_row0, const int32_t* cloud_len, int32_t n_pairs,
                                   int32_t max_len, int64_t rows_src, float* dpred, void* stream) {
    SCREAM_REQUIRE(loss_call_ok(pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len, rows_src), SCREAM_EINVAL);
    SCREAM_REQUIRE(n_pairs <= 65535, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(dout && dpred, SCREAM_EINVAL);
    LossArgs A = {pred, xyz, rot, trans, target, cloud_row0, cloud_len, n_pairs, max_len, n_chunks(max_len), rows_src};
    l1_bwd_kernel<<<dim3(A.nchunk, n_pairs), dim3(PREP_CHUNK), 0, as_stream(stream)>>>(A, dout, dpred);
    SCREAM_LAUNCH_CHECK();
    return 0;
}
