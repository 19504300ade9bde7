// Multi-tensor Adam (include/scream_hip.h, "The optimiser step"): every parameter of a model in one launch, the scalar state
// advanced by a one-thread launch behind it.  Built with -ffp-contract=off: every step of the contract is one IEEE float64
// operation, and the numpy restatement of tests/adam_ref.py does the same operations in the same order.
//
// The kernel is a stream: per element it reads p, grad, m, v and writes p, m, v (28 bytes), and does a few dozen float64
// instructions (one square root, two divisions).  One block of 256 lanes owns one chunk of SCREAM_ADAM_CHUNK elements of one
// tensor, four 16-byte accesses per lane and array when the four bases are 16-byte aligned (a chunk begins at a multiple of the
// chunk size, so it is as aligned as its tensor), element by element when one of them is not.  The grid is the chunk count.
#include "common.h"

namespace {

struct AdamTensor {  // one row of the work list: 40 bytes, the layout scream_amd/optim.py writes
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
};
static_assert(sizeof(AdamTensor) == SCREAM_ADAM_TENSOR_BYTES, "work-list row");

struct AdamScalars {  // what every element of a step shares
    double inv, one_b1, b2, one_b2, step_size, sqrt_bc2, eps;
};

__device__ __forceinline__ void adam_element(float& p, float g32, float& m, float& v, const AdamScalars& k) {
    const double g = (double)g32 * k.inv;
    const double md = (double)m, vd = (double)v;
    const double m1 = md + (g - md) * k.one_b1;
    const double v1 = (k.b2 * vd) + (k.one_b2 * (g * g));
    const double denom = sqrt(v1) / k.sqrt_bc2 + k.eps;
    p = (float)((double)p - k.step_size * (m1 / denom));
    m = (float)m1;
    v = (float)v1;
}

__global__ __launch_bounds__(256) void adam_kernel(const AdamTensor* __restrict__ tensors, int32_t n_tensors,
                                                   const int2* __restrict__ chunks, const double* __restrict__ state,
                                                   const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                   double lr, double b1, double b2, double eps) {
    if (found_inf && *found_inf != 0.0f) return;  // a skipped step: nothing is written
    const int2 c = chunks[blockIdx.x];
    if (c.x < 0 || c.x >= n_tensors || c.y < 0) return;
    const AdamTensor t = tensors[c.x];
    const int64_t begin = (int64_t)c.y * SCREAM_ADAM_CHUNK;
    if (begin >= t.n) return;
    const int64_t end = begin + SCREAM_ADAM_CHUNK < t.n ? begin + SCREAM_ADAM_CHUNK : t.n;
    AdamScalars k;
    k.inv = grad_scale ? 1.0 / (double)*grad_scale : 1.0;
    k.one_b1 = 1.0 - b1;
    k.b2 = b2;
    k.one_b2 = 1.0 - b2;
    const double q1 = state[0] * b1, q2 = state[1] * b2;  // this step's powers; scream_adam_advance stores them behind us
    k.step_size = lr / (1.0 - q1);
    k.sqrt_bc2 = sqrt(1.0 - q2);
    k.eps = eps;
    const int tid = threadIdx.x;
    const uintptr_t bases = reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                            reinterpret_cast<uintptr_t>(t.v);
    if ((bases & 15) == 0) {
        const int64_t vec_end = begin + ((end - begin) & ~(int64_t)3);
        for (int64_t i = begin + 4 * tid; i < vec_end; i += 4 * 256) {  // i + 4 <= vec_end: both are multiples of 4
            f32x4 p = *reinterpret_cast<const f32x4*>(t.p + i);
            const f32x4 g = *reinterpret_cast<const f32x4*>(t.g + i);
            f32x4 m = *reinterpret_cast<const f32x4*>(t.m + i);
            f32x4 v = *reinterpret_cast<const f32x4*>(t.v + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = p[j], mj = m[j], vj = v[j];
                adam_element(pj, g[j], mj, vj, k);
                p[j] = pj, m[j] = mj, v[j] = vj;
            }
            *reinterpret_cast<f32x4*>(t.p + i) = p;
            *reinterpret_cast<f32x4*>(t.m + i) = m;
            *reinterpret_cast<f32x4*>(t.v + i) = v;
        }
        const int64_t i = vec_end + tid;  // the tail of numel % 4 elements (only a tensor's last chunk has one)
        if (i < end) adam_element(t.p[i], t.g[i], t.m[i], t.v[i], k);
    } else {
        for (int64_t i = begin + tid; i < end; i += 256) adam_element(t.p[i], t.g[i], t.m[i], t.v[i], k);
    }
}

// One thread, behind the element launch on the same stream: no block of that launch can still read the state it writes.
__global__ void adam_advance_kernel(double* state, const float* __restrict__ found_inf, double b1, double b2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf && *found_inf != 0.0f) return;
    state[0] = state[0] * b1;
    state[1] = state[1] * b2;
    float* step = reinterpret_cast<float*>(state + 2);
    *step = *step + 1.0f;
}

}  // namespace

extern "C" int scream_adam_step(const void* tensors, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, double* state,
                                const float* grad_scale, const float* found_inf, double lr, double beta1, double beta2, double eps,
                                void* stream) {
    SCREAM_REQUIRE(n_tensors >= 0 && n_chunks >= 0 && n_chunks <= INT32_MAX, SCREAM_EINVAL);
    SCREAM_REQUIRE(state && aligned8(state), SCREAM_EINVAL);
    SCREAM_REQUIRE(n_chunks == 0 || (tensors && chunks && n_tensors > 0), SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned8(tensors) && aligned8(chunks), SCREAM_EINVAL);
    SCREAM_REQUIRE(lr >= 0.0 && lr < INFINITY && beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && eps < INFINITY,
                   SCREAM_EINVAL);
    hipStream_t st = as_stream(stream);
    if (n_chunks > 0) {
        adam_kernel<<<dim3((unsigned)n_chunks), dim3(256), 0, st>>>(static_cast<const AdamTensor*>(tensors), n_tensors,
                                                                    reinterpret_cast<const int2*>(chunks), state, grad_scale, found_inf,
                                                                    lr, beta1, beta2, eps);
        SCREAM_LAUNCH_CHECK();
    }
    adam_advance_kernel<<<dim3(1), dim3(64), 0, st>>>(state, found_inf, beta1, beta2);
    SCREAM_LAUNCH_CHECK();
    return 0;
}
