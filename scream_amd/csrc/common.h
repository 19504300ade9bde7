// Shared helpers for the gfx950 kernels of libscream_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/scream_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define SCREAM_LAUNCH_CHECK()                         \
    do {                                              \
        hipError_t e_ = hipGetLastError();            \
        if (e_ != hipSuccess) return (int)e_;         \
    } while (0)

#define SCREAM_REQUIRE(cond, code) \
    do {                           \
        if (!(cond)) return (code); \
    } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// what the entry points ask of a caller's pointer: 16 bytes for the dwordx4 accesses, 8 for arrays of doubles and of pointers,
// 256 for the raw-scan ICP's workspace
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool aligned256(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 255) == 0; }

// ---- host helpers of the ops on packed clouds (the rows of many clouds back to back, row0 / len per cloud)
static inline int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
// blocks of 256 threads that cover the longest cloud of a call
static inline unsigned row_blocks(int32_t max_len) { return (unsigned)(((int64_t)max_len + 255) / 256); }
// what a caller may declare about one packed array: int32 row indices, no cloud longer than the array
static inline bool rows_ok(int64_t rows, int32_t max_len) { return rows >= 0 && rows <= INT32_MAX && max_len >= 0 && max_len <= rows; }
// A workspace handed out front to back, every piece at a multiple of 256 bytes.  Carved from a null base it only measures:
// `used` afterwards is the size that the same sequence of take() calls needs.
struct Carver {
    void* base;
    int64_t used = 0;
    template <class T> T* take(int64_t count) {
        T* r = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + (uintptr_t)used);
        used += align256(count * (int64_t)sizeof(T));
        return r;
    }
};

// ---- device helpers of the matrix kernels (gemm_f32.hip, gemm_split.hip / gemm_epilogue.h, ring.h, backward.hip)
typedef const __attribute__((address_space(1))) void* gptr_t;  // source and destination of an LDS-DMA piece
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// s_waitcnt vmcnt(N) lgkmcnt(0) + workgroup barrier: the N youngest vector-memory operations of this wave (gemm_split.hip: the A
// loads of the k-tile after next; the ring kernels: the DMA pieces of the stage after the one about to be read) stay in flight
template <int N>
__device__ __forceinline__ void ring_barrier() {
    __builtin_amdgcn_s_waitcnt(0x0070 | (N & 15) | ((N >> 4) << 14));
    __builtin_amdgcn_s_barrier();
}

// workgroup barrier that waits for this wave's LDS traffic only: a __syncthreads() would also drain the LDS-DMA prefetch that is
// deliberately left in flight (the vector-memory queue stays untouched)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
    __builtin_amdgcn_s_barrier();
}

// Row index inside a 32x32 MFMA accumulator tile held by lane (lane>>5 = half) in register reg.
// (cdna_hip_programming.md section 3: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * half.)
__device__ __forceinline__ int mfma32_row(int reg, int half) { return (reg & 3) + 8 * (reg >> 2) + 4 * half; }

__device__ __forceinline__ float half_wave_sum(float v) {
    // Sum over the 32 lanes that share lane>>5 (xor masks < 32 never cross the half).
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    return v;
}

// Sum over the 64 lanes of a wave, result in every lane.  DPP inclusive scan (row_shr 1/2/4/8 inside each 16-lane
// row, then row_bcast15 into rows 1/3 and row_bcast31 into rows 2/3) leaves the total in lane 63; six VALU
// instructions and one v_readlane instead of six dependent ds_bpermute round trips through the LDS pipeline.
__device__ __forceinline__ float wave_sum(float v) {
#define SCREAM_DPP_ADD(ctrl, row_mask)                                                                      \
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, row_mask, \
                                                               0xf, true))
    SCREAM_DPP_ADD(0x111, 0xf);  // row_shr:1 (out-of-row lanes read 0: bound_ctrl)
    SCREAM_DPP_ADD(0x112, 0xf);  // row_shr:2
    SCREAM_DPP_ADD(0x114, 0xf);  // row_shr:4
    SCREAM_DPP_ADD(0x118, 0xf);  // row_shr:8  -> lane 15 of each row holds the row sum
    SCREAM_DPP_ADD(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
    SCREAM_DPP_ADD(0x143, 0xc);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave sum
#undef SCREAM_DPP_ADD
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// elu(x) + 1 (models/transformer.py:7-8: the feature map of the linear attention) = x + 1 for x > 0, exp(x) otherwise.  The
// exponential runs on the hardware's exp2 (v_exp_f32, 1 ulp) with the rounding of x * log2(e) -- product and constant -- carried
// into a first-order correction, exp2(hi) (1 + lo ln 2): within 2 ulp of exp(x), where expf() spends 14 vector instructions on
// range handling that an argument <= 0 never needs (2 x 10^9 of these per 32-pair step, in epilogues no MFMA hides).
// Round 4: no compare / select.  exp2's result is CLAMPED to [0, 1] (an output modifier of the instruction: free), so the
// exponential branch is exact for x <= 0 and ~1 for x > 0, and since e^x >= 1 + x everywhere, elu(x) + 1 = max(1 + x, that):
// eight instructions instead of ten (at the socket power cap every vector instruction of an epilogue is paid in time).
// elu1s(t, c): elu(t c) + 1 for an accumulator t in units of 1 / c, c an exact power of two: the constants carry c (a power of
// two commutes with every rounding), so the scaling multiply in front of the epilogue disappears -- bit for bit elu1(t * c).
// Valid for |x| < 2^126 (beyond that x log2(e) overflows and 0 * inf appears).
struct Elu1Consts {
    float c, cl2e, cl2e_lo;  // c, c * log2(e) rounded to fp32, c * (log2(e) - that)
};
static inline Elu1Consts elu1_consts(float c) { return Elu1Consts{c, c * 1.44269502162933349609375f, c * 1.925963033500011e-08f}; }
__device__ __forceinline__ float elu1s(float t, const Elu1Consts& k) {
    const float LN2 = 0.693147182464599609375f;
    const float hi = t * k.cl2e;
    const float lo = __builtin_fmaf(t, k.cl2e_lo, __builtin_fmaf(t, k.cl2e, -hi));
    const float r = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(hi), 0.0f, 1.0f);  // folds into v_exp_f32 ... clamp
    const float e = __builtin_fmaf(r, lo * LN2, r);
    return fmaxf(__builtin_fmaf(t, k.c, 1.0f), e);
}
// elu1s of TWO independent elements in place (element i of a and of b), cut into four steps of four instructions that a caller
// spreads over four gaps between matrix instructions (proj_ring.hip): the same eight instructions per element on the same
// operands -- bit for bit elu1s -- but no instruction reads the result of the one in front of it, each step holds at most one
// v_exp_f32, and a step's results are consumed a gap later.  The state between the steps is four registers; the element itself
// turns into 1 + t c in step 2 / 3, once nothing reads t any more.
struct Elu1Pair {
    float r[2], l[2];  // hi, then exp2(hi) clamped | the rounding term, then lo, then lo ln 2, then the exponential branch
};
// An empty statement that hipcc neither moves nor looks through: what it is given has been computed where it stands.  (Left
// alone hipcc SINKS a computation whose only reader stands in a conditional block into that block -- all of a query chunk's
// elu + 1 landed behind one matrix instruction, in front of the chunk's stores.)
__device__ __forceinline__ void keep_here(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void keep_here(float& x, float& y) { asm volatile("" : "+v"(x), "+v"(y)); }
__device__ __forceinline__ void keep_here(float& x, float& y, float& z) { asm volatile("" : "+v"(x), "+v"(y), "+v"(z)); }
__device__ __forceinline__ void keep_here(float& x, float& y, float& z, float& w) { asm volatile("" : "+v"(x), "+v"(y), "+v"(z), "+v"(w)); }
__device__ __forceinline__ void elu1s_pair(int step, f32x16& a, f32x16& b, int i, Elu1Pair& s, const Elu1Consts& k) {
    const float LN2 = 0.693147182464599609375f;
    if (step == 0) {
        s.r[0] = a[i] * k.cl2e;
        s.r[1] = b[i] * k.cl2e;
        s.l[0] = __builtin_fmaf(a[i], k.cl2e, -s.r[0]);
        s.l[1] = __builtin_fmaf(b[i], k.cl2e, -s.r[1]);
        keep_here(s.l[0], s.l[1]);
    } else if (step == 1) {
        s.r[0] = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(s.r[0]), 0.0f, 1.0f);  // folds into v_exp_f32 ... clamp
        s.l[0] = __builtin_fmaf(a[i], k.cl2e_lo, s.l[0]);
        s.l[1] = __builtin_fmaf(b[i], k.cl2e_lo, s.l[1]);
        s.l[0] = s.l[0] * LN2;
        keep_here(s.r[0], s.l[0], s.l[1]);
    } else if (step == 2) {
        s.r[1] = __builtin_amdgcn_fmed3f(__builtin_amdgcn_exp2f(s.r[1]), 0.0f, 1.0f);
        s.l[1] = s.l[1] * LN2;
        s.l[0] = __builtin_fmaf(s.r[0], s.l[0], s.r[0]);
        float p = __builtin_fmaf(a[i], k.c, 1.0f);
        keep_here(s.r[1], s.l[1], s.l[0], p);
        a[i] = p;
    } else {
        s.l[1] = __builtin_fmaf(s.r[1], s.l[1], s.r[1]);
        // (v_max_f32 spelled out: behind keep_here hipcc no longer knows its operands to be canonical and would put a v_max x, x in
        // front of each)
        float pa, pb = __builtin_fmaf(b[i], k.c, 1.0f);
        asm volatile("v_max_f32 %0, %1, %2" : "=v"(pa) : "v"(a[i]), "v"(s.l[0]));
        asm volatile("v_max_f32 %0, %1, %2" : "=v"(pb) : "v"(pb), "v"(s.l[1]));
        a[i] = pa;
        b[i] = pb;
    }
}
__device__ __forceinline__ float elu1(float x) {
    return elu1s(x, Elu1Consts{1.0f, 1.44269502162933349609375f, 1.925963033500011e-08f});
}

// blocks of the persistent grids: one per CU (fewer measured slower: 240 / 224 blocks 1 872 / 1 882 pairs/s against 1 898,
// profiles/r04_persistent_grid_sweep.txt)
constexpr int SCREAM_MAX_GRID = 256;
