// The q / k / v projections of an MHAttention block (models/transformer.py:79-81 with the elu(.) + 1 of :28-29 on q and k) and the
// fused K^T V reduction (:38-41) as a RING kernel on the fp16 matrix cores of gfx950 (round 4) -- the geometry of the layer tail
// (tail_split.hip: one wave per SIMD, the weights streamed through a ring of LDS stages by LDS-DMA, one barrier per stage) with
// SIXTY-FOUR rows per wave:
//
//   * a wave owns two 32-row groups of x and keeps BOTH groups' operand planes (split.h: x 2^e = x0 + x1 in fp16) in registers
//     for the whole 256-row tile: x is read and split ONCE per tile, where gemm_split_kernel re-reads and re-splits its A rows for
//     every 256-column tile (three times for q | k | v; PMC: 1.9 x the input fetched);
//   * every weight fragment read from LDS feeds SIX matrix instructions (three per row group) instead of three: half the LDS
//     fragment reads per product of both older kernels, and a stage -- one 32-column chunk of W over the whole K = 256, 32 KiB
//     -- carries 96 MFMAs per wave between two barriers instead of 48;
//   * the epilogue of a chunk RIDES inside the MFMA groups of the next stage (the accumulators are double buffered):
//       - a query chunk is computed transposed (A = weights, B = x rows): lane = row, registers = features, which IS the
//         fragment-major layout of Q' (include/scream_hip.h) -- elu + 1 and four 1 KiB stores per row group, no LDS;
//       - a key or value chunk is computed the other way round (A = x rows, B = weights): lane = feature, registers = rows --
//         the operand layout of a product whose contraction index is the ROW.  K' = elu(k) + 1 (padding rows zeroed) and V are
//         split into fp16 planes straight from the accumulators and K'^T V of the wave's 64 rows is 12 MFMAs; the two waves
//         of a 128-row tile add their tiles through 8 KiB of LDS in a fixed order and write the per-tile partial
//         [head][33][32] that scream_kv_finalize_image sums per cloud.  K' and V never exist in memory.
//     In the 8-wave GEMM a query tile's epilogue (a third of its time) ran with the matrix pipe idle -- its block-wide k-loop
//     barriers keep both waves of a SIMD in lockstep.
//     WHERE a ride's instructions stand is decided here, not by hipcc: a ride is cut into pieces of about four vector
//     instructions, at most one v_exp_f32 among them, one piece behind each of a stage's 96 matrix instructions, with a
//     sched_barrier(0) on both sides of every matrix instruction; its dependent chains run two elements in lock-step and a
//     result is read a gap after it was made (common.h: elu1s_pair, split.h: split1s_pair_here).  Behind a 32-cycle matrix
//     instruction about five vector instructions issue for free; a longer run makes the matrix pipe wait, and with one wave
//     per SIMD so does a chain that waits for its own results.  (Scheduled by hipcc -- sched_group_barrier slots, "up to six
//     behind each" -- the rides filled the first gaps of a group and left 886 of 1 187 empty, and a query chunk's whole
//     elu + 1, 260 instructions, was SUNK into the conditional block of its stores, behind ONE matrix instruction.  Placing them by
//     hand took 12 % off the kernel's cycles, 5-6 % off its time: profiles/r05_proj_rides_ab.txt; tests/test_proj_ring_rides_host.py holds the generated code to it.)
//     (Built first with LDS-DMA "touches" -- one dword per 128-byte line of the NEXT tile's rows, one instruction per stage -- to have
//     the rows in the L2 before the tile boundary reads them: 3-5 % SLOWER and 3.7 x the HBM fetch traffic by the counters, the
//     narrow loads are fetched line by line and do not stay; removed -- profiles/r04_ring_proj_prefetch_experiment.txt.)
//   * work is cut into UNITS of two stages (two query chunks, or the K and V chunk of one head) and every block takes a
//     CONTIGUOUS range of the launch's units, tile-major: no partial last round (1 302 row tiles on 256 CUs were 5.09 -> 6 rounds
//     of the old persistent grid), at the price of one extra x tile load per block.  A row's results do not depend on how its
//     tile was cut: chunks and heads are independent outputs.
//
// Stage sequence per 256-row tile (= image order): Q chunk 0 .. 7 (absent for a key/value-only call), then per layer of the
// call and head h: K_h, V_h.  Vector-memory discipline: the ring's barrier waits with a COUNTED vmcnt that leaves the pieces
// issued during the previous stage in flight; every store of a stage is issued before that stage's pieces (a counted wait is
// only sound if what it leaves in flight are loads: stores retire out of order against loads) -- a ride's stores stand in
// groups 0 .. Q_WIN = 12 of a stage's 16, its pieces in groups 13 .. 15, still more than a stage ahead of their use; the only register loads are the
// x rows at a tile boundary, plain loads that hipcc waits for with vmcnt(0).
#include <type_traits>

#include "matrix_front.h"
#include "ring.h"

namespace {

constexpr int P_PF = 2;  // register sets of weight fragments: fragments are read P_PF - 1 MFMA groups ahead (a third set does not fit: 512 registers)
constexpr int P_LB = 2;  // x segments per load batch at a tile boundary (two batches in flight)

constexpr int P_KV_ELEMS = (SCREAM_HEAD_DIM + 1) * SCREAM_HEAD_DIM;  // 1056
constexpr int P_SLAB_BYTES = 4 * P_KV_ELEMS * 4;                      // one K^T V tile + Ksum per wave

struct ProjArgs {
    const float* x;        // fragment-major [M, 256]
    const char* Wimg;      // [S][NP][16][64][16 B]
    float* Q;              // fragment-major [M, 256] (n_q == 8) or NULL
    int64_t M;
    int32_t n_q;           // query stages per tile: 0 or 8
    int32_t S;             // stages per tile: n_q + 16 L
    float* kv_partial;     // [L][M / 128][8][1056]
    int64_t kv_layer_stride;
    const int32_t* tile_cloud;
    const int32_t* cloud_row0;
    const int32_t* cloud_len;
    int64_t row_base;
    float a_scale, kv_sk, kv_cv, kv_inv;  // 2^a_exp; 2^k_exp; 2^(v_exp - a_exp - w_exp); 2^-(k_exp + v_exp)
    Elu1Consts ec;                         // of c = 2^-(a_exp + w_exp): accumulator -> q, k (common.h: elu1s)
};

template <class SP>
__global__ __launch_bounds__(TT, 1) void proj_ring_kernel(ProjArgs pa) {
    typedef typename SP::vec V;
    constexpr int NP = SP::NP;
    constexpr int STAGE = stage_bytes<SP>();
    constexpr int PIECES = wave_pieces<SP>();   // LDS-DMA weight pieces per wave and stage
    constexpr int INFLIGHT = PIECES;            // what a ring wait leaves in flight: the pieces issued during the previous stage
    constexpr int GM = 2 * SP::NPROD;           // matrix instructions of a group = gaps that a ride can fill
    constexpr int Q_WIN = 12;                   // a query chunk's elu + 1 rides in groups 0 .. Q_WIN - 1, its stores go out in group Q_WIN
    constexpr int PIECE_STRIDE = (15 - Q_WIN) * GM / PIECES;  // one weight piece per so many gaps of groups Q_WIN + 1 .. 15
    static_assert(PIECE_STRIDE >= 1, "the groups behind the stores hold the stage's pieces");
    __shared__ __attribute__((aligned(16))) char smem[T_SLOTS * STAGE + P_SLAB_BYTES];  // the ONLY LDS object
    float* slabs = reinterpret_cast<float*>(smem + T_SLOTS * STAGE);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, r = lane & 31;
    const unsigned v_lane16 = lane * 16;

    // ---- this block's units -----------------------------------------------------------------------------------------------
    const int S = pa.S, UPT = S >> 1, nq2 = pa.n_q >> 1;
    const int64_t n_tiles = (pa.M + 255) >> 8;
    const int64_t U = n_tiles * UPT;
    const int64_t u_lo = U * blockIdx.x / gridDim.x, u_hi = U * (blockIdx.x + 1) / gridDim.x;
    if (u_lo >= u_hi) return;
    const int s0 = (int)(u_lo % UPT) * 2;  // image stage of the block's first ring stage

    unsigned q = 0;  // ring stages consumed so far
    auto dma_piece = [&](unsigned qq, int u) __attribute__((always_inline)) {
        const unsigned img = (unsigned)(s0 + qq) % (unsigned)S, slot = qq % (unsigned)T_SLOTS;
        const char* sbase = pa.Wimg + (size_t)img * STAGE + (wave * PIECES + (u & ~3)) * 1024;
        dma_1k(sbase + v_lane16, smem + slot * STAGE + (wave * PIECES + (u & ~3)) * 1024, u & 3);
    };
#pragma unroll
    for (int u = 0; u < PIECES; ++u) dma_piece(0, u);
#pragma unroll
    for (int u = 0; u < PIECES; ++u) dma_piece(1, u);

    // ---- per-tile state ---------------------------------------------------------------------------------------------------
    V xp[2][16][NP];     // operand planes of the wave's two row groups: xp[rg][2 blk + s2] = 16-deep step s2 of feature segment blk
    int64_t tile = -1;
    bool wave_ok = false;      // the wave's rows exist (the last tile of an odd number of 128-row tiles has two idle waves)
    int valid0 = 0;            // real tokens among the wave's 64 rows and behind (padding rows do not exist for K^T V)
    float* part_tile = nullptr;  // kv_partial of the wave's 128-row tile, layer 0, head 0
    float* qg = nullptr;         // Q + first float of the wave's 64 rows + this lane's 4 floats

    auto enter_tile = [&](int64_t t) __attribute__((always_inline)) {
        tile = t;
        const int64_t t128 = t * 2 + (wave >> 1);
        wave_ok = t128 * 128 < pa.M;
        const int64_t row0 = wave_ok ? t * 256 + wave * 64 : t * 256;  // (idle waves recompute the tile's first rows; nothing of it is stored)
        const float* g = pa.x + row0 * SCREAM_D_MODEL + lane * 4;
        valid0 = 0;
        if (wave_ok && pa.S > pa.n_q) {
            const int64_t arow = pa.row_base + t128 * 128;
            const int cloud = pa.tile_cloud[arow / SCREAM_ROW_TILE];
            valid0 = pa.cloud_len[cloud] - (int)(arow - pa.cloud_row0[cloud]) - (wave & 1) * 64;
        }
        part_tile = pa.kv_partial + t128 * SCREAM_NHEAD * P_KV_ELEMS;
        qg = pa.Q + row0 * SCREAM_D_MODEL + lane * 4;
        // the wave's 64 rows, P_LB segments of one row group (4 P_LB loads, 16 P_LB registers) at a time, two batches in flight:
        // the next batch is requested before the previous one is split (the whole tile at once would not fit beside the
        // pending accumulators and the K' planes)
        constexpr int LB = P_LB, NB = 16 / LB;  // batch b: row group b / (NB / 2), segments LB (b % (NB / 2)) .. + LB - 1
        f32x4 raw[2][LB][4];
        auto request = [&](int b) __attribute__((always_inline)) {
            const int rg = b / (NB / 2), blk0 = LB * (b % (NB / 2));
#pragma unroll
            for (int k = 0; k < LB; ++k)
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    raw[b & 1][k][a] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + rg * 8192 + ((blk0 + k) * 4 + a) * 256));
        };
        request(0);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int rg = b / (NB / 2), blk0 = LB * (b % (NB / 2));
            __builtin_amdgcn_sched_barrier(0);
            if (b + 1 < NB) request(b + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < LB; ++k)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                {
                    V tmp[NP];
#pragma unroll
                    for (int j = 0; j < 8; ++j) SP::split1s(raw[b & 1][k][2 * s2 + (j >> 2)][j & 3], pa.a_scale, j, tmp);
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        // the planes LIVE in accumulation registers (the MFMA reads its A / B operand from either file): 256 of them,
                        // the whole AGPR file -- left to itself hipcc keeps them VGPR-class and moves each one back before every use
                        asm volatile("" : "+a"(tmp[p]));
                        xp[rg][2 * (blk0 + k) + s2][p] = tmp[p];
                    }
                }
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- pipeline state: the accumulators of a stage are consumed by the ride of the next one -----------------------------------
    f32x16 acc[2][2];       // [stage parity][row group]
    f16x8 kp[2][2][2];      // K' planes [row group][16-row step][plane]: A operand of K'^T V (the reduction runs on fp16 x 2 for every SP)
    f32x16 kv;              // K'^T V of the wave's 64 rows: lane = v, registers = d
    float ks = 0.f;         // Ksum[d = r] over the wave's rows
    float* q_pend = nullptr;     // where the pending query chunk goes (its tile's qg + chunk offset)
    bool q_pend_ok = false;
    float* part_pend = nullptr;  // where the pending head's partial goes
    bool part_pend_ok = false;

    // One ring stage: 16 groups = one 32-column chunk of W over K = 256 against the wave's 64 rows; a group is the 16-deep step g of
    // both row groups against the same weight fragment, GM matrix instructions (row group 0's products, then row group 1's).
    // KIND 0: acc^T += W . x^T (lane = row, registers = features); KIND 1: acc += x . W^T (lane = feature, registers = rows).
    // Every matrix instruction is placed BY HAND: sched_barrier(0) on both sides of it, so what stands between two of them in the
    // source is what stands between them in the code.  ride(g, m) is the piece of the previous chunk's epilogue that goes behind
    // matrix instruction m of group g: every ride cuts itself into GM pieces per group of a few vector instructions each, at most
    // one of them a transcendental -- behind a 32-cycle matrix instruction about five vector instructions issue for free, one
    // wave per SIMD has nothing else to issue while a dependent chain waits, and a gap left empty hides nothing.  The fragment
    // reads of the next group go behind the group's first matrix instruction, the ride's stores in groups <= Q_WIN, this stage's
    // weight pieces one per PIECE_STRIDE gaps from group Q_WIN + 1 on.
    auto stage = [&](auto kind, f32x16 (&a)[2], auto ride) __attribute__((always_inline)) {
        constexpr int KIND = decltype(kind)::value;
        ring_barrier<INFLIGHT>();
        __builtin_amdgcn_sched_barrier(0);
        const char* wb = smem + (q % T_SLOTS) * STAGE + lane * 16;
        V wf[P_PF][NP];
        f32x16 z;
#pragma unroll
        for (int e = 0; e < 16; ++e) z[e] = 0.f;
#pragma unroll
        for (int g0 = 0; g0 < P_PF - 1; ++g0)
#pragma unroll
            for (int p = 0; p < NP; ++p) wf[g0][p] = ld_frag<V>(wb + (p * 16 + g0) * 1024);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
#pragma unroll
            for (int m = 0; m < GM; ++m) {
                const int rg = m / SP::NPROD, i = m % SP::NPROD;
                __builtin_amdgcn_sched_barrier(0);
                if (KIND == 0) a[rg] = SP::product(i, wf[g % P_PF], xp[rg][g], g == 0 && i == 0 ? z : a[rg]);
                else a[rg] = SP::product(i, xp[rg][g], wf[g % P_PF], g == 0 && i == 0 ? z : a[rg]);
                __builtin_amdgcn_sched_barrier(0);
                if (m == 0 && g + P_PF - 1 < 16) {
#pragma unroll
                    for (int p = 0; p < NP; ++p) wf[(g + P_PF - 1) % P_PF][p] = ld_frag<V>(wb + (p * 16 + g + P_PF - 1) * 1024);
                }
                const int ps = (g - Q_WIN - 1) * GM + m;  // the PIECES weight pieces of the stage after next, behind every store of this stage's ride
                if (ps >= 0 && ps % PIECE_STRIDE == 0 && ps / PIECE_STRIDE < PIECES) dma_piece(q + 2, ps / PIECE_STRIDE);
                ride(g, m);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        ++q;
    };
    static_assert(wave_pieces<SP>() <= 8, "the request schedule of a stage holds eight pieces");
    constexpr std::integral_constant<int, 0> kindQ{};
    constexpr std::integral_constant<int, 1> kindKV{};

    // ---- rides --------------------------------------------------------------------------------------------------------------
    // items k0 .. k1 - 1 of n_items go into slot s of n_slots: in order, as evenly as the two numbers allow
    auto first_item = [](int s, int n_items, int n_slots) __attribute__((always_inline)) { return (s * n_items + n_slots - 1) / n_slots; };
    auto per_slot = [](int n_items, int n_slots) constexpr { return (n_items + n_slots - 1) / n_slots; };  // the most a slot holds
    Elu1Pair ep;  // the elu + 1 chains under way: element i of both row groups in lock-step (common.h: elu1s_pair)
    // Q' chunk = elu(q) + 1 in place, fragment-major: piece a of an accumulator tile is one 1 KiB wave store (tail_split.hip: store_chunk)
    // 16 pairs of four steps over the Q_WIN * GM gaps of groups 0 .. Q_WIN - 1
    auto ride_q = [&](f32x16 (&t)[2], int g, int m) __attribute__((always_inline)) {
        if (g < Q_WIN) {
            const int s = g * GM + m;
#pragma unroll
            for (int j = 0; j < per_slot(64, Q_WIN * GM); ++j) {
                const int k = first_item(s, 64, Q_WIN * GM) + j;
                if (k < first_item(s + 1, 64, Q_WIN * GM)) elu1s_pair(k & 3, t[0], t[1], k >> 2, ep, pa.ec);
            }
        }
        if (g == Q_WIN && m == 0) {
            if (q_pend_ok) {
#pragma unroll
                for (int rg = 0; rg < 2; ++rg)
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const f32x4 o = {t[rg][4 * a], t[rg][4 * a + 1], t[rg][4 * a + 2], t[rg][4 * a + 3]};
                        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(q_pend + rg * 8192 + a * 256));
                    }
            }
        }
    };
    // K' = elu(k) + 1 with the padding rows zeroed, its row sum and its two fp16 planes: register g of both row groups in group g,
    // six items (the four steps of the pair's elu + 1, mask and row sum, the split) over the group's GM gaps.
    // MASK (compile time; wave-uniform per tile): only a cloud's last tile has padding rows -- everywhere else the compare and
    // select per element are left out
    auto ride_k = [&](auto mask, f32x16 (&t)[2], int valid, int g, int m) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < per_slot(6, GM); ++j) {
            const int k = first_item(m, 6, GM) + j;
            if (k >= first_item(m + 1, 6, GM)) continue;
            if (k < 4) elu1s_pair(k, t[0], t[1], g, ep, pa.ec);
            if (k == 4) {
                if (g == 0) ks = 0.f;
#pragma unroll
                for (int rg = 0; rg < 2; ++rg) {
                    if (decltype(mask)::value && (g & 3) + 8 * (g >> 2) + 32 * rg >= valid) t[rg][g] = 0.f;  // row mfma32_row(g, half) + 32 rg of the wave's 64 (valid carries the half)
                    ks += t[rg][g];
                }
                keep_here(ks);
            }
            if (k == 5) {
                SplitH2::split1s_pair_here(t[0][g], t[1][g], pa.kv_sk, g & 7, kp[0][g >> 3], kp[1][g >> 3]);
                if (g == 15) ks += __shfl_xor(ks, 32);
            }
        }
    };
    // V's planes, the 12 MFMAs of K'^T V over the wave's 64 rows, the wave's tile into its LDS slab
    f16x8 vp[2][2];  // [row group][plane] of the 16-row step being made
    auto ride_v = [&](const f32x16 (&t)[2], int g, int m) __attribute__((always_inline)) {
        if (g < 8) {
            const int s2 = g >> 2;  // groups 0-3: rows' step 0, groups 4-7: step 1
            // the group's two elements of both row groups behind its first two matrix instructions; a step's products behind the last
            // matrix instruction of its fourth group
            if (m < 2) {
                const int i = 8 * s2 + 2 * (g & 3) + m;
                SplitH2::split1s_pair_here(t[0][i], t[1][i], pa.kv_cv, i & 7, vp[0], vp[1]);
            }
            if ((g & 3) == 3 && m == GM - 1) {
                f32x16 z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0.f;
                SplitH2::products(kv, kp[0][s2], vp[0], s2 == 0 ? z : kv);
                SplitH2::products(kv, kp[1][s2], vp[1], kv);
            }
        }
        if (g == 9) {  // exact: a power of two (1 / v_length is applied once, in scream_kv_finalize_image)
#pragma unroll
            for (int j = 0; j < per_slot(16, GM); ++j) {
                const int e = first_item(m, 16, GM) + j;
                if (e < first_item(m + 1, 16, GM)) kv[e] *= pa.kv_inv;
            }
        }
        if (g >= 10 && g < 14) {
            float* sw = slabs + wave * P_KV_ELEMS;
            const int s = (g - 10) * GM + m;
#pragma unroll
            for (int j = 0; j < per_slot(16, 4 * GM); ++j) {
                const int e = first_item(s, 16, 4 * GM) + j;
                if (e < first_item(s + 1, 16, 4 * GM)) sw[mfma32_row(e, half) * 32 + r] = kv[e];  // [d][v]
            }
            if (g == 13 && m == GM - 1 && half == 0) sw[32 * 32 + r] = ks;
        }
    };
    // the two waves of a 128-row tile add their K'^T V tiles (even wave's first) and write the partial: 1 056 floats, half each;
    // the two LDS reads behind one matrix instruction, the sum and its store behind a later one
    float kvs[2];
    auto ride_kvstore = [&](int g, int m) __attribute__((always_inline)) {
        constexpr int M_RD = GM >= 4 ? 1 : 0, M_ST = GM >= 4 ? 3 : GM - 1;
        if (g > 8 || (m != M_RD && m != M_ST)) return;
        const int i = (wave & 1) * 64 + lane + 128 * g;
        if (i < P_KV_ELEMS && part_pend_ok) {
            const float* s2 = slabs + (wave & ~1) * P_KV_ELEMS + i;
            if (m == M_RD) {
                kvs[0] = s2[0];
                kvs[1] = s2[P_KV_ELEMS];
            }
            if (m == M_ST) part_pend[i] = kvs[0] + kvs[1];  // a plain store: non-temporal, kv_finalize_image reads the partials from memory (profiles/r04_nontemporal_and_stash.txt)
        }
    };

    // ---- the block's units ----------------------------------------------------------------------------------------------------
    int prev = 0;  // what the previous unit left pending in acc[1]: 0 nothing, 1 a query chunk, 2 a value chunk (+ its head's K' planes)
    auto no_ride = [&](int, int) __attribute__((always_inline)) {};
#define LAMBDA(...) [&](__VA_ARGS__) __attribute__((always_inline))
    for (int64_t u = u_lo; u < u_hi; ++u) {
        const int64_t t = u / UPT;
        const int uu = (int)(u - t * UPT);
        if (t != tile) enter_tile(t);
        if (uu < nq2) {
            // ---- two query chunks 2 uu, 2 uu + 1
            float* q_even = qg + (2 * uu) * 1024;
            if (prev == 0) stage(kindQ, acc[0], no_ride);
            else if (prev == 1) stage(kindQ, acc[0], LAMBDA(int g, int m) { ride_q(acc[1], g, m); });
            else stage(kindQ, acc[0], LAMBDA(int g, int m) { ride_v(acc[1], g, m); });
            const bool store_kv = prev == 2;
            q_pend = q_even;
            q_pend_ok = wave_ok;
            if (store_kv) stage(kindQ, acc[1], LAMBDA(int g, int m) { ride_kvstore(g, m); ride_q(acc[0], g, m); });
            else stage(kindQ, acc[1], LAMBDA(int g, int m) { ride_q(acc[0], g, m); });
            q_pend = q_even + 1024;
            prev = 1;
        } else {
            // ---- head h of layer l: K chunk, then V chunk
            const int p = uu - nq2, l = p >> 3, h = p & 7;
            if (prev == 0) stage(kindKV, acc[0], no_ride);
            else if (prev == 1) stage(kindKV, acc[0], LAMBDA(int g, int m) { ride_q(acc[1], g, m); });
            else stage(kindKV, acc[0], LAMBDA(int g, int m) { ride_v(acc[1], g, m); });
            const bool store_kv = prev == 2;
            const int valid = valid0 - 4 * half;  // per lane: the compare below is then against a literal
            constexpr std::integral_constant<bool, true> masked{};
            constexpr std::integral_constant<bool, false> whole{};
            if (valid0 < 64) {  // (idle waves: valid0 == 0)
                if (store_kv) stage(kindKV, acc[1], LAMBDA(int g, int m) { ride_kvstore(g, m); ride_k(masked, acc[0], valid, g, m); });
                else stage(kindKV, acc[1], LAMBDA(int g, int m) { ride_k(masked, acc[0], valid, g, m); });
            } else {
                if (store_kv) stage(kindKV, acc[1], LAMBDA(int g, int m) { ride_kvstore(g, m); ride_k(whole, acc[0], valid, g, m); });
                else stage(kindKV, acc[1], LAMBDA(int g, int m) { ride_k(whole, acc[0], valid, g, m); });
            }
            part_pend = part_tile + (int64_t)l * pa.kv_layer_stride + h * P_KV_ELEMS;
            part_pend_ok = wave_ok;
            prev = 2;
        }
    }
    // ---- the pipeline's end, in the open
    __builtin_amdgcn_sched_barrier(0);
    if (prev == 1) {
#pragma unroll
        for (int g = 0; g <= Q_WIN; ++g)
#pragma unroll
            for (int m = 0; m < GM; ++m) ride_q(acc[1], g, m);
    } else if (prev == 2) {
        lds_barrier();  // every wave has read the previous head's slabs (the ride of the stage just finished)
#pragma unroll
        for (int g = 0; g < 14; ++g)
#pragma unroll
            for (int m = 0; m < GM; ++m) ride_v(acc[1], g, m);
        lds_barrier();
#pragma unroll
        for (int g = 0; g < 9; ++g)
#pragma unroll
            for (int m = 0; m < GM; ++m) ride_kvstore(g, m);
    }
#undef LAMBDA
    VM_WAIT(0);  // the ring's last two stages (requested past the end) must have landed before the LDS is released
}

// W [N][256] fp32 in the row order of the q/k/v GEMM (include/scream_hip.h: q (n_q rows) | per layer: k heads 0-3 | v heads 0-3 |
// k heads 4-7 | v heads 4-7) -> the stage images of proj_ring_kernel, [S][NP][16 fragments][64 lanes][8] 16-bit values, S = N / 32,
// in the order the kernel consumes them: query chunk 0 .. 7, then per layer and head K_h, V_h.  Lane (m, half) of fragment f holds
// row 32 c + m of the chunk, contraction indices 32 (f >> 1) + chunk_k(f & 1, half, 0 .. 7) -- the same for either operand side.
template <class SP>
__global__ void pack_proj_kernel(const float* __restrict__ W, int n_q, int S, float w_scale, typename SP::vec* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S * 16 * 64) return;
    const int lane = t & 63, frag = (t >> 6) & 15, stage = t >> 10;
    const int m = lane & 31, half = lane >> 5;
    int row0;
    if (stage < n_q / 32) {
        row0 = 32 * stage;
    } else {
        const int st = stage - n_q / 32, p = st >> 1, l = p >> 3, h = p & 7, is_v = st & 1;
        row0 = n_q + l * 512 + (h >> 2) * 256 + is_v * 128 + (h & 3) * 32;
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W[(int64_t)(row0 + m) * 256 + 32 * (frag >> 1) + chunk_k(frag & 1, half, j)];
    typename SP::vec p[SP::NP];
#pragma unroll
    for (int j = 0; j < 8; ++j) SP::split1(v[j] * w_scale, j, p);
#pragma unroll
    for (int pl = 0; pl < SP::NP; ++pl) out[(((int64_t)stage * SP::NP + pl) * 16 + frag) * 64 + lane] = p[pl];
}

}  // namespace

// (the ring kernel is built for the fp16 splits only)
extern "C" int64_t scream_proj_image_bytes(int32_t N, int32_t split) {
    if (!split_fp16(split) || N <= 0 || N % 64 != 0) return SCREAM_EINVAL;
    return (int64_t)(N / 32) * split * 16 * 1024;
}

extern "C" int scream_pack_proj(const float* W, int32_t N, int32_t n_q, int32_t split, int32_t w_exp, void* image, void* stream) {
    SCREAM_REQUIRE(W && image && split_fp16(split), SCREAM_EINVAL);
    SCREAM_REQUIRE((n_q == 0 || n_q == SCREAM_D_MODEL) && N > n_q && (N - n_q) % 512 == 0, SCREAM_EUNSUPPORTED);
    SCREAM_REQUIRE(operand_exp_ok(w_exp) && aligned16(image), SCREAM_EINVAL);
    const int S = N / 32;
    const dim3 grid(S * 16 * 64 / 256), block(256);
    with_split(split, [&](auto tag) {
        typedef typename decltype(tag)::type SP;
        if constexpr (SP::SCALED)
            pack_proj_kernel<SP><<<grid, block, 0, as_stream(stream)>>>(W, n_q, S, exp2i(w_exp), reinterpret_cast<f16x8*>(image));
    });
    SCREAM_LAUNCH_CHECK();
    return 0;
}

extern "C" int scream_proj_qkv_f32(const float* x, const void* proj_image, float* Q, int64_t M, int32_t N, int32_t n_q,
                                   const int32_t* tile_cloud, const int32_t* cloud_row0, const int32_t* cloud_len,
                                   int64_t row_base, float* kv_partial, int32_t split, int32_t a_exp, int32_t w_exp, int32_t k_exp,
                                   int32_t v_exp, void* stream) {
    SCREAM_REQUIRE(split_fp16(split), SCREAM_EINVAL);
    // x and Q' are fragment-major [M,256] matrices: K, lda and ldq are the model width
    if (int rc = check_qkv(x, SCREAM_D_MODEL, proj_image, Q, SCREAM_D_MODEL, M, N, SCREAM_D_MODEL, n_q, tile_cloud, cloud_row0, cloud_len,
                           row_base, kv_partial, K_64_PLUS_192, true))
        return rc;
    SCREAM_REQUIRE(proj_exps_ok(a_exp, w_exp, k_exp, v_exp), SCREAM_EINVAL);
    SCREAM_REQUIRE(aligned16(Q) && aligned16(kv_partial), SCREAM_EINVAL);
    if (M == 0) return 0;
    ProjArgs pa;
    pa.x = x;
    pa.Wimg = reinterpret_cast<const char*>(proj_image);
    pa.Q = Q;
    pa.M = M;
    pa.n_q = n_q / 32;
    pa.S = N / 32;
    pa.kv_partial = kv_partial;
    pa.kv_layer_stride = (M / SCREAM_ROW_TILE) * SCREAM_NHEAD * (int64_t)P_KV_ELEMS;
    pa.tile_cloud = tile_cloud;
    pa.cloud_row0 = cloud_row0;
    pa.cloud_len = cloud_len;
    pa.row_base = row_base;
    pa.a_scale = exp2i(a_exp);
    pa.ec = elu1_consts(exp2i(-a_exp - w_exp));
    pa.kv_sk = exp2i(k_exp);
    pa.kv_cv = exp2i(-a_exp - w_exp + v_exp);
    pa.kv_inv = exp2i(-k_exp - v_exp);
    const int grid = persistent_grid(((M + 255) / 256) * (pa.S / 2), SCREAM_MAX_GRID, false);  // (the kernel numbers its units in 64 bits)
    with_split(split, [&](auto tag) {
        typedef typename decltype(tag)::type SP;
        if constexpr (SP::SCALED) proj_ring_kernel<SP><<<dim3(grid), dim3(TT), 0, as_stream(stream)>>>(pa);
    });
    SCREAM_LAUNCH_CHECK();
    return 0;
}
