// kernels_mq_i8.hip -- the exact integer shared sweeps (mq_device.h), one object per row width: -DSZG_ROW_BITS=8 | 4.
#include "mq_device.h"
#ifndef SZG_ROW_BITS
#error "build with -DSZG_ROW_BITS=8|4"
#endif

namespace szg {

namespace {

#ifndef SZG_MQ_RING
#define SZG_MQ_RING 4  // 16-byte loads per lane in flight (4 vs 6: -1.5 % on the int8 sweeps, no change on f32)
#endif
constexpr int kRingMq = SZG_MQ_RING;
constexpr int kMq8Threads = 64 * SZG_MQ8_WAVES;

// ---- exact integer shared sweep, 8-bit rows and 4-bit rows ---------------------------------------
//
// With v' = v - 128 (one xor per dword) the decoded element is n = 2v' + 1, and the
// prepared query is the integer vector Q = 16384 h + 128 m + l of balanced int8 digits
// (prep_query, the same planes the single-query integer path uses).  One
// v_mfma_i32_16x16x64_i8 per digit plane multiplies 64 elements of 16 rows with 16
// queries, exactly: B operand = the row bytes as they come from HBM (lane = chunk*16 +
// row holds 16 consecutive elements), A operand = the plane's bytes from LDS (lane =
// chunk*16 + query, same elements).  Both operands use the same lane -> K mapping, so the
// products pair element with element whatever the hardware's K order is.  The row norm
// comes from two v_dot4_i32_i8 per dword.  The finish is RowAcc<8>::finish's, so the key
// and its error bound (key_eps, integer branch) are the single-query path's.
typedef int v4i32 __attribute__((ext_vector_type(4)));

template <int NB, int METRIC, bool COLLECT, bool FAST = false, int RB = 8>
__global__ __launch_bounds__(kMq8Threads) void mq_score_i8_kernel(const MqArgs a)
{
    // RB = 8: one B operand per 16-byte piece (the bytes, xor 0x80).  RB = 4: two -- the
    // high nibbles (even elements) and the low nibbles (odd elements) as unsigned bytes
    // 0..15, against the digit planes of the even / odd elements; n = 2x - 15 turns
    // sum Q x into sum Q n on the host side of the constants table.
    constexpr int T = RB == 4 ? 2 : 1;
    constexpr int NPL = kMqPlanes;  // digit planes of the query (radix 128)
    // prefetch the A operands one step ahead -- where the registers are there: with three query blocks the prefetched
    // set (48 VGPRs for 4-bit rows) pushed these kernels over the 168 registers of 12 waves per CU and they spilled
    // 8-21 of them (round 3's builds; -Rpass-analysis=kernel-resource-usage, scripts/kernel_resources.sh)
    constexpr bool PF = NB < 3;
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int r16 = a.r16;
    const int steps = (r16 + 3) / 4;  // 64-byte steps per row
    const RowLayout mlay{a.pitch, a.tiled, a.steps};
    const uint32_t istep = a.tiled ? 1024u : 64u;  // bytes from one 64-byte step of a row to the next
    const int n16 = steps * NPL * T * NB * 64;  // image, 16-byte words
    // One launch walks the passes of up to two query groups (48 queries each) back to back, as the
    // single-query scan walks its sweeps: a 0.13 ms pass at 1M rows otherwise pays its start-up and its
    // tail (9 %) once per launch.  Both groups' images are staged in LDS up front (2 x 73 KiB at 768
    // dims), so a wave that finishes its share of the first pass goes straight on to the second.
    const int n_groups = a.n_groups > 0 ? a.n_groups : 1;
    const size_t grp_lds = (size_t)n16 * 16 + 4 * 48 * sizeof(float);  // image | qscale, qconst, qnorm2 | thresholds
    for (int g = 0; g < n_groups; g++) {
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.queries) +
                                                           (size_t)g * a.group_stride);
        uint4 *dst = reinterpret_cast<uint4 *>(smem + (size_t)g * grp_lds);
        const int n = n16 + (3 * 48 * 4) / 16;  // + constants table
        stage_image(dst, src, n, tid, blockDim.x);
        if (COLLECT && tid < 48)
            reinterpret_cast<float *>(smem + (size_t)g * grp_lds + (size_t)n * 16)[tid] =
                g * 48 + tid < a.n_queries ? a.thr[g * 48 + tid] : -3.0e38f;
    }
    HitBuf hb;
    {
        uint8_t *base = smem + (size_t)n_groups * grp_lds;
        hb.cand = reinterpret_cast<uint64_t *>(base) + (size_t)wave * kHitCap;
        hb.query = base + (size_t)nwaves * kHitCap * 8 + (size_t)wave * kHitCap;
        hb.n = 0;
    }
    for (int grp = 0; grp < n_groups; grp++) {
    const int qoff = grp * 48;  // first query of the group
    const uint8_t *gbase = smem + (size_t)grp * grp_lds;
    // (the barrier that publishes the image comes after the ring's first loads have been issued:
    // the rows do not depend on it, and a 140 us sweep notices a 5 us start-up)
    const v4i32 *qimg = reinterpret_cast<const v4i32 *>(gbase);
    const float *qtab = reinterpret_cast<const float *>(gbase + (size_t)n16 * 16);
    const float *thr_lds = qtab + 3 * 48;

    const int trow = lane & 15;
    const int c = lane >> 4;
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
    const uint64_t tile_stride = (uint64_t)gridDim.x * nwaves;
    const uint64_t tile_first = (uint64_t)blockIdx.x * nwaves + wave;
    const uint64_t n_it = tile_first < n_tiles ? (n_tiles - tile_first + tile_stride - 1) / tile_stride : 0;
    const uint64_t NP = n_it * (uint64_t)steps;

    uint64_t itile = tile_first;
    int is = 0;
    uint64_t ctile = tile_first;
    int cs = 0;

    u32x4 ring[kRingMq];
    v4i32 acc[NPL][NB];
#pragma unroll
    for (int p = 0; p < NPL; p++)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[p][b] = v4i32{0, 0, 0, 0};
    int SQ = 0, SV = 0;
    const int qstep8 = NPL * T * NB * 64;  // 16-byte words of the image per 64-byte step
    // A operands of the step about to be multiplied (fetched one step ahead when PF)
    v4i32 qn[NPL][T][NB];

    // FAST (r16 % 4 == 0): no range predicates, addresses advance by constants
    auto row_ptr = [&](uint64_t tile) -> const uint8_t * {
        const uint64_t r = min(tile * 16 + trow, (uint64_t)a.n_rows - 1);
        return a.rows + piece_offset(mlay, r, (uint32_t)c);
    };
    const uint8_t *iptr = row_ptr(tile_first);

#define MQ8F_ISSUE(u)                                                                    \
    {                                                                                    \
        ring[u] = load_stream<true>(iptr); /* FAST: tiled */                                      \
        if (++is == steps) {                                                             \
            is = 0;                                                                      \
            itile += tile_stride;                                                        \
            iptr = row_ptr(itile);                                                       \
        } else {                                                                         \
            iptr += istep;                                                               \
        }                                                                                \
    }

#define MQ8_ISSUE(u)                                                                     \
    {                                                                                    \
        const uint64_t row_ = itile * 16 + trow;                                         \
        const int j_ = is * 4 + c;                                                       \
        const bool ok_ = row_ < a.n_rows && j_ < r16;                                    \
        ring[u] = load_plain(ok_ ? a.rows + piece_offset(mlay, row_, (uint32_t)j_) : a.zero16); \
        if (++is == steps) {                                                             \
            is = 0;                                                                      \
            itile += tile_stride;                                                        \
        }                                                                                \
    }

    // PRED: the piece may be the dummy one (not part of the row): its operands become 0
#define MQ8_CONSUME_X(u, PRED)                                                           \
    {                                                                                    \
        const u32x4 v_ = ring[u];                                                        \
        const bool in_ = !(PRED) || cs * 4 + c < r16;                                    \
        const uint32_t raw_[4] = {v_.x, v_.y, v_.z, v_.w};                               \
        v4i32 bop_[T];                                                                   \
        int wn_[4];                                                                      \
        _Pragma("unroll") for (int d = 0; d < 4; d++)                                    \
        {                                                                                \
            if (RB == 8) {                                                               \
                wn_[d] = in_ ? (int)(raw_[d] ^ 0x80808080u) : 0;                         \
                bop_[0][d] = wn_[d];                                                     \
            } else {                                                                     \
                wn_[d] = in_ ? (int)(raw_[d] ^ 0x88888888u) : 0;                         \
                bop_[0][d] = in_ ? (int)((raw_[d] >> 4) & 0x0F0F0F0Fu) : 0;              \
                bop_[T - 1][d] = in_ ? (int)(raw_[d] & 0x0F0F0F0Fu) : 0;                 \
            }                                                                            \
        }                                                                                \
        v4i32 qc_[NPL][T][NB];                                                            \
        const int qcur_ = lane + cs * qstep8;                                            \
        const int qnext_ = lane + (cs + 1 == steps ? 0 : cs + 1) * qstep8;               \
        _Pragma("unroll") for (int p = 0; p < NPL; p++)                                   \
            _Pragma("unroll") for (int t = 0; t < T; t++)                                \
                _Pragma("unroll") for (int b = 0; b < NB; b++)                           \
                {                                                                        \
                    if (PF) {                                                            \
                        qc_[p][t][b] = qn[p][t][b];                                      \
                        qn[p][t][b] = qimg[qnext_ + ((p * T + t) * NB + b) * 64];        \
                    } else {                                                             \
                        qc_[p][t][b] = qimg[qcur_ + ((p * T + t) * NB + b) * 64];        \
                    }                                                                    \
                }                                                                        \
        _Pragma("unroll") for (int t = 0; t < T; t++)                                    \
            _Pragma("unroll") for (int p = 0; p < NPL; p++)                               \
                _Pragma("unroll") for (int b = 0; b < NB; b++)                           \
                {                                                                        \
                    acc[p][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qc_[p][t][b], bop_[t], acc[p][b], 0, 0, 0); \
                }                                                                        \
        _Pragma("unroll") for (int d = 0; d < 4; d++)                                    \
        {                                                                                \
            if (RB == 8) {                                                               \
                SQ = __builtin_amdgcn_sdot4(wn_[d], wn_[d], SQ, false);                  \
                SV = __builtin_amdgcn_sdot4(wn_[d], 0x01010101, SV, false);              \
            } else {                                                                     \
                SQ = __builtin_amdgcn_sdot8(wn_[d], wn_[d], SQ, false);                  \
                SV = __builtin_amdgcn_sdot8(wn_[d], 0x11111111, SV, false);              \
            }                                                                            \
        }                                                                                \
        if (++cs == steps) {                                                             \
            finish_tile8(ctile);                                                         \
            cs = 0;                                                                      \
            ctile += tile_stride;                                                        \
        }                                                                                \
    }
#define MQ8_CONSUME(u) MQ8_CONSUME_X(u, true)
#define MQ8F_CONSUME(u) MQ8_CONSUME_X(u, false)

    auto finish_tile8 = [&](uint64_t tile) {
        int nrm = 4 * (SQ + SV);
        nrm += __shfl_xor(nrm, 16);
        nrm += __shfl_xor(nrm, 32);
        const float norm = (float)nrm + a.norm_bias;
        const float inv = __frsqrt_rn(norm);
        const uint64_t row = tile * 16 + trow;
        if (COLLECT || row < a.n_rows) {
            float keys[NB][4];
            uint32_t hm = 0;
            const bool row_ok = row < a.n_rows;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                // this lane's four queries of block b are consecutive: 16-byte reads of the tables
                const int q0 = b * 16 + c * 4;
                const float4 qs4 = *reinterpret_cast<const float4 *>(qtab + q0);
                const float4 qc4 = *reinterpret_cast<const float4 *>(qtab + 48 + q0);
                const float4 qn4 = METRIC == kCosine ? make_float4(0.f, 0.f, 0.f, 0.f)
                                                     : *reinterpret_cast<const float4 *>(qtab + 96 + q0);
                const float4 th4 = COLLECT ? *reinterpret_cast<const float4 *>(thr_lds + q0)
                                           : make_float4(0.f, 0.f, 0.f, 0.f);
                const float qsv[4] = {qs4.x, qs4.y, qs4.z, qs4.w}, qcv[4] = {qc4.x, qc4.y, qc4.z, qc4.w};
                const float qnv[4] = {qn4.x, qn4.y, qn4.z, qn4.w}, thv[4] = {th4.x, th4.y, th4.z, th4.w};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int q = q0 + r;
                    float dot = (float)acc[0][b][r];  // plane 0 = the top digit
#pragma unroll
                    for (int p = 1; p < NPL; p++) dot = fmaf(128.0f, dot, (float)acc[p][b][r]);
                    const float d2 = fmaf(2.0f, dot, qcv[r]);  // sum Q n
                    float key;
                    if (METRIC == kCosine)
                        key = -(d2 * qsv[r]) * inv;
                    else
                        key = fmaf(-2.0f * qsv[r], d2, qnv[r] + norm);
                    // (finite by construction: integer sums, norm >= dim > 0 -- no NaN / inf clamps)
                    keys[b][r] = key;
                    if (COLLECT)
                        hm |= (uint32_t)(row_ok & (key <= thv[r])) << (b * 4 + r);  // unused queries: thr = -3e38
                    else if (qoff + q < a.n_queries)
                        a.keys[(size_t)(qoff + q) * a.key_stride + row] = key;
                }
            }
            if (COLLECT) offer_tile_hits<NB>(a, hb, lane, c, hm, keys, row, qoff);
        }
        if (!COLLECT) __builtin_amdgcn_s_waitcnt(0x0F70);  // drain the key stores: gfx9 counts loads and stores in ONE vmcnt, a pending store would turn every ring wait into vmcnt(0)
#pragma unroll
        for (int p = 0; p < NPL; p++)
#pragma unroll
            for (int b = 0; b < NB; b++) acc[p][b] = v4i32{0, 0, 0, 0};
        SQ = 0;
        SV = 0;
    };

#define MQ8_RUN_RING(ISSUE, CONSUME)                                                     \
    {                                                                                    \
        uint64_t issued = kRingMq, consumed = 0;                                         \
        _Pragma("unroll") for (int u = 0; u < kRingMq; u++)                              \
        {                                                                                \
            ISSUE(u)                                                                     \
            __builtin_amdgcn_sched_barrier(0);                                           \
        }                                                                                \
        if (grp == 0) __syncthreads(); /* the query images are complete */               \
        if (PF) {                                                                        \
            _Pragma("unroll") for (int p = 0; p < NPL; p++)                              \
                _Pragma("unroll") for (int t = 0; t < T; t++)                            \
                    _Pragma("unroll") for (int b = 0; b < NB; b++)                       \
                        qn[p][t][b] = qimg[((p * T + t) * NB + b) * 64 + lane];          \
        }                                                                                \
        while (consumed + 2 * kRingMq <= NP) {                                           \
            _Pragma("unroll") for (int u = 0; u < kRingMq; u++)                          \
            {                                                                            \
                CONSUME(u)                                                               \
                ISSUE(u)                                                                 \
                __builtin_amdgcn_sched_barrier(0);                                       \
            }                                                                            \
            consumed += kRingMq;                                                         \
            issued += kRingMq;                                                           \
        }                                                                                \
        while (consumed < NP) {                                                          \
            _Pragma("unroll") for (int u = 0; u < kRingMq; u++)                          \
            {                                                                            \
                if (consumed < NP) {                                                     \
                    CONSUME(u)                                                           \
                    consumed++;                                                          \
                    if (issued < NP) {                                                   \
                        ISSUE(u)                                                         \
                        issued++;                                                        \
                    }                                                                    \
                }                                                                        \
            }                                                                            \
        }                                                                                \
    }
    if (FAST)
        MQ8_RUN_RING(MQ8F_ISSUE, MQ8F_CONSUME)
    else
        MQ8_RUN_RING(MQ8_ISSUE, MQ8_CONSUME)
    }  // groups
    if (COLLECT) hit_flush(a, hb, lane);  // once for both groups (see mq_score_i8s_kernel)
#undef MQ8F_ISSUE
#undef MQ8F_CONSUME
#undef MQ8_CONSUME_X
#undef MQ8_RUN_RING
#undef MQ8_ISSUE
#undef MQ8_CONSUME
}

// ---- the same sweep with the row shape fixed at compile time ----------------------------------------------------
//
// STEPS = 64-byte steps per row (12 for 768 8-bit dims, 6 for 768 4-bit or 384 8-bit, 3 for 384 4-bit).  The loop
// walks one TILE per iteration, its STEPS steps unrolled with slot = step % D (D divides STEPS), so every load
// address is `tile pointer + constant`, every A operand an LDS read at a constant offset, the ring wait a fixed
// vmcnt(D-1), and there is ONE copy of the tile finish (the rotating-slot loop above carries four, each with the
// inlined hit path: 13 000 lines of ISA).  Whole 64-byte steps of tiled rows, fused selection only; other shapes
// keep mq_score_i8_kernel.  Measured against it (1M rows, ms per 48-query pass): 768 dims 8-bit 0.122 / 0.134,
// 768 dims 4-bit 0.088 / 0.092, 384 dims 4-bit 0.053 / 0.062 (profiles/r03_i8_sweep_experiments.txt, which also
// has the probe -- scripts/readbw -- that found the int8 sweeps running without their non-temporal hint).
// Per-query constants of the shape kernels' hit PRE-TEST (see the kernel's tile finish).  With g = sum Q n (a float)
// the key is  cosine: -fl(fl(g qs) inv)   Euclidean: fl(fma(-2 qs, g, fl(qn + norm))),  and a hit is key <= thr.
//   cosine:     key <= thr  ==>  g inv >= (-thr - 4e-7 |thr|) / qs =: T             pre-test  fma(g, inv, w) >= 0, w = -T
//   Euclidean:  key <= thr  ==>  2 qs g - norm (1 - 6e-8) >= qn - thr - 2e-6 (qn + |thr|) =: V
//                                                          pre-test  fma(g, s, w) >= norm (1 - 2e-6), s = 2 qs, w = -V
// (two roundings of 2^-24 each in the cosine chain, one plus the rounded qn + norm in the Euclidean one; the margins
// are several times that, and the float forms of w are nudged two more ulps towards "pass").  A query the algebra
// does not cover (qs <= 0, a NaN anywhere) gets w = +inf: every tile takes the exact path for it.  An unused query
// slot (thr = -3e38) gets w = -inf.
template <int METRIC>
__device__ __forceinline__ void pretest_consts(float thr, float qs, float qn, float *ps, float *pw)
{
    float s = 0.0f, w;
    if (thr <= -3.0e38f) {
        w = -__builtin_inff();
    } else if (METRIC == kCosine) {
        const double T = (-(double)thr - 4.0e-7 * fabs((double)thr)) / (double)qs;
        w = (float)(-T);
        w += fabsf(w) * 2.4e-7f + 1.0e-37f;
        if (!(qs > 0.0f) || w != w) w = __builtin_inff();
    } else {
        const double V = (double)qn - (double)thr - 2.0e-6 * (fabs((double)qn) + fabs((double)thr));
        s = 2.0f * qs;
        w = (float)(-V);
        w += fabsf(w) * 2.4e-7f + 1.0e-37f;
        if (!(qs > 0.0f) || !(qn >= 0.0f) || w != w) w = __builtin_inff();
    }
    *ps = s;
    *pw = w;
}

// Waves per CU and ring depth (16-byte loads per lane in flight; divides STEPS) of the shape kernels.  768-byte rows
// (12 steps): 8 waves with 6 KiB each in flight -- 0.122 ms per 1M-row pass against 0.134 with 12 x 4, fewer waves
// queueing behind one another's tile finish.  Shorter rows have a finish per fewer bytes and want the 12 waves
// (384 bytes: 0.069 against 0.075; 192: 0.046 against 0.052), and so do 4-bit rows with twice the arithmetic per byte.
#ifndef SZG_S12_WAVES
#define SZG_S12_WAVES 8
#endif
#ifndef SZG_S12_RING
#define SZG_S12_RING 6
#endif
#ifndef SZG_S6_RING
#define SZG_S6_RING 3
#endif
#ifndef SZG_I8S_RN
#define SZG_I8S_RN 1  // the shape kernels take the rows' norms from the resident array (MqArgs::row_norm) instead of summing them
#endif
template <int RB, int STEPS>
constexpr int i8s_waves()
{   // (4-bit rows of 12 steps -- 1 536 dims -- at 12 waves per CU spilled 2-4 of their 168 registers: 8 waves, 256)
    return STEPS == 12 ? SZG_S12_WAVES : SZG_MQ8_WAVES;
}
template <int RB, int STEPS>
constexpr int i8s_ring()
{
    if (RB == 8 && STEPS == 12) return SZG_S12_RING;
    if (RB == 8 && STEPS == 6) return SZG_S6_RING;
#ifdef SZG_S6R4_RING
    if (RB == 4 && STEPS == 6) return SZG_S6R4_RING;
#endif
    return STEPS % 4 == 0 ? 4 : (STEPS % 3 == 0 ? 3 : (STEPS % 2 == 0 ? 2 : 1));
}
template <int NB, int METRIC, int RB, int STEPS>
__global__ __launch_bounds__((64 * i8s_waves<RB, STEPS>())) void mq_score_i8s_kernel(const MqArgs a)
{
    constexpr int T = RB == 4 ? 2 : 1;
    constexpr int NPL = kMqPlanes;
    constexpr int D = i8s_ring<RB, STEPS>();
    static_assert(NPL == 2, "the integer plane combine in the tile finish assumes two digit planes");
    constexpr int QSTEP = NPL * T * NB * 64;  // 16-byte words of the image per 64-byte step
    constexpr int N16 = STEPS * QSTEP;
    constexpr bool RN = SZG_I8S_RN != 0;
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const RowLayout mlay{a.pitch, a.tiled, a.steps};
    const uint32_t istep = a.tiled ? 1024u : 64u;
    const int n_groups = a.n_groups > 0 ? a.n_groups : 1;
    constexpr size_t grp_lds = (size_t)N16 * 16 + kMq8TableRows * 48 * sizeof(float);  // image | qscale, qconst, qnorm2 | thresholds, pre-test s, w
    for (int g = 0; g < n_groups; g++) {
        const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.queries) +
                                                           (size_t)g * a.group_stride);
        uint4 *dst = reinterpret_cast<uint4 *>(smem + (size_t)g * grp_lds);
        constexpr int n = N16 + (3 * 48 * 4) / 16;  // + constants table
        stage_image(dst, src, n, tid, blockDim.x);
        if (tid < 48) {
            float *tab = reinterpret_cast<float *>(smem + (size_t)g * grp_lds + (size_t)n * 16);
            const float thr = g * 48 + tid < a.n_queries ? a.thr[g * 48 + tid] : -3.0e38f;
            const float *qconsts = reinterpret_cast<const float *>(src + N16);  // qscale | qconst | qnorm2
            float ps, pw;
            pretest_consts<METRIC>(thr, qconsts[tid], qconsts[96 + tid], &ps, &pw);
            tab[tid] = thr;
            tab[48 + tid] = ps;
            tab[96 + tid] = pw;
        }
    }
    const int trow = lane & 15;
    const int c = lane >> 4;
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
    const uint64_t tile_stride = (uint64_t)gridDim.x * nwaves;
    const uint64_t tile_first = (uint64_t)blockIdx.x * nwaves + wave;
    const uint64_t n_it = tile_first < n_tiles ? (n_tiles - tile_first + tile_stride - 1) / tile_stride : 0;
    auto row_ptr = [&](uint64_t tile) -> const uint8_t * {
        const uint64_t r = min(tile * 16 + trow, (uint64_t)a.n_rows - 1);  // past the end: a valid row, discarded
        return a.rows + piece_offset(mlay, r, (uint32_t)c);
    };
    HitBuf hb;
    {
        uint8_t *base = smem + (size_t)n_groups * grp_lds;
        hb.cand = reinterpret_cast<uint64_t *>(base) + (size_t)wave * kHitCap;
        hb.query = base + (size_t)nwaves * kHitCap * 8 + (size_t)wave * kHitCap;
        hb.n = 0;
    }

    for (int grp = 0; grp < n_groups; grp++) {
        const int qoff = grp * 48;
        const uint8_t *gbase = smem + (size_t)grp * grp_lds;
        const v4i32 *qimg = reinterpret_cast<const v4i32 *>(gbase) + lane;
        const float *qtab = reinterpret_cast<const float *>(gbase + (size_t)N16 * 16);
        const float *thr_lds = qtab + 3 * 48;
        u32x4 ring[D];
        v4i32 acc[NPL][NB];
#pragma unroll
        for (int p = 0; p < NPL; p++)
#pragma unroll
            for (int b = 0; b < NB; b++) acc[p][b] = v4i32{0, 0, 0, 0};
        int SQ = 0, SV = 0;
        uint64_t tile = tile_first;
        const uint8_t *cur = row_ptr(tile);
        // the ring's first D steps (D <= STEPS: all inside the first tile)
#pragma unroll
        for (int u = 0; u < D; u++) {
            ring[u] = load_stream<true>(cur + (size_t)u * istep);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (grp == 0) __syncthreads();  // the query images are complete (the rows do not depend on them)
        // The A operands travel one PHASE ahead of the matrix instructions that use them.  A phase is the G = NPL x NB
        // operands of one (step, nibble half); while the G MFMAs of phase ph issue (G x 16 cycles), the G ds_read_b128
        // of phase ph + 1 are in flight into the other half of a double buffer.  Round 3's form left the reads to the
        // compiler, which issued each one or two instructions ahead of the MFMA that needs it (84 reads, 72 MFMAs and
        // an `s_waitcnt lgkmcnt` before nearly every one of them in the 4-bit 6-step kernel): every wave paid the LDS
        // latency once per couple of MFMAs and the other two waves of its SIMD were all that hid it.  sched_barriers pin
        // the order read-group / MFMA-group; the decode of the row bytes shares the MFMA groups' regions, where the
        // scheduler slots it into the matrix instructions' shadows.  (Needs an even number of phases per tile, so that
        // the buffer halves are compile-time facts: 8-bit rows of 3 steps keep the plain form.)  Same box, 1M x 768
        // 4-bit: 0.092 -> 0.084 ms per pass.
        constexpr int G = NPL * NB, PHASES = STEPS * T;
        constexpr bool PIPE = PHASES % 2 == 0;
        v4i32 qbuf[2][G];
        auto read_phase = [&](int ph, v4i32 (&dst)[G]) {
            const int st_ = ph / T, t_ = ph % T;
#pragma unroll
            for (int p = 0; p < NPL; p++)
#pragma unroll
                for (int b = 0; b < NB; b++) dst[p * NB + b] = qimg[st_ * QSTEP + ((p * T + t_) * NB + b) * 64];
        };
        if (PIPE) read_phase(0, qbuf[0]);
        for (uint64_t it = 0; it < n_it; it++, tile += tile_stride) {
            // (past the wave's last tile: its own tile again -- D loads nobody consumes)
            const uint8_t *nxt = it + 1 < n_it ? row_ptr(tile + tile_stride) : cur;
            // resident norms: the tile's 16 arrive while its steps run (the decode below then spends nothing on them:
            // 12 of its 24 vector instructions per 64-byte step of 4-bit rows, 8 of 12 for 8-bit rows)
            float norm_res = 0.f;
            if constexpr (RN) norm_res = a.row_norm[min(tile * 16 + trow, (uint64_t)a.n_rows - 1)];
#pragma unroll
            for (int st = 0; st < STEPS; st++) {
                const u32x4 v_ = ring[st % D];
                // this slot's next load: the step D ahead, in this tile or the next
                ring[st % D] = st + D < STEPS ? load_stream<true>(cur + (size_t)(st + D) * istep)
                                              : load_stream<true>(nxt + (size_t)(st + D - STEPS) * istep);
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t raw_[4] = {v_.x, v_.y, v_.z, v_.w};
                v4i32 bop_[T];
                if constexpr (PIPE) {
                    // region 0: the first operand of the step, and the NEXT phase's reads
#pragma unroll
                    for (int d = 0; d < 4; d++)
                        bop_[0][d] = RB == 8 ? (int)(raw_[d] ^ 0x80808080u) : (int)((raw_[d] >> 4) & 0x0F0F0F0Fu);
                    read_phase((st * T + 1) % PHASES, qbuf[(st * T + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    // region 1: G MFMAs of phase st * T, with the rest of the decode in their shadows
                    // (the tile's first matrix instructions start from a literal zero: no accumulator clearing per tile)
#pragma unroll
                    for (int g = 0; g < G; g++)
                        acc[g / NB][g % NB] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                            qbuf[(st * T) & 1][g], bop_[0], st == 0 ? v4i32{0, 0, 0, 0} : acc[g / NB][g % NB], 0, 0, 0);
                    if constexpr (RB == 8) {
                        if constexpr (!RN) {
#pragma unroll
                            for (int d = 0; d < 4; d++) {
                                SQ = __builtin_amdgcn_sdot4(bop_[0][d], bop_[0][d], SQ, false);
                                SV = __builtin_amdgcn_sdot4(bop_[0][d], 0x01010101, SV, false);
                            }
                        }
                    } else {
#pragma unroll
                        for (int d = 0; d < 4; d++) bop_[T - 1][d] = (int)(raw_[d] & 0x0F0F0F0Fu);
                        __builtin_amdgcn_sched_barrier(0);
                        // region 2: the reads of the phase after next;  region 3: the low nibbles' MFMAs + the norm
                        read_phase((st * T + 2) % PHASES, qbuf[(st * T + 2) & 1]);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int g = 0; g < G; g++)
                            acc[g / NB][g % NB] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qbuf[(st * T + 1) & 1][g], bop_[T - 1],
                                                                                      acc[g / NB][g % NB], 0, 0, 0);
                        if constexpr (!RN) {
#pragma unroll
                            for (int d = 0; d < 4; d++) {
                                const int wn_ = (int)(raw_[d] ^ 0x88888888u);
                                SQ = __builtin_amdgcn_sdot8(wn_, wn_, SQ, false);
                                SV = __builtin_amdgcn_sdot8(wn_, 0x11111111, SV, false);
                            }
                        }
                    }
                } else {
#pragma unroll
                    for (int d = 0; d < 4; d++) {
                        if (RB == 8) {
                            const int wn_ = (int)(raw_[d] ^ 0x80808080u);
                            bop_[0][d] = wn_;
                            if constexpr (!RN) {
                                SQ = __builtin_amdgcn_sdot4(wn_, wn_, SQ, false);
                                SV = __builtin_amdgcn_sdot4(wn_, 0x01010101, SV, false);
                            }
                        } else {
                            const int wn_ = (int)(raw_[d] ^ 0x88888888u);
                            bop_[0][d] = (int)((raw_[d] >> 4) & 0x0F0F0F0Fu);
                            bop_[T - 1][d] = (int)(raw_[d] & 0x0F0F0F0Fu);
                            if constexpr (!RN) {
                                SQ = __builtin_amdgcn_sdot8(wn_, wn_, SQ, false);
                                SV = __builtin_amdgcn_sdot8(wn_, 0x11111111, SV, false);
                            }
                        }
                    }
#pragma unroll
                    for (int t = 0; t < T; t++)
#pragma unroll
                        for (int p = 0; p < NPL; p++)
#pragma unroll
                            for (int b = 0; b < NB; b++) {
                                const v4i32 qc_ = qimg[st * QSTEP + ((p * T + t) * NB + b) * 64];
                                acc[p][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                                    qc_, bop_[t], st == 0 && t == 0 ? v4i32{0, 0, 0, 0} : acc[p][b], 0, 0, 0);
                            }
                }
            }
            // ---- the tile is done: row norms across the 4 chunk lanes, then the hit test in two stages.  On a large
            // shard a tile of 16 rows x 48 queries holds a hit a few times in a hundred (a radius batch: far less), so
            // every tile pays only a PRE-TEST of ~4 VALU instructions per (row, query) -- one integer combine, one
            // convert, two fmas, a running max -- against per-query constants staged with a safety margin
            // (pretest_consts), and only a tile in which some lane passes it forms the keys proper and tests them
            // against the thresholds.  The pre-test passes whenever key <= thr would (the same inequality solved for
            // the integer dot product, the rounding of the key's float chain covered by the margin), so the hits are
            // exactly the one-stage test's.  (1M rows with the default 1 024 expected hits per query: more than half
            // the tiles hold a hit and the two-stage form measures the same as the one-stage form; 12.5M rows: see
            // profiles/r03_i8_sweep_experiments.txt, section 11.)
            float norm;
            if constexpr (RN) {
                norm = norm_res;
            } else {
                int nrm = 4 * (SQ + SV);
                nrm += __shfl_xor(nrm, 16);
                nrm += __shfl_xor(nrm, 32);
                norm = (float)nrm + a.norm_bias;
            }
            const float inv = __frsqrt_rn(norm);
            const uint64_t row = tile * 16 + trow;
            const bool row_ok = row < a.n_rows;
            // (d2 = sum Q n of a pair, the float its key is made of, is formed again in the rare second stage rather than
            // kept: twelve registers that the prefetched operands of the next tile need more)
            auto pair_d2 = [&](int b, int r, float qc) -> float {
                // planes combined as integers: |plane sums| < 2^24 and |dot| < 2^31 for these row shapes, so the one
                // conversion rounds exactly as fmaf(128, float(acc0), float(acc1)) does (the generic kernel's form,
                // which the prefix pass made the thresholds with)
                int di = acc[0][b][r];
#pragma unroll
                for (int p = 1; p < NPL; p++) di = di * 128 + acc[p][b][r];
                return fmaf(2.0f, (float)di, qc);
            };
            float best = -__builtin_inff();
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const int q0 = b * 16 + c * 4;
                const float4 qc4 = *reinterpret_cast<const float4 *>(qtab + 48 + q0);
                const float4 ps4 = *reinterpret_cast<const float4 *>(thr_lds + 48 + q0);
                const float4 pw4 = *reinterpret_cast<const float4 *>(thr_lds + 96 + q0);
                const float qcv[4] = {qc4.x, qc4.y, qc4.z, qc4.w};
                const float psv[4] = {ps4.x, ps4.y, ps4.z, ps4.w}, pwv[4] = {pw4.x, pw4.y, pw4.z, pw4.w};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float g = pair_d2(b, r, qcv[r]);
                    const float e = METRIC == kCosine ? fmaf(g, inv, pwv[r]) : fmaf(g, psv[r], pwv[r]);
                    best = fmaxf(best, e);
                }
            }
            const bool pass = row_ok && best >= (METRIC == kCosine ? 0.0f : norm * (1.0f - 2.0e-6f));
            if (__ballot(pass)) {
                float keys[NB][4];
                uint32_t hm = 0;
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    const int q0 = b * 16 + c * 4;
                    const float4 qs4 = *reinterpret_cast<const float4 *>(qtab + q0);
                    const float4 qc4 = *reinterpret_cast<const float4 *>(qtab + 48 + q0);
                    const float4 qn4 = METRIC == kCosine ? make_float4(0.f, 0.f, 0.f, 0.f)
                                                         : *reinterpret_cast<const float4 *>(qtab + 96 + q0);
                    const float4 th4 = *reinterpret_cast<const float4 *>(thr_lds + q0);
                    const float qsv[4] = {qs4.x, qs4.y, qs4.z, qs4.w}, qcv[4] = {qc4.x, qc4.y, qc4.z, qc4.w};
                    const float qnv[4] = {qn4.x, qn4.y, qn4.z, qn4.w}, thv[4] = {th4.x, th4.y, th4.z, th4.w};
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float d2 = pair_d2(b, r, qcv[r]);
                        float key;
                        if (METRIC == kCosine)
                            key = -(d2 * qsv[r]) * inv;
                        else
                            key = fmaf(-2.0f * qsv[r], d2, qnv[r] + norm);
                        keys[b][r] = key;
                        hm |= (row_ok & (key <= thv[r])) ? (1u << (b * 4 + r)) : 0u;  // unused queries: thr = -3e38
                    }
                }
                offer_tile_hits<NB>(a, hb, lane, c, hm, keys, row, qoff);
            }
            SQ = 0;
            SV = 0;
            cur = nxt;
        }
    }
    // one flush for both groups (the buffered query index carries the group): a flush is a returning atomic per hit
    // and a drained load queue -- a memory round trip with nothing in flight, which at the end of every pass cost 3 %
    hit_flush(a, hb, lane);
}

template <int NB, int METRIC, int RB>
bool launch_mq_score_i8s(const MqArgs &a, int grid, size_t lds, hipStream_t stream, hipError_t *e)
{
    switch (a.r16 / 4) {  // the row shapes with a kernel of their own (768 / 384 dims, 8- and 4-bit)
    case 12: *e = launch_lds(&mq_score_i8s_kernel<NB, METRIC, RB, 12>, grid, 64 * i8s_waves<RB, 12>(), lds, stream, a); return true;
    case 6: *e = launch_lds(&mq_score_i8s_kernel<NB, METRIC, RB, 6>, grid, 64 * i8s_waves<RB, 6>(), lds, stream, a); return true;
    case 3: *e = launch_lds(&mq_score_i8s_kernel<NB, METRIC, RB, 3>, grid, 64 * i8s_waves<RB, 3>(), lds, stream, a); return true;
    default: return false;
    }
}
template <int NB, int RB>
hipError_t launch_mq_score_i8_m(const MqArgs &a, int grid, size_t lds, hipStream_t stream)
{
    return with_metric_collect(a, [&](auto metric, auto collect) -> hipError_t {
        const bool whole = a.tiled && a.r16 % 4 == 0 && a.n_rows > 0;  // whole 64-byte steps of tiled rows
        if constexpr (collect && NB == 3) {  // full query groups: the row shapes with a kernel of their own
            hipError_t e = hipSuccess;
            if (a.shape_kernels && whole && (!SZG_I8S_RN || a.row_norm) && launch_mq_score_i8s<NB, metric, RB>(a, grid, lds, stream, &e))
                return e;
        }
        if constexpr (collect) {
            if (whole)  // the predicate-free kernel
                return launch_lds(&mq_score_i8_kernel<NB, metric, true, true, RB>, grid, kMq8Threads, lds, stream, a);
        }
        return launch_lds(&mq_score_i8_kernel<NB, metric, collect, false, RB>, grid, kMq8Threads, lds, stream, a);
    });
}

}  // namespace

template <int ROW_BITS>
hipError_t launch_mq_i8_rows(const MqArgs &a, int nb, int grid, size_t lds, hipStream_t stream)
{
    switch (nb) {
    case 1: return launch_mq_score_i8_m<1, ROW_BITS>(a, grid, lds, stream);
    case 2: return launch_mq_score_i8_m<2, ROW_BITS>(a, grid, lds, stream);
    case 3: return launch_mq_score_i8_m<3, ROW_BITS>(a, grid, lds, stream);
    default: return hipErrorInvalidValue;
    }
}
template hipError_t launch_mq_i8_rows<SZG_ROW_BITS>(const MqArgs &, int, int, size_t, hipStream_t);

}  // namespace szg
