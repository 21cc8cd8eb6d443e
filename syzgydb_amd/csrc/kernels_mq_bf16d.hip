// kernels_mq_bf16d.hip -- the direct bfloat16 shared sweeps (mq_device.h): the codes arrive in the MFMA operand layout.
// mq_score_bf16d_kernel for 16-bit rows, mq_score_bf16d8_kernel for 8-bit rows; one object holds both (neither is the
// build's long pole).
#include "mq_device.h"

namespace szg {

namespace {

// ---- 16-bit rows without the LDS stage: the codes arrive in the MFMA operand layout ---------------------------------
//
// A 16-byte chunk of a 16-bit row is eight codes -- exactly one lane's share (eight bfloat16) of the B operand of
// v_mfma_f32_16x16x32_bf16 (lane = k-group * 16 + row).  So the lanes load the chunks themselves, decode
// (n = 2v - 65535), round to bfloat16 in registers and multiply: no ds_write / ds_read / wait between the load and the
// matrix instruction, where the staged kernel above -- 56 VALU of decode, then write -> read -> wait TWICE per step --
// held 16-bit rows at 4.2-5.0 TB/s.
//
// WHICH chunk a lane loads is the round-4 lesson.  Loading the operand layout directly (lane = row & 15, chunk =
// lane >> 4: 64 bytes of each of 16 rows per instruction, the line's other half one instruction later) streams at
// 5.1-5.6 TB/s with NOTHING but the loads in the kernel (scripts/readbw/rowpat, mode 0), and the sweep sat at 5.3-5.5
// whatever was removed from its arithmetic (resident norms: 8 of 30 VALU per step gone, same time).  128 bytes of each
// of 8 rows per instruction (lane = row & 7, chunk = lane >> 3) streams at 7.0-7.2 (mode 2).  So a DOUBLE step loads X
// = rows 0-7 and Y = rows 8-15 of the tile, 128 bytes of each, and one DPP exchange per dword (row_ror:8 -- lane L
// takes from lane L ^ 8 -- under a bank mask) turns the pair into two operands in MFMA layout:
//     E[L] = L & 8 ? Y[L ^ 8] : X[L]      row L & 15, chunk 2 * (L >> 4)        (the even chunks of the 128 bytes)
//     O[L] = L & 8 ? Y[L] : X[L ^ 8]      row L & 15, chunk 2 * (L >> 4) + 1    (the odd chunks)
// The k order inside a matrix instruction is free as long as both operands agree, so the A operands are the SAME image
// read at permuted addresses: k-group g of E pairs with chunk 2g = K-step 2t + (g >> 1), k-group 2 (g & 1) of the
// image; O with the k-group after it.
#ifndef SZG_MQD_RING
#define SZG_MQD_RING 2  // PAIRS of 16-byte loads per lane in flight (2 x 2 KiB per wave)
#endif
#ifndef SZG_MQD_WAVES
#define SZG_MQD_WAVES 12  // waves per block (one block per CU): no staging KiB per wave, <= 168 registers: three per SIMD
#endif
constexpr int kMqdThreads = 64 * SZG_MQD_WAVES;
template <int NB, int METRIC, bool COLLECT>
__global__ __launch_bounds__(kMqdThreads) void mq_score_bf16d_kernel(const MqArgs a)
{
    constexpr int D = COLLECT ? SZG_MQD_RING : 4;  // (the threshold pass: a few tiles per wave, latency-bound)
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int DT = (a.r16 + 7) / 8;        // double steps (64 elements, 128 bytes of a row) per row, the last possibly short
    const bool partial = (a.r16 & 7) != 0;
    const int n16 = 2 * DT * NB * 64;      // the image holds an even number of K-steps (mq_bf16_image_bytes), zero-filled
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.queries);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        stage_image(dst, src, n16, tid, blockDim.x);
        // table: [0, 96) thresholds, [96, 192) |q|^2
        if (COLLECT && tid < kMqMaxQueries)
            reinterpret_cast<float *>(smem + (size_t)n16 * 16)[tid] = tid < a.n_queries ? a.thr[tid] : -3.0e38f;
        if (METRIC != kCosine && tid >= 128 && tid < 128 + kMqMaxQueries)
            reinterpret_cast<float *>(smem + (size_t)n16 * 16)[tid - 32] = a.qnorm2[tid - 128];
    }
    const v4i32b *qimg = reinterpret_cast<const v4i32b *>(smem);
    const float *thr_lds = reinterpret_cast<const float *>(smem + (size_t)n16 * 16);
    HitBuf hb;
    {
        uint8_t *base = smem + (size_t)n16 * 16 + 2 * kMqMaxQueries * sizeof(float);
        hb.cand = reinterpret_cast<uint64_t *>(base) + (size_t)wave * kHitCap;
        hb.query = base + (size_t)nwaves * kHitCap * 8 + (size_t)wave * kHitCap;
        hb.n = 0;
    }
    const int row8 = lane & 7, chunk = lane >> 3;  // as loaded: 128 bytes of each of 8 rows
    const int trow = lane & 15, c = lane >> 4;     // as multiplied (after the exchange), and the result's layout
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
    const uint64_t tile_stride = (uint64_t)gridDim.x * nwaves;
    const uint64_t tile_first = (uint64_t)blockIdx.x * nwaves + wave;
    const uint64_t n_it = tile_first < n_tiles ? (n_tiles - tile_first + tile_stride - 1) / tile_stride : 0;
    const uint64_t NP = n_it * (uint64_t)DT;
    const bool past = (DT - 1) * 8 + chunk >= a.r16;  // this lane's chunk of a short last double step lies beyond the row
    // the A operand of (double step t, half h, block b): qimg[t * 2 * NB * 64 + h * 16 + b * 64 + lane_e]
    const int lane_e = trow + 32 * (c & 1) + (c >> 1) * (NB * 64);

    uint64_t itile = tile_first, ctile = tile_first;
    int is = 0, cs = 0;
    u32x4 ring[2 * D];
    f32x4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float nrm = 0.f;
    v4i32b qn[NB];
    auto row_ptr = [&](uint64_t tile, int half) -> const uint8_t * {
        const uint64_t r = min(tile * 16 + half * 8 + row8, (uint64_t)a.n_rows - 1);  // past the end: a valid row, discarded
        return a.rows + (size_t)r * a.pitch + (size_t)chunk * 16;
    };
    const uint8_t *ipx = row_ptr(tile_first, 0), *ipy = row_ptr(tile_first, 1);

#define MQD_ISSUE(u)                                                                     \
    {                                                                                    \
        const bool z_ = partial && is == DT - 1 && past;                                 \
        ring[2 * (u)] = load_stream<true>(z_ ? a.zero16 : ipx); /* (whole lines, used once: past the caches) */ \
        ring[2 * (u) + 1] = load_stream<true>(z_ ? a.zero16 : ipy);                      \
        if (++is == DT) {                                                                \
            is = 0;                                                                      \
            itile += tile_stride;                                                        \
            ipx = row_ptr(itile, 0);                                                     \
            ipy = row_ptr(itile, 1);                                                     \
        } else {                                                                         \
            ipx += 128;                                                                  \
            ipy += 128;                                                                  \
        }                                                                                \
    }

    // one operand (half h_ of the double step): decode, norm, NB matrix instructions, the next operands' reads
    // (Tried on the 64-byte form: the decode in packed float32 pairs -- v_pk_fma_f32, 20 instead of 28 vector
    // instructions per K-step -- 3-5 % SLOWER on the same box.  profiles/r04_bf16_16bit_experiments.txt.)
#define MQD_HALF(raw_, h_)                                                               \
    {                                                                                    \
        const uint32_t w_[4] = {raw_.x, raw_.y, raw_.z, raw_.w};                         \
        float x_[8];                                                                     \
        v4i32b bop_;                                                                     \
        _Pragma("unroll") for (int i = 0; i < 4; i++)                                    \
        {                                                                                \
            x_[2 * i] = fmaf((float)(w_[i] & 0xFFFFu), 2.0f, -65535.0f);                 \
            x_[2 * i + 1] = fmaf((float)(w_[i] >> 16), 2.0f, -65535.0f);                 \
            bop_[i] = (int)__builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{x_[2 * i], x_[2 * i + 1]}, bf16x2)); \
        }                                                                                \
        /* resident norms (MqArgs::row_norm): this tile's 16 arrive while its steps run.  (Summing them here -- eight */ \
        /* more vector instructions per operand -- measured 3.5 % slower, and the threshold pass then spilled: */        \
        /* without the array the staged kernel runs, which sums its own.) */                                              \
        if ((h_) == 0 && cs == 0) nrm = a.row_norm[min(ctile * 16 + trow, (uint64_t)a.n_rows - 1)]; \
        const int qnext_ = lane_e + ((h_) == 0 ? cs * (2 * NB * 64) + 16 : (cs + 1 == DT ? 0 : cs + 1) * (2 * NB * 64)); \
        _Pragma("unroll") for (int b = 0; b < NB; b++)                                   \
        {                                                                                \
            const v4i32b qc_ = qn[b];                                                    \
            qn[b] = qimg[qnext_ + b * 64];                                               \
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, qc_),              \
                                                             __builtin_bit_cast(bf16x8, bop_), acc[b], 0, 0, 0); \
        }                                                                                \
    }

#define MQD_CONSUME(u)                                                                   \
    {                                                                                    \
        const u32x4 vx_ = ring[2 * (u)], vy_ = ring[2 * (u) + 1];                         \
        u32x4 ve_, vo_;                                                                  \
        _Pragma("unroll") for (int i = 0; i < 4; i++)                                    \
        {   /* row_ror:8 = 0x128; bank mask 0x3: lanes 0-7 of every 16 are written, 0xC: lanes 8-15 */ \
            vo_[i] = (uint32_t)__builtin_amdgcn_update_dpp((int)vy_[i], (int)vx_[i], 0x128, 0xF, 0x3, false); \
            ve_[i] = (uint32_t)__builtin_amdgcn_update_dpp((int)vx_[i], (int)vy_[i], 0x128, 0xF, 0xC, false); \
        }                                                                                \
        MQD_HALF(ve_, 0)                                                                 \
        MQD_HALF(vo_, 1)                                                                 \
        if (++cs == DT) {                                                                \
            finish_tile(ctile);                                                          \
            cs = 0;                                                                      \
            ctile += tile_stride;                                                        \
        }                                                                                \
    }

    auto finish_tile = [&](uint64_t tile) {
        const uint64_t row = tile * 16 + trow;  // (the MFMA result's column = the row, as the operand's)
        const float inv = __frsqrt_rn(nrm);
        // (a decoded code is odd: the norm of a 16-bit row is neither 0 nor beyond float32 -- no fixed keys here; the
        // clamps are one v_min_f32 and the hit bits have no short-circuits: see mq_score_bf16s_kernel's finish)
        if (COLLECT || row < a.n_rows) {
            float keys[NB][4];
            uint32_t hm = 0;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const float4 th = COLLECT ? *reinterpret_cast<const float4 *>(thr_lds + b * 16 + c * 4)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
                const float thv[4] = {th.x, th.y, th.z, th.w};
                const float4 qn4 = METRIC == kCosine ? make_float4(0.f, 0.f, 0.f, 0.f)
                                                     : *reinterpret_cast<const float4 *>(thr_lds + kMqMaxQueries + b * 16 + c * 4);
                const float qnv[4] = {qn4.x, qn4.y, qn4.z, qn4.w};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float key = METRIC == kCosine ? -acc[b][r] * inv : fmaf(-2.0f, acc[b][r], nrm + qnv[r]);
                    key = fminf(key, 3.0e38f);  // NaN, +inf -> 3e38
                    keys[b][r] = key;
                    if (COLLECT)  // (unused query slots carry a threshold of -3e38: never a hit)
                        hm |= (uint32_t)(key <= thv[r]) << (b * 4 + r);
                    else if (b * 16 + c * 4 + r < a.n_queries)
                        a.keys[(size_t)(b * 16 + c * 4 + r) * a.key_stride + row] = key;
                }
            }
            if (COLLECT) {
                hm = row < a.n_rows ? hm : 0u;
                offer_tile_hits<NB>(a, hb, lane, c, hm, keys, row);
            }
        }
        if (!COLLECT) __builtin_amdgcn_s_waitcnt(0x0F70);  // drain the key stores (one vmcnt for loads and stores)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        nrm = 0.f;
    };

    {
        uint64_t issued = D, consumed = 0;
#pragma unroll
        for (int u = 0; u < D; u++) {
            MQD_ISSUE(u)
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // the query image is complete (the rows do not depend on it)
#pragma unroll
        for (int b = 0; b < NB; b++) qn[b] = qimg[lane_e + b * 64];
        while (consumed + 2 * D <= NP) {
#pragma unroll
            for (int u = 0; u < D; u++) {
                MQD_CONSUME(u)
                MQD_ISSUE(u)
                __builtin_amdgcn_sched_barrier(0);
            }
            consumed += D;
            issued += D;
        }
        while (consumed < NP) {
#pragma unroll
            for (int u = 0; u < D; u++) {
                if (consumed < NP) {
                    MQD_CONSUME(u)
                    consumed++;
                    if (issued < NP) {
                        MQD_ISSUE(u)
                        issued++;
                    }
                }
            }
        }
    }
#undef MQD_ISSUE
#undef MQD_HALF
#undef MQD_CONSUME
    if (COLLECT) hit_flush(a, hb, lane);
}

// ---- 8-bit rows through the bfloat16 matrix instruction: 96 queries per pass -----------------------------------------
//
// An 8-bit code is EXACT in bfloat16: v - 128 = -128..127 has eight significant bits.  So the rows need no digit planes and no
// integer arithmetic to be multiplied exactly -- only the QUERY is rounded (to bfloat16, as for float rows), which the
// bfloat16 path's second stage (float32 re-score of the band, §4.2a) and bounds already cover.  What that buys: the
// image of 96 queries is 6 KiB per 32 elements instead of the int8 sweep's 2 planes x 3 KiB per 48 queries, i.e. ONE
// pass of the rows per 96 queries where the int8 sweep makes two, for the same number of matrix instructions.
// The row operand: lane (row = lane & 15, c = lane >> 4) loads its 16 bytes of the 64-byte step of a TILED row (one
// contiguous KiB per wave instruction) = 16 codes = its share of TWO B operands (codes 0-7 and 8-15); the A operands
// are the natural image at the permuted addresses of mq_score_bf16d_kernel.  With v' = v - 128, n = 2v' + 1:
// sum g n = 2 sum g v' + sum g; sum g (over the ROUNDED image) is a per-query constant staged beside the thresholds
// (MqArgs::qsum).
// Norms: the resident array (launch_row_norms, the int8 formula = sum n^2 of the real elements).
#ifndef SZG_MQD8_WAVES
#define SZG_MQD8_WAVES 12
#endif
#ifndef SZG_MQD8_RING
#define SZG_MQD8_RING 4
#endif
constexpr int kMqd8Threads = 64 * SZG_MQD8_WAVES;
template <int NB, int METRIC, bool COLLECT>
__global__ __launch_bounds__(kMqd8Threads) void mq_score_bf16d8_kernel(const MqArgs a)
{
    constexpr int D = COLLECT ? SZG_MQD8_RING : 6;
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int DT = (int)a.steps;        // 64-byte steps per (tiled) row = double K-steps
    const int n16 = 2 * DT * NB * 64;   // a KiB per 32-element K-step and query block
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.queries);
        uint4 *dst = reinterpret_cast<uint4 *>(smem);
        stage_image(dst, src, n16, tid, blockDim.x);
        // table: [0, 96) thresholds, [96, 192) |g|^2, [192, 288) sum g
        float *tab = reinterpret_cast<float *>(smem + (size_t)n16 * 16);
        if (COLLECT && tid < kMqMaxQueries) tab[tid] = tid < a.n_queries ? a.thr[tid] : -3.0e38f;
        if (tid >= 128 && tid < 128 + kMqMaxQueries) tab[tid - 32] = a.qnorm2[tid - 128];
        if (tid >= 256 && tid < 256 + kMqMaxQueries) tab[tid - 64] = a.qsum[tid - 256];
    }
    const v4i32b *qimg = reinterpret_cast<const v4i32b *>(smem);
    const float *thr_lds = reinterpret_cast<const float *>(smem + (size_t)n16 * 16);
    HitBuf hb;
    {
        uint8_t *base = smem + (size_t)n16 * 16 + 3 * kMqMaxQueries * sizeof(float);
        hb.cand = reinterpret_cast<uint64_t *>(base) + (size_t)wave * kHitCap;
        hb.query = base + (size_t)nwaves * kHitCap * 8 + (size_t)wave * kHitCap;
        hb.n = 0;
    }
    const int trow = lane & 15, c = lane >> 4;
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
    const uint64_t tile_stride = (uint64_t)gridDim.x * nwaves;
    const uint64_t tile_first = (uint64_t)blockIdx.x * nwaves + wave;
    const uint64_t n_it = tile_first < n_tiles ? (n_tiles - tile_first + tile_stride - 1) / tile_stride : 0;
    const uint64_t NP = n_it * (uint64_t)DT;
    const int lane_e = trow + 32 * (c & 1) + (c >> 1) * (NB * 64);  // (see mq_score_bf16d_kernel)
    const size_t tile_bytes = (size_t)DT * 1024;
    const size_t lane_off = (size_t)trow * 64 + (size_t)c * 16;

    uint64_t itile = tile_first, ctile = tile_first;
    int is = 0, cs = 0;
    u32x4 ring[D];
    f32x4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float nrm = 0.f;
    v4i32b qn[NB];
    const uint8_t *iptr = a.rows + (size_t)min(tile_first, n_tiles - 1) * tile_bytes + lane_off;

#define MQD8_ISSUE(u)                                                                     \
    {                                                                                    \
        ring[u] = load_stream<true>(iptr);                                               \
        if (++is == DT) {                                                                \
            is = 0;                                                                      \
            itile += tile_stride;                                                        \
            iptr = a.rows + (size_t)min(itile, n_tiles - 1) * tile_bytes + lane_off; /* (past the end: the last tile, discarded) */ \
        } else {                                                                         \
            iptr += 1024;                                                                \
        }                                                                                \
    }

    // one operand: two dwords = eight codes -> v - 128 as float -> bfloat16 pairs (exact), NB matrix instructions
// The codes are multiplied as v' = v - 128 (one xor per dword, then a sign-extending byte convert), NOT as v: with
// n = 2v' + 1 the accumulator holds sum g v' -- small when the row is (a zero vector is all codes 128) -- whereas
// sum g v - 127.5 sum g would cancel two numbers 128 x larger than their difference inside the matrix core's float32
// sums, an error key_eps' bfloat16 branch has no term for.  (The unsigned form measured 2 % faster.)
#define MQD8_PK(a_, b_) (int)__builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{(float)(a_), (float)(b_)}, bf16x2))
#define MQD8_DECODE(w0_, w1_)                                                             \
        {                                                                                \
            const uint32_t s0_ = (w0_) ^ 0x80808080u, s1_ = (w1_) ^ 0x80808080u;         \
            bop_[0] = MQD8_PK((int8_t)s0_, (int8_t)(s0_ >> 8));                           \
            bop_[1] = MQD8_PK((int8_t)(s0_ >> 16), (int8_t)(s0_ >> 24));                  \
            bop_[2] = MQD8_PK((int8_t)s1_, (int8_t)(s1_ >> 8));                           \
            bop_[3] = MQD8_PK((int8_t)(s1_ >> 16), (int8_t)(s1_ >> 24));                  \
        }
#define MQD8_HALF(w0_, w1_, h_)                                                           \
    {                                                                                    \
        v4i32b bop_;                                                                     \
        MQD8_DECODE(w0_, w1_)                                                             \
        if ((h_) == 0 && cs == 0) nrm = a.row_norm[min(ctile * 16 + trow, (uint64_t)a.n_rows - 1)]; \
        const int qnext_ = lane_e + ((h_) == 0 ? cs * (2 * NB * 64) + 16 : (cs + 1 == DT ? 0 : cs + 1) * (2 * NB * 64)); \
        _Pragma("unroll") for (int b = 0; b < NB; b++)                                   \
        {                                                                                \
            const v4i32b qc_ = qn[b];                                                    \
            qn[b] = qimg[qnext_ + b * 64];                                               \
            acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, qc_),              \
                                                             __builtin_bit_cast(bf16x8, bop_), acc[b], 0, 0, 0); \
        }                                                                                \
    }

#define MQD8_CONSUME(u)                                                                   \
    {                                                                                    \
        const u32x4 v_ = ring[u];                                                        \
        MQD8_HALF(v_.x, v_.y, 0)                                                          \
        MQD8_HALF(v_.z, v_.w, 1)                                                          \
        if (++cs == DT) {                                                                \
            finish_tile(ctile);                                                          \
            cs = 0;                                                                      \
            ctile += tile_stride;                                                        \
        }                                                                                \
    }

    auto finish_tile = [&](uint64_t tile) {
        const uint64_t row = tile * 16 + trow;
        const float inv = __frsqrt_rn(nrm);  // (every n is odd: the norm of an 8-bit row is at least its dimension)
        if (COLLECT || row < a.n_rows) {
            float keys[NB][4];
            uint32_t hm = 0;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const float4 th = COLLECT ? *reinterpret_cast<const float4 *>(thr_lds + b * 16 + c * 4)
                                          : make_float4(0.f, 0.f, 0.f, 0.f);
                const float thv[4] = {th.x, th.y, th.z, th.w};
                const float4 qn4 = METRIC == kCosine ? make_float4(0.f, 0.f, 0.f, 0.f)
                                                     : *reinterpret_cast<const float4 *>(thr_lds + kMqMaxQueries + b * 16 + c * 4);
                const float qnv[4] = {qn4.x, qn4.y, qn4.z, qn4.w};
                const float4 qs4 = *reinterpret_cast<const float4 *>(thr_lds + 2 * kMqMaxQueries + b * 16 + c * 4);
                const float qsv[4] = {qs4.x, qs4.y, qs4.z, qs4.w};
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float dotn = fmaf(2.0f, acc[b][r], qsv[r]);  // sum g n = 2 sum g v' + sum g
                    float key = METRIC == kCosine ? -dotn * inv : fmaf(-2.0f, dotn, nrm + qnv[r]);
                    key = fminf(key, 3.0e38f);  // NaN, +inf -> 3e38
                    keys[b][r] = key;
                    if (COLLECT)  // (unused query slots carry a threshold of -3e38: never a hit)
                        hm |= (uint32_t)(key <= thv[r]) << (b * 4 + r);
                    else if (b * 16 + c * 4 + r < a.n_queries)
                        a.keys[(size_t)(b * 16 + c * 4 + r) * a.key_stride + row] = key;
                }
            }
            if (COLLECT) {
                hm = row < a.n_rows ? hm : 0u;
                offer_tile_hits<NB>(a, hb, lane, c, hm, keys, row);
            }
        }
        if (!COLLECT) __builtin_amdgcn_s_waitcnt(0x0F70);  // drain the key stores (one vmcnt for loads and stores)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        nrm = 0.f;
    };

    {
        uint64_t issued = D, consumed = 0;
#pragma unroll
        for (int u = 0; u < D; u++) {
            MQD8_ISSUE(u)
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // the query image is complete (the rows do not depend on it)
#pragma unroll
        for (int b = 0; b < NB; b++) qn[b] = qimg[lane_e + b * 64];
        while (consumed + 2 * D <= NP) {
#pragma unroll
            for (int u = 0; u < D; u++) {
                MQD8_CONSUME(u)
                MQD8_ISSUE(u)
                __builtin_amdgcn_sched_barrier(0);
            }
            consumed += D;
            issued += D;
        }
        while (consumed < NP) {
#pragma unroll
            for (int u = 0; u < D; u++) {
                if (consumed < NP) {
                    MQD8_CONSUME(u)
                    consumed++;
                    if (issued < NP) {
                        MQD8_ISSUE(u)
                        issued++;
                    }
                }
            }
        }
    }
#undef MQD8_ISSUE
#undef MQD8_HALF
#undef MQD8_CONSUME
    if (COLLECT) hit_flush(a, hb, lane);
}

}  // namespace

template <int ROW_BITS>
hipError_t launch_mq_bf16d_rows(const MqArgs &a, int nb, int grid, size_t lds, hipStream_t stream)
{
    if constexpr (ROW_BITS == 16) {
        if (a.tiled || a.n_rows == 0 || !a.zero16 || !a.row_norm) return hipErrorInvalidValue;
    } else {
        if (!a.tiled || a.steps == 0 || a.n_rows == 0 || !a.row_norm) return hipErrorInvalidValue;
    }
    return with_query_blocks6(nb, [&](auto nb_c) {
        return with_metric_collect(a, [&](auto metric, auto collect) {
            constexpr int NB = decltype(nb_c)::value;
            if constexpr (ROW_BITS == 16)
                return launch_lds(&mq_score_bf16d_kernel<NB, metric, collect>, grid, kMqdThreads, lds, stream, a);
            else
                return launch_lds(&mq_score_bf16d8_kernel<NB, metric, collect>, grid, kMqd8Threads, lds, stream, a);
        });
    });
}
template hipError_t launch_mq_bf16d_rows<16>(const MqArgs &, int, int, size_t, hipStream_t);
template hipError_t launch_mq_bf16d_rows<8>(const MqArgs &, int, int, size_t, hipStream_t);

}  // namespace szg
