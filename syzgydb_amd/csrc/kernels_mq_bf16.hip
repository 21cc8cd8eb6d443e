// kernels_mq_bf16.hip -- the LDS-staged bfloat16 shared sweep (mq_device.h), one object per row width:
// -DSZG_ROW_BITS=32 | 16 | 64.
#include "mq_device.h"
#ifndef SZG_ROW_BITS
#error "build with -DSZG_ROW_BITS=32|16|64"
#endif

namespace szg {

namespace {

constexpr int kMqbThreads = 64 * SZG_MQB_WAVES;

// ---- bfloat16 shared sweep: 32-, 16- and 64-bit rows ---------------------------------------------------------------------------
//
// The sweep only has to RANK: what it keeps is re-scored in float64 and certified against the
// bound of its own arithmetic (key_eps, bf16 branch), so its products need not carry 24 bits.
// Rows and queries are rounded to bfloat16 on the fly (v_cvt_pk_bf16_f32, round to nearest
// even: 7 fraction bits, relative error <= 2^-8 each, same exponent range as float32) and multiplied by
// v_mfma_f32_16x16x32_bf16 -- 16 x the rate of the float32 MFMA, which turns the 48-query
// sweep from matrix-bound (0.64 ms at 1M x 768) into a plain stream of the rows.  By
// Cauchy-Schwarz the dot product moves by at most (2^-7 + 2^-16) |x| |q|, i.e. 0.0078 in -cos:
// a band that holds on the order of a hundred rows of a million, all of which the float32 re-score sees.
//
// A wave owns a tile of 16 rows and multiplies 32 elements of them per step with one A operand per
// query block (image [32-element step][query block][lane = k-group*16 + query][8 bf16]).  Row
// norms (of the float32 values) are VALU side work.  Any dimension: rows are walked in
// 128-byte steps and the chunks of a short last step that lie past the row are read as zeros.

#ifndef SZG_MQB_RING
#define SZG_MQB_RING 2  // 32-byte (two-load) steps per lane in flight
#endif
constexpr int kRingB = SZG_MQB_RING;
#ifndef SZG_MQB_RING_PREFIX
#define SZG_MQB_RING_PREFIX 6
#endif
constexpr int kRingBPrefix = SZG_MQB_RING_PREFIX;

// Staged form: a load instruction reads 128 contiguous bytes of each of 8 rows (8 lanes x 16 bytes per
// row) instead of 64 bytes of each of 16 -- the streaming pattern the memory system likes better
// (scripts/readbw: 6.95 vs 6.2 TB/s) -- and the wave turns the two loads of a 32-element step into
// the MFMA operand layout through its own KiB of LDS: convert, ds_write_b64 in row-major order,
// ds_read_b128 as lane (row, k-group).  The image is in natural order: lane (query, k-group g)
// holds elements 8g..8g+7 of the step.
//
// QBITS = 16: the rows are 16-bit codes v, decoded on the fly to n = 2v - 65535 (exact in float32) and rounded to
// bfloat16 like float rows.  A 128-byte step then holds 64 elements = two MFMA K-steps: the wave stages and
// multiplies the lower and the upper four chunks one after the other through the same KiB.  A chunk read from the
// zero block (past a short last step) decodes to -65535 per element: zeros stand against it in the image, and
// those lanes stay out of the norm, and so do the padding codes inside the row's last piece (dim % 8 != 0).
template <int NB, int METRIC, bool COLLECT, int QBITS>
__global__ __launch_bounds__(kMqbThreads) void mq_score_bf16s_kernel(const MqArgs a)
{
    constexpr int KS = QBITS == 16 ? 2 : 1;  // 32-element MFMA K-steps per 128-byte step of a row (64-bit rows: half a one)
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int SS = (a.r16 + 7) / 8;             // 128-byte steps per row, the last one possibly short
    const int last_valid = a.r16 - 8 * (SS - 1);  // 16-byte chunks of the last step that belong to the row (1..8)
    const bool partial = last_valid < 8;
    const int n16 = (QBITS == 64 ? (SS + 1) / 2 : SS * KS) * NB * 64;  // a KiB per K-step and query block
    const int pad16 = QBITS == 16 ? a.r16 * 8 - a.dim : 0;  // 16-bit rows: padding codes in the row's last 16-byte piece
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
    uint8_t *stage;
    {
        uint8_t *base = smem + (size_t)n16 * 16 + 2 * kMqMaxQueries * sizeof(float);
        hb.cand = reinterpret_cast<uint64_t *>(base) + (size_t)wave * kHitCap;
        hb.query = base + (size_t)nwaves * kHitCap * 8 + (size_t)wave * kHitCap;
        hb.n = 0;
        stage = base + (size_t)nwaves * kHitCap * 9 + (size_t)wave * 1024;  // (kHitCap * 9 * nwaves is a multiple of 16)
    }

    const int trow = lane & 15, c = lane >> 4;  // MFMA role: row of the tile, k-group
    const int r8 = lane >> 3, ch = lane & 7;    // load role: rows r8 and 8 + r8, 16-byte chunk of the 128-byte step
    uint2 *w_a = reinterpret_cast<uint2 *>(stage + r8 * 64 + ch * 8);
    uint2 *w_b = reinterpret_cast<uint2 *>(stage + 512 + r8 * 64 + ch * 8);
    uint4 *w16_a = reinterpret_cast<uint4 *>(stage + r8 * 64 + (ch & 3) * 16);  // QBITS = 16: 8 bf16 per chunk, half a step at a time
    uint4 *w16_b = reinterpret_cast<uint4 *>(stage + 512 + r8 * 64 + (ch & 3) * 16);
    uint32_t *w64_a = reinterpret_cast<uint32_t *>(stage + r8 * 64 + ch * 4);  // QBITS = 64: 2 bf16 per chunk, 16 elements per step
    uint32_t *w64_b = reinterpret_cast<uint32_t *>(stage + 512 + r8 * 64 + ch * 4);
    const v4i32b *r_op = reinterpret_cast<const v4i32b *>(stage + trow * 64 + c * 16);

    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
    const uint64_t tile_stride = (uint64_t)gridDim.x * nwaves;
    const uint64_t tile_first = (uint64_t)blockIdx.x * nwaves + wave;
    const uint64_t n_it = tile_first < n_tiles ? (n_tiles - tile_first + tile_stride - 1) / tile_stride : 0;
    const uint64_t NP = n_it * (uint64_t)SS;

    uint64_t itile = tile_first;
    int is = 0;
    uint64_t ctile = tile_first;
    int cs = 0;

    // the threshold pass (no COLLECT) sweeps a few tiles per wave on a few CUs: latency-bound, deeper ring
    constexpr int R = COLLECT ? kRingB : kRingBPrefix;
    u32x4 ring_a[R], ring_b[R];
    f32x4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    float nrm_a = 0.f, nrm_b = 0.f;
    uint32_t nz_a = 0, nz_b = 0;
    uint32_t nzl_a = 0, nzl_b = 0;  // 64-bit rows: the low words (whose bit 31 is data, not a sign)
    v4i32b qn[NB];

    const uint8_t *iptr_a, *iptr_b;
    auto set_rows = [&](uint64_t tile) {
        const uint64_t last = (uint64_t)a.n_rows - 1;  // past the end: a valid row, discarded
        iptr_a = a.rows + (size_t)min(tile * 16 + r8, last) * a.pitch + (size_t)ch * 16;
        iptr_b = a.rows + (size_t)min(tile * 16 + 8 + r8, last) * a.pitch + (size_t)ch * 16;
    };
    set_rows(tile_first);
    // a short step at the end of a row whose pitch is not a multiple of 128 bytes (any dimension that is not a
    // multiple of 32): the chunks past the row belong to the next row -- those lanes read the shard's zero block
    // instead (zeros for the products, the norm and the zero-row test alike; the padding inside the row's last
    // 16-byte piece is stored as zeros)
    const bool past = ch >= last_valid;

#define MQS_ISSUE(u)                                                                     \
    {                                                                                    \
        const bool z_ = partial && is == SS - 1 && past;                                 \
        ring_a[u] = load_stream<true>(z_ ? a.zero16 : iptr_a); /* whole 128-byte lines, used once: non-temporal */ \
        ring_b[u] = load_stream<true>(z_ ? a.zero16 : iptr_b);                           \
        if (++is == SS) {                                                                \
            is = 0;                                                                      \
            itile += tile_stride;                                                        \
            set_rows(itile);                                                             \
        } else {                                                                         \
            iptr_a += 128;                                                               \
            iptr_b += 128;                                                               \
        }                                                                                \
    }

#define MQS_CONSUME(u)                                                                   \
    {                                                                                    \
        const u32x4 va_ = ring_a[u], vb_ = ring_b[u];                                    \
        if constexpr (QBITS == 32) {                                                     \
            const float xa_[4] = {__uint_as_float(va_.x), __uint_as_float(va_.y), __uint_as_float(va_.z),   \
                                  __uint_as_float(va_.w)};                               \
            const float xb_[4] = {__uint_as_float(vb_.x), __uint_as_float(vb_.y), __uint_as_float(vb_.z),   \
                                  __uint_as_float(vb_.w)};                               \
            _Pragma("unroll") for (int i = 0; i < 4; i++) nrm_a = fmaf(xa_[i], xa_[i], nrm_a);   \
            _Pragma("unroll") for (int i = 0; i < 4; i++) nrm_b = fmaf(xb_[i], xb_[i], nrm_b);   \
            nz_a |= va_.x | va_.y;                                                       \
            nz_a |= va_.z | va_.w;                                                       \
            nz_b |= vb_.x | vb_.y;                                                       \
            nz_b |= vb_.z | vb_.w;                                                       \
            const bf16x2 t0_ = __builtin_convertvector(f32x2{xa_[0], xa_[1]}, bf16x2);   \
            const bf16x2 t1_ = __builtin_convertvector(f32x2{xa_[2], xa_[3]}, bf16x2);   \
            const bf16x2 t2_ = __builtin_convertvector(f32x2{xb_[0], xb_[1]}, bf16x2);   \
            const bf16x2 t3_ = __builtin_convertvector(f32x2{xb_[2], xb_[3]}, bf16x2);   \
            *w_a = make_uint2(__builtin_bit_cast(uint32_t, t0_), __builtin_bit_cast(uint32_t, t1_)); \
            *w_b = make_uint2(__builtin_bit_cast(uint32_t, t2_), __builtin_bit_cast(uint32_t, t3_)); \
            __builtin_amdgcn_wave_barrier();                                             \
            const v4i32b bop_ = *r_op;                                                   \
            __builtin_amdgcn_wave_barrier();                                             \
            const int qnext_ = lane + (cs + 1 == SS ? 0 : cs + 1) * (NB * 64);           \
            _Pragma("unroll") for (int b = 0; b < NB; b++)                               \
            {                                                                            \
                const v4i32b qc_ = qn[b];                                                \
                qn[b] = qimg[qnext_ + b * 64];                                           \
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, qc_),          \
                                                                 __builtin_bit_cast(bf16x8, bop_), acc[b], 0, 0, 0); \
            }                                                                            \
        } else if constexpr (QBITS == 64) {                                              \
            /* two float64 elements per 16-byte chunk: narrowed to float32 (v_cvt_f32_f64; beyond the float32 range */ \
            /* -> inf or 0, and the row is forced into the candidates by its norm, as for float32 rows), the norm and */ \
            /* the bfloat16 operand are made of the float32 values.  A 128-byte step is HALF a K-step: the wave */ \
            /* stages two steps side by side in its KiB and multiplies after the second (or after a last odd one, */ \
            /* whose missing half is zeroed). */                                         \
            const float xa0_ = (float)__hiloint2double((int)va_.y, (int)va_.x);          \
            const float xa1_ = (float)__hiloint2double((int)va_.w, (int)va_.z);          \
            const float xb0_ = (float)__hiloint2double((int)vb_.y, (int)vb_.x);          \
            const float xb1_ = (float)__hiloint2double((int)vb_.w, (int)vb_.z);          \
            nrm_a = fmaf(xa0_, xa0_, nrm_a);                                             \
            nrm_a = fmaf(xa1_, xa1_, nrm_a);                                             \
            nrm_b = fmaf(xb0_, xb0_, nrm_b);                                             \
            nrm_b = fmaf(xb1_, xb1_, nrm_b);                                             \
            nz_a |= va_.y | va_.w;                                                       \
            nzl_a |= va_.x | va_.z;                                                      \
            nz_b |= vb_.y | vb_.w;                                                       \
            nzl_b |= vb_.x | vb_.z;                                                      \
            const int half_ = cs & 1;                                                    \
            const bool last_ = cs == SS - 1;                                             \
            w64_a[half_ * 8] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{xa0_, xa1_}, bf16x2)); \
            w64_b[half_ * 8] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{xb0_, xb1_}, bf16x2)); \
            if (last_ && half_ == 0) { /* (wave-uniform) an odd number of steps: no second half */ \
                w64_a[8] = 0u;                                                           \
                w64_b[8] = 0u;                                                           \
            }                                                                            \
            if (last_ || half_ == 1) {                                                   \
                __builtin_amdgcn_wave_barrier();                                         \
                const v4i32b bop_ = *r_op;                                               \
                __builtin_amdgcn_wave_barrier();                                         \
                const int qnext_ = lane + (last_ ? 0 : (cs >> 1) + 1) * (NB * 64);       \
                _Pragma("unroll") for (int b = 0; b < NB; b++)                           \
                {                                                                        \
                    const v4i32b qc_ = qn[b];                                            \
                    qn[b] = qimg[qnext_ + b * 64];                                       \
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, qc_),      \
                                                                     __builtin_bit_cast(bf16x8, bop_), acc[b], 0, 0, 0); \
                }                                                                        \
            }                                                                            \
        } else {                                                                         \
            const uint32_t wa_[4] = {va_.x, va_.y, va_.z, va_.w}, wb_[4] = {vb_.x, vb_.y, vb_.z, vb_.w};    \
            const bool out_ = partial && cs == SS - 1 && past; /* read from the zero block: not part of the row */ \
            uint32_t pa_[4], pb_[4];                                                     \
            float xa_[8], xb_[8];                                                        \
            _Pragma("unroll") for (int i = 0; i < 4; i++)                                \
            {                                                                            \
                xa_[2 * i] = fmaf((float)(wa_[i] & 0xFFFFu), 2.0f, -65535.0f);           \
                xa_[2 * i + 1] = fmaf((float)(wa_[i] >> 16), 2.0f, -65535.0f);           \
                xb_[2 * i] = fmaf((float)(wb_[i] & 0xFFFFu), 2.0f, -65535.0f);           \
                xb_[2 * i + 1] = fmaf((float)(wb_[i] >> 16), 2.0f, -65535.0f);           \
                pa_[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{xa_[2 * i], xa_[2 * i + 1]}, bf16x2)); \
                pb_[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{xb_[2 * i], xb_[2 * i + 1]}, bf16x2)); \
            }                                                                            \
            float sa_ = 0.f, sb_ = 0.f;                                                  \
            if ((partial || pad16) && cs == SS - 1) { /* (wave-uniform) the row's last step: zero-block lanes and the */ \
                /* padding codes of the last piece decode to -65535 -- zeros stand against them in the image, and */ \
                /* they stay out of the norm (subtracting their squares afterwards would cost the small rows' norms */ \
                /* all their bits) */                                                    \
                const int nk_ = out_ ? 0 : (ch == last_valid - 1 ? 8 - pad16 : 8);       \
                _Pragma("unroll") for (int i = 0; i < 8; i++)                            \
                {                                                                        \
                    sa_ = i < nk_ ? fmaf(xa_[i], xa_[i], sa_) : sa_;                     \
                    sb_ = i < nk_ ? fmaf(xb_[i], xb_[i], sb_) : sb_;                     \
                }                                                                        \
            } else {                                                                     \
                _Pragma("unroll") for (int i = 0; i < 8; i++)                            \
                {                                                                        \
                    sa_ = fmaf(xa_[i], xa_[i], sa_);                                     \
                    sb_ = fmaf(xb_[i], xb_[i], sb_);                                     \
                }                                                                        \
            }                                                                            \
            nrm_a += sa_;                                                                \
            nrm_b += sb_;                                                                \
            nz_a = nz_b = 1u; /* a decoded code is odd: never a zero row */              \
            _Pragma("unroll") for (int h = 0; h < 2; h++)                                \
            {                                                                            \
                if ((ch >> 2) == h) {                                                    \
                    *w16_a = make_uint4(pa_[0], pa_[1], pa_[2], pa_[3]);                 \
                    *w16_b = make_uint4(pb_[0], pb_[1], pb_[2], pb_[3]);                 \
                }                                                                        \
                __builtin_amdgcn_wave_barrier();                                         \
                const v4i32b bop_ = *r_op;                                               \
                __builtin_amdgcn_wave_barrier();                                         \
                const int kn_ = cs * 2 + h + 1;                                          \
                const int qnext_ = lane + (kn_ == SS * 2 ? 0 : kn_) * (NB * 64);         \
                _Pragma("unroll") for (int b = 0; b < NB; b++)                           \
                {                                                                        \
                    const v4i32b qc_ = qn[b];                                            \
                    qn[b] = qimg[qnext_ + b * 64];                                       \
                    acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, qc_),      \
                                                                     __builtin_bit_cast(bf16x8, bop_), acc[b], 0, 0, 0); \
                }                                                                        \
            }                                                                            \
        }                                                                                \
        if (++cs == SS) {                                                                \
            finish_tile(ctile);                                                          \
            cs = 0;                                                                      \
            ctile += tile_stride;                                                        \
        }                                                                                \
    }

    auto finish_tile = [&](uint64_t tile) {
        // row norms: over the 8 chunk lanes of each row, then to the lanes of the MFMA result (column = row)
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            nrm_a += __shfl_xor(nrm_a, o);
            nrm_b += __shfl_xor(nrm_b, o);
            nz_a |= __shfl_xor(nz_a, o);
            nz_b |= __shfl_xor(nz_b, o);
            if constexpr (QBITS == 64) {
                nzl_a |= __shfl_xor(nzl_a, o);
                nzl_b |= __shfl_xor(nzl_b, o);
            }
        }
        const int src = (trow & 7) * 8;
        const float na = __shfl(nrm_a, src), nb2 = __shfl(nrm_b, src);
        const uint32_t za = __shfl(nz_a, src), zb = __shfl(nz_b, src);
        const float nrm = trow < 8 ? na : nb2;
        uint32_t nz = (trow < 8 ? za : zb) & 0x7FFFFFFFu;
        if constexpr (QBITS == 64) {
            const uint32_t zla = __shfl(nzl_a, src), zlb = __shfl(nzl_b, src);
            nz |= trow < 8 ? zla : zlb;
        }
        const uint64_t row = tile * 16 + trow;
        const float inv = __frsqrt_rn(nrm);
        // What depends on the ROW alone is settled once per lane, not once per (row, query) pair: a zero row (distance
        // 1.0, collection.go:828-830) or a norm beyond float32 (forced in: see RowAcc::finish) has one fixed key for
        // every query.  The two clamps (NaN and +inf -> the worst finite key) are ONE v_min_f32 -- minnum returns the
        // other operand for a NaN -- and the hit bits are combined without short-circuits: round 3's form compiled to
        // three exec-masked branches and ~12 vector instructions per pair, 40 % of the sweep's vector instructions on
        // 16-bit rows (PMC: 57 per K-step against the 30 of its step loop), on kernels whose SIMDs issue all the time.
        const bool use_fixed = METRIC == kCosine && (nrm == 0.f || !(nrm <= 3.0e38f));
        const float fixed = (nrm == 0.f && !nz) ? 1.0f : -2.0f;
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
                    float key;
                    if (METRIC == kCosine) {
                        key = -acc[b][r] * inv;
                        key = use_fixed ? fixed : key;
                    } else {
                        key = fmaf(-2.0f, acc[b][r], nrm + qnv[r]);
                    }
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
        if (!COLLECT) __builtin_amdgcn_s_waitcnt(0x0F70);  // drain the key stores: gfx9 counts loads and stores in ONE vmcnt, a pending store would turn every ring wait into vmcnt(0)
#pragma unroll
        for (int b = 0; b < NB; b++) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
        nrm_a = nrm_b = 0.f;
        nz_a = nz_b = 0;
        nzl_a = nzl_b = 0;
    };

    {
        uint64_t issued = R, consumed = 0;
#pragma unroll
        for (int u = 0; u < R; u++) {
            MQS_ISSUE(u)
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // the query image is complete (the rows do not depend on it)
#pragma unroll
        for (int b = 0; b < NB; b++) qn[b] = qimg[lane + b * 64];
        while (consumed + 2 * R <= NP) {
#pragma unroll
            for (int u = 0; u < R; u++) {
                MQS_CONSUME(u)
                MQS_ISSUE(u)
                __builtin_amdgcn_sched_barrier(0);
            }
            consumed += R;
            issued += R;
        }
        while (consumed < NP) {
#pragma unroll
            for (int u = 0; u < R; u++) {
                if (consumed < NP) {
                    MQS_CONSUME(u)
                    consumed++;
                    if (issued < NP) {
                        MQS_ISSUE(u)
                        issued++;
                    }
                }
            }
        }
    }
#undef MQS_ISSUE
#undef MQS_CONSUME
    if (COLLECT) hit_flush(a, hb, lane);
}

}  // namespace

template <int ROW_BITS>
hipError_t launch_mq_bf16s_rows(const MqArgs &a, int nb, int grid, size_t lds, hipStream_t stream)
{
    if (a.tiled || a.n_rows == 0 || !a.zero16) return hipErrorInvalidValue;
    return with_query_blocks6(nb, [&](auto nb_c) {
        return with_metric_collect(a, [&](auto metric, auto collect) {
            return launch_lds(&mq_score_bf16s_kernel<decltype(nb_c)::value, metric, collect, ROW_BITS>, grid, kMqbThreads, lds, stream, a);
        });
    });
}
template hipError_t launch_mq_bf16s_rows<SZG_ROW_BITS>(const MqArgs &, int, int, size_t, hipStream_t);

}  // namespace szg
