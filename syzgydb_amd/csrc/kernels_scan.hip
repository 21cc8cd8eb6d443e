// kernels_scan.hip -- the fused brute-force scan for gfx950 (MI355X).
//
// One launch sweeps the resident corpus once and replaces the reference's HOT
// LOOP (collection.go:672-684): per row it dequantizes (collection.go:768-794,
// quantization.go:25-36), accumulates the distance terms of
// euclideanDistance / angularDistance (collection.go:812-832) and feeds a
// running selection (collection.go:598-619).
//
// The kernel is HBM-bound by construction: every lane issues 16-byte loads of
// the packed rows, lanes of one row group read contiguous bytes, the query
// lives in LDS (piece-swizzled so ds_read_b128 is conflict-free), per-row sums
// are reduced with wave shuffles and candidates go to per-wave sorted lists in
// LDS that are merged block-wide at the end.  Ranking keys are monotone
// surrogates of the reference distance (-cos or squared L2); the exact
// float64 distance is recomputed for the few survivors by kernels_exact.hip.
#include "kernels.h"
#include "device_lists.h"

#include <type_traits>

// One object per quantization and metric: -DSZG_QBITS=4/8/16/32/64 -DSZG_SCAN_METRIC=0/1 carries the scan kernels of
// that width and metric and their launcher (80 instantiations in one unit took minutes to compile); with
// -DSZG_GROUP_FORM=0..3 on top (8-bit rows), the G > 1 kernels of one form instead.  scan_plan.cpp decides which kernel
// a launch takes; the list-merge kernels and the by-width dispatcher are kernels_scan_merge.hip's.
#ifndef SZG_QBITS
#error "kernels_scan.hip needs SZG_QBITS (4, 8, 16, 32 or 64)"
#endif
#ifndef SZG_SCAN_METRIC
#error "kernels_scan.hip with SZG_QBITS needs SZG_SCAN_METRIC (0 or 1)"
#endif

namespace szg {

#ifndef SZG_GROUP_FORM
// the G > 1 kernels of 8-bit rows, one object per metric and form (see SZG_GROUP_FORM below)
static hipError_t launch_scan_g8(int metric, int form, const ScanArgs &a, const ScanVariant &v, int grid, int block, size_t lds,
                                 hipStream_t stream)
{
    static constexpr decltype(&launch_scan_g8m0f0) by_metric_form[2][4] = {
        {launch_scan_g8m0f0, launch_scan_g8m0f1, launch_scan_g8m0f2, launch_scan_g8m0f3},
        {launch_scan_g8m1f0, launch_scan_g8m1f1, launch_scan_g8m1f2, launch_scan_g8m1f3}};
    if (form < 0 || form > 3) return hipErrorInvalidValue;
    return by_metric_form[metric == kCosine ? 1 : 0][form](a, v, grid, block, lds, stream);
}
#endif

namespace {

constexpr int kWave = 64;
#ifndef SZG_MIN_BLOCKS
#define SZG_MIN_BLOCKS 3  // 256-thread blocks per CU the register budget allows: the sweeps run 2-3 per CU
                          // (scan_geometry), and 168 registers keep every variant free of spills (at 128
                          // the deep-ring and row-unrolled kernels spilled 2-59 registers)
#endif
#ifndef SZG_QPF
#define SZG_QPF 0  // integer paths: fetch the query's digit planes of the NEXT piece from LDS before this piece's dots
#endif
// G > 1 kernels hold G lists and G accumulator triples per lane: two blocks per CU (256 registers) keep them free of
// spills, and two blocks of four waves are what the sweeps over tiled 8-bit rows run per CU anyway (scan_geometry)
constexpr int kGroupMinBlocks = 2;

template <int QBITS>
struct Traits {
    using acc_t = float;
};
template <>
struct Traits<64> {
    using acc_t = double;
};

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

// streaming 16-byte load of one piece of a packed row (read once per scan).
// NT (non-temporal): the corpus is far larger than L2 + Infinity Cache and each
// byte is used once per scan -- measured 6.18 vs 5.66 TB/s on the 1M x 768 f32
// scan.  Only when a lane group reads whole 128-byte lines per load: with
// narrower groups (L < 8, 64-byte segments) the neighbouring piece needs the
// same line a moment later and nt evicts it first (4-bit 384-dim rows: 4.6 TB/s
// with nt, 5.5 plain).
template <bool NT>
__device__ __forceinline__ u32x4 load_piece(const uint8_t *p)
{
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return *reinterpret_cast<const u32x4 *>(p);
}

// value of the lane a DPP control pairs this lane with (quad_perm xor 1 / xor 2,
// row_half_mirror, row_mirror: after the four steps every lane of an aligned
// 2/4/8/16-lane group holds the group's sum)
template <int CTRL>
__device__ __forceinline__ float dpp_xchg(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_xchg(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ double dpp_xchg(double v)
{
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// ---- row accumulators ---------------------------------------------------------
// RowAcc<QBITS, METRIC> holds one lane's partial sums for the row its group is
// walking: reset(), piece() for each 16-byte piece, finish() reduces over the
// group's L lanes and returns the ranking key (valid in the group's first lane).

struct Grp {
    int L, lig;
    bool pow2;
};

// sum over the L lanes of a row group; every lane of an aligned power-of-two
// group gets the total, otherwise the group's first lane does
template <typename T>
__device__ __forceinline__ T grp_sum(T v, const Grp &g)
{
    if (g.pow2) {
        if (g.L >= 2) v += dpp_xchg<0xB1>(v);
        if (g.L >= 4) v += dpp_xchg<0x4E>(v);
        if (g.L >= 8) v += dpp_xchg<0x141>(v);
        if (g.L >= 16) v += dpp_xchg<0x140>(v);
        if (g.L >= 32) v += __shfl_xor(v, 16);
        if (g.L >= 64) v += __shfl_xor(v, 32);
    } else {
        for (int w = g.L; w > 1;) {
            const int half = (w + 1) >> 1;
            const T o = __shfl_down(v, half);
            if (g.lig + half < w) v += o;
            w = half;
        }
    }
    return v;
}

__device__ __forceinline__ uint32_t grp_or(uint32_t v, const Grp &g)
{
    for (int w = g.L; w > 1;) {
        const int half = (w + 1) >> 1;
        const uint32_t o = __shfl_down(v, half);
        if (g.lig + half < w) v |= o;
        w = half;
    }
    return v;
}

// Float rows (16/32-bit, float32 sums) and 64-bit rows (float64 sums).
// a0: dot (cosine) or sum of squared differences (euclid); a1: sum of squares of
// the row; nz: OR of the row's magnitude bits (tells a true zero row from an
// underflowed norm).  The query is pre-normalised (cosine: key = -cos) or, for
// 16-bit rows under euclid, pre-scaled by maxInt.
template <int QBITS, int METRIC>
struct RowAcc {
    using acc_t = typename Traits<QBITS>::acc_t;
    static constexpr bool kPrefetch = false;
    acc_t a0, a1;
    uint32_t nz;
    __device__ __forceinline__ void fetch(const uint8_t *, int, int) {}
    __device__ __forceinline__ void piece_pf(const uint4, const uint8_t *, int, int) {}
    __device__ __forceinline__ void reset()
    {
        a0 = 0;
        a1 = 0;
        nz = 0;
    }
    __device__ __forceinline__ void add4(const float4 q, float x0, float x1, float x2, float x3)
    {
        if (METRIC == kCosine) {
            a0 = fmaf(q.x, x0, a0);
            a0 = fmaf(q.y, x1, a0);
            a0 = fmaf(q.z, x2, a0);
            a0 = fmaf(q.w, x3, a0);
            a1 = fmaf(x0, x0, a1);
            a1 = fmaf(x1, x1, a1);
            a1 = fmaf(x2, x2, a1);
            a1 = fmaf(x3, x3, a1);
        } else {
            const float d0 = q.x - x0, d1 = q.y - x1, d2 = q.z - x2, d3 = q.w - x3;
            a0 = fmaf(d0, d0, a0);
            a0 = fmaf(d1, d1, a0);
            a0 = fmaf(d2, d2, a0);
            a0 = fmaf(d3, d3, a0);
        }
    }
    __device__ __forceinline__ void piece(const uint4 raw, const uint8_t *q, int j, const int r16, const int dim)
    {
        if (QBITS == 32) {  // resident elements are little-endian IEEE floats
            const float4 qv = reinterpret_cast<const float4 *>(q)[j];
            add4(qv, __uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z),
                 __uint_as_float(raw.w));
            if (METRIC == kCosine) nz |= (raw.x | raw.y | raw.z | raw.w) & 0x7FFFFFFFu;
        } else if (QBITS == 64) {  // native float64 arithmetic (FP64 VALU is ample at HBM rate)
            const double2 qv = reinterpret_cast<const double2 *>(q)[j];
            const double x0 = __longlong_as_double(((long long)raw.y << 32) | (long long)raw.x);
            const double x1 = __longlong_as_double(((long long)raw.w << 32) | (long long)raw.z);
            if (METRIC == kCosine) {
                a0 = fma(qv.x, x0, a0);
                a0 = fma(qv.y, x1, a0);
                a1 = fma(x0, x0, a1);
                a1 = fma(x1, x1, a1);
                nz |= (raw.x | raw.z) | ((raw.y | raw.w) & 0x7FFFFFFFu);
            } else {
                const double d0 = qv.x - x0, d1 = qv.y - x1;
                a0 = fma(d0, d0, a0);
                a0 = fma(d1, d1, a0);
            }
        } else {  // 16-bit: n = 2v - 65535 (odd, exact in float); dequantize(v) = n / 65535
            const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
            float n[8];
#pragma unroll
            for (int d = 0; d < 4; d++) {
                n[2 * d] = fmaf((float)(w[d] & 0xFFFFu), 2.0f, -65535.0f);
                n[2 * d + 1] = fmaf((float)(w[d] >> 16), 2.0f, -65535.0f);
            }
            const int e0 = j * 8;
            if (e0 + 8 > dim) {  // tail piece: padding decodes to -maxInt, mask it
#pragma unroll
                for (int i = 0; i < 8; i++)
                    if (e0 + i >= dim) n[i] = 0.0f;
            }
            const float4 *q4 = reinterpret_cast<const float4 *>(q);
            add4(q4[j], n[0], n[1], n[2], n[3]);
            add4(q4[r16 + j], n[4], n[5], n[6], n[7]);
        }
    }
    __device__ __forceinline__ float finish(const QConst &a, const Grp &g, bool lead)
    {
        a0 = grp_sum(a0, g);
        if (METRIC != kCosine) return (float)a0;
        a1 = grp_sum(a1, g);
        // a zero row is distance 1.0 (collection.go:828-830) == cos -1; an underflowed
        // norm is forced in (key -2) and settled by the float64 rerank -- and so is an
        // overflowed one (float32 rows with elements beyond ~1e19: finite in float64, the
        // reference ranks them; a row with an Inf / NaN element lands here too, its float64
        // distance is NaN and the host drops it)
        const bool zero = a1 == (acc_t)0;
        const bool over = sizeof(acc_t) == 4 && !((float)a1 <= 3.0e38f);
        float key;
        if (sizeof(acc_t) == 4)
            key = -(float)a0 * __frsqrt_rn((float)a1);
        else
            key = (float)(-a0 / sqrt(a1));
        if (__ballot((zero || over) && lead)) {  // rare
            nz = grp_or(nz, g);
            if (zero) key = nz ? -2.0f : 1.0f;
            if (over) key = -2.0f;
        }
        return key;
    }
};

// 8-bit rows, exact integer arithmetic.  With v' = v - 128 (one xor per dword)
// the decoded element is n = 2v - 255 = 2v' + 1.  The query is quantized on the
// host to Q_i = h*16384 + m*128 + l (balanced int8 digits, |Q| < 2^20), so
//     sum Q_i n_i = 2*(16384*H + 128*M + L) + sum Q_i,   H = sum h_i v'_i ...
// and sum n_i^2 = 4*sum v'^2 + 4*sum v' + count, all via v_dot4_i32_i8: five VALU
// ops per four elements, no conversions, and the only error left in the key is
// the query's quantization (bounded on the host, key_eps).
template <int METRIC>
struct RowAcc<8, METRIC> {
    static constexpr bool kPrefetch = SZG_QPF != 0;
    int H, M, L, SQ, SV;
    uint4 ph, pm, pl;  // digit planes of the piece about to be multiplied (dense phase, fetched one piece ahead)
    __device__ __forceinline__ void reset() { H = M = L = SQ = SV = 0; }
    __device__ __forceinline__ void fetch(const uint8_t *q, int j, int r16)
    {
        const uint4 *q4 = reinterpret_cast<const uint4 *>(q);
        ph = q4[j];
        pm = q4[r16 + j];
        pl = q4[2 * r16 + j];
    }
    __device__ __forceinline__ void piece_pf(const uint4 raw, const uint8_t *q, int jnext, const int r16)
    {
        const uint4 qh = ph, qm = pm, ql = pl;
        fetch(q, jnext, r16);
        mul(raw, qh, qm, ql);
    }
    __device__ __forceinline__ void mul(const uint4 raw, const uint4 qh, const uint4 qm, const uint4 ql)
    {
        const uint32_t w[4] = {raw.x ^ 0x80808080u, raw.y ^ 0x80808080u, raw.z ^ 0x80808080u,
                               raw.w ^ 0x80808080u};
        const uint32_t h[4] = {qh.x, qh.y, qh.z, qh.w};
        const uint32_t m[4] = {qm.x, qm.y, qm.z, qm.w};
        const uint32_t l[4] = {ql.x, ql.y, ql.z, ql.w};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            H = __builtin_amdgcn_sdot4((int)h[d], (int)w[d], H, false);
            M = __builtin_amdgcn_sdot4((int)m[d], (int)w[d], M, false);
            L = __builtin_amdgcn_sdot4((int)l[d], (int)w[d], L, false);
            SQ = __builtin_amdgcn_sdot4((int)w[d], (int)w[d], SQ, false);
            SV = __builtin_amdgcn_sdot4((int)w[d], 0x01010101, SV, false);
        }
    }
    __device__ __forceinline__ void piece(const uint4 raw, const uint8_t *q, int j, const int r16, const int dim)
    {
        const uint4 *q4 = reinterpret_cast<const uint4 *>(q);
        mul(raw, q4[j], q4[r16 + j], q4[2 * r16 + j]);
    }
    __device__ __forceinline__ float finish(const QConst &a, const Grp &g, bool lead)
    {
        // per-lane sums are exact integers below 2^24; combining the planes in float32
        // costs a few roundings (bounded in key_eps) and saves the float64 reduction
        float dot = fmaf(16384.0f, (float)H, fmaf(128.0f, (float)M, (float)L));
        int nrm = 4 * (SQ + SV);
        dot = grp_sum(dot, g);
        nrm = grp_sum(nrm, g);
        return key_of(dot, (float)nrm + a.norm_bias, a);
    }
    // the ranking key from the row's reduced sums: dot = 16384 H + 128 M + L, norm = sum n^2
    static __device__ __forceinline__ float key_of(float dot, float norm, const QConst &a)
    {
        const float d2 = fmaf(2.0f, dot, a.qconst);  // sum Q n
        if (METRIC == kCosine) return -(d2 * a.qscale) * __frsqrt_rn(norm);
        return fmaf(-2.0f * a.qscale, d2, a.qnorm2 + norm);
    }
};

// 8-bit rows, G queries scored per row read: the G query images lie side by side in LDS, `qbytes`
// apart.  A piece of the row is loaded, xor-ed and summed into the row norm (SQ, SV) once; each query of the group
// then costs its three plane reads and 12 v_dot4.  The arithmetic is RowAcc<8>'s, integer and exact, and the key
// is formed by the same float operations: a query's key for a row does not depend on how the queries are grouped.
// PL = 2: the queries carry two digit planes (|Q| <= 16000, a sketch index): the images in LDS hold the m and l planes
// only, `2 * r16 * 16` bytes apart, and a query costs two reads and 8 v_dot4; the key fmaf(128, M, L) is the float the
// three-plane form computes on the all-zero h plane.  NF: the row's norm comes from the resident array (the kernel
// loads it), SQ / SV are not summed.
template <int METRIC, int G, int PL = 3, bool NF = false>
struct RowAccGroup8 {
    static_assert(PL == 2 || PL == 3, "two or three digit planes");
    static constexpr bool kPrefetch = false;
    int H[PL == 3 ? G : 1], M[G], L[G], SQ, SV;
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int x = 0; x < G; x++) {
            if constexpr (PL == 3) H[x] = 0;
            M[x] = L[x] = 0;
        }
        SQ = SV = 0;
    }
    __device__ __forceinline__ void fetch(const uint8_t *, int, int) {}
    __device__ __forceinline__ void piece_pf(const uint4, const uint8_t *, int, int) {}
    __device__ __forceinline__ void piece(const uint4 raw, const uint8_t *q, int j, const int r16, const int dim)
    {
        const uint32_t w[4] = {raw.x ^ 0x80808080u, raw.y ^ 0x80808080u, raw.z ^ 0x80808080u,
                               raw.w ^ 0x80808080u};
        if constexpr (!NF) {
#pragma unroll
            for (int d = 0; d < 4; d++) {
                SQ = __builtin_amdgcn_sdot4((int)w[d], (int)w[d], SQ, false);
                SV = __builtin_amdgcn_sdot4((int)w[d], 0x01010101, SV, false);
            }
        }
        const int qbytes = PL * r16 * 16;
#pragma unroll
        for (int x = 0; x < G; x++) {
            const uint4 *q4 = reinterpret_cast<const uint4 *>(q + x * qbytes);
            if constexpr (PL == 3) {
                const uint4 qh = q4[j];
                const uint32_t h[4] = {qh.x, qh.y, qh.z, qh.w};
#pragma unroll
                for (int d = 0; d < 4; d++) H[x] = __builtin_amdgcn_sdot4((int)h[d], (int)w[d], H[x], false);
            }
            const uint4 qm = q4[(PL - 2) * r16 + j], ql = q4[(PL - 1) * r16 + j];
            const uint32_t m[4] = {qm.x, qm.y, qm.z, qm.w};
            const uint32_t l[4] = {ql.x, ql.y, ql.z, ql.w};
#pragma unroll
            for (int d = 0; d < 4; d++) {
                M[x] = __builtin_amdgcn_sdot4((int)m[d], (int)w[d], M[x], false);
                L[x] = __builtin_amdgcn_sdot4((int)l[d], (int)w[d], L[x], false);
            }
        }
        // The sums are due HERE (an empty asm that takes and returns them; no instruction).  Left free, instruction
        // selection puts the dots of the group's later queries off to the end of an unrolled row: their digit planes and
        // the row's xor-ed pieces then stay in registers for the whole row -- 256 registers and spills at G = 2 already.
#pragma unroll
        for (int x = 0; x < G; x++) {
            if constexpr (PL == 3) asm volatile("" : "+v"(H[x]));
            asm volatile("" : "+v"(M[x]), "+v"(L[x]));
        }
    }
    // the row's norm, reduced once for the whole group (norm_bias is the launch's)
    __device__ __forceinline__ float finish_norm(const QConst &a, const Grp &g)
    {
        const int nrm = grp_sum(4 * (SQ + SV), g);
        return (float)nrm + a.norm_bias;
    }
    __device__ __forceinline__ float finish_key(int x, float norm, const QConst &a, const Grp &g)
    {
        float dot = fmaf(128.0f, (float)M[x], (float)L[x]);
        if constexpr (PL == 3) dot = fmaf(16384.0f, (float)H[x], dot);  // (H == 0: the same float as without)
        dot = grp_sum(dot, g);
        return RowAcc<8, METRIC>::key_of(dot, norm, a);
    }
};

// 4-bit rows: the same with v'' = v - 8 (xor 0x88888888), n = 2v - 15 = 2v'' + 1,
// the query in five balanced int4 digit planes (|Q| < 2^19) and v_dot8_i32_i4:
// seven VALU ops per eight elements, no nibble unpacking.
template <int METRIC>
struct RowAcc<4, METRIC> {
    static constexpr bool kPrefetch = SZG_QPF != 0;
    int D[kPlanes4], SQ, SV;
    uint4 pp[kPlanes4];  // digit planes fetched one piece ahead (dense phase, SZG_QPF)
    __device__ __forceinline__ void reset()
    {
#pragma unroll
        for (int x = 0; x < kPlanes4; x++) D[x] = 0;
        SQ = SV = 0;
    }
    __device__ __forceinline__ void fetch(const uint8_t *q, int j, int r16)
    {
        const uint4 *q4 = reinterpret_cast<const uint4 *>(q);
#pragma unroll
        for (int x = 0; x < kPlanes4; x++) pp[x] = q4[x * r16 + j];
    }
    __device__ __forceinline__ void piece_pf(const uint4 raw, const uint8_t *q, int jnext, const int r16)
    {
        uint4 cur[kPlanes4];
#pragma unroll
        for (int x = 0; x < kPlanes4; x++) cur[x] = pp[x];
        fetch(q, jnext, r16);
        mul(raw, cur);
    }
    __device__ __forceinline__ void mul(const uint4 raw, const uint4 (&p)[kPlanes4])
    {
        const uint32_t w[4] = {raw.x ^ 0x88888888u, raw.y ^ 0x88888888u, raw.z ^ 0x88888888u,
                               raw.w ^ 0x88888888u};
#pragma unroll
        for (int d = 0; d < 4; d++) {
#pragma unroll
            for (int x = 0; x < kPlanes4; x++) {
                const uint32_t qd = d == 0 ? p[x].x : d == 1 ? p[x].y : d == 2 ? p[x].z : p[x].w;
                D[x] = __builtin_amdgcn_sdot8((int)qd, (int)w[d], D[x], false);
            }
            SQ = __builtin_amdgcn_sdot8((int)w[d], (int)w[d], SQ, false);
            SV = __builtin_amdgcn_sdot8((int)w[d], 0x11111111, SV, false);
        }
    }
    __device__ __forceinline__ void piece(const uint4 raw, const uint8_t *q, int j, const int r16, const int dim)
    {
        const uint4 *q4 = reinterpret_cast<const uint4 *>(q);
        uint4 p[kPlanes4];
#pragma unroll
        for (int x = 0; x < kPlanes4; x++) p[x] = q4[x * r16 + j];
        mul(raw, p);
    }
    // INT_OK: a lane's share of the row is short enough (<= 12 pieces) for the weighted plane sum
    // to stay inside int32 (|digit| <= 8, |v''| <= 8, 32 elements per piece): combine the planes
    // exactly with shift-adds and convert once.
    template <bool INT_OK = false>
    __device__ __forceinline__ float finish(const QConst &a, const Grp &g, bool lead)
    {
        float dot;
        if (INT_OK) {
            int t = D[kPlanes4 - 1];
#pragma unroll
            for (int x = kPlanes4 - 2; x >= 0; x--) t = (t << 4) + D[x];
            dot = (float)t;
        } else {
            dot = (float)D[kPlanes4 - 1];
#pragma unroll
            for (int x = kPlanes4 - 2; x >= 0; x--) dot = fmaf(16.0f, dot, (float)D[x]);
        }
        int nrm = 4 * (SQ + SV);
        dot = grp_sum(dot, g);
        nrm = grp_sum(nrm, g);
        const float norm = (float)nrm + a.norm_bias;
        const float d2 = fmaf(2.0f, dot, a.qconst);
        if (METRIC == kCosine) return -(d2 * a.qscale) * __frsqrt_rn(norm);
        return fmaf(-2.0f * a.qscale, d2, a.qnorm2 + norm);
    }
};

// ---- the scan ---------------------------------------------------------------

// LL, PP > 0: the row shape (lanes per row, pieces per lane) is a compile-time constant
// -- the common dims (384, 768, ...) get kernels whose addressing, reductions and query
// offsets are folded; 0, 0 = any shape, from a.map.
//
// G > 1 (8-bit top-k sweeps without masks, lists in registers): the launch's queries are walked in groups of up to G
// consecutive ones, every group in ONE pass over the rows -- G query images, G wave lists and G accumulator triples
// per lane against one load of each piece (RowAccGroup8).  G = 1 is the kernel without groups.
// Two compile-time forms of the G > 1 kernels beside today's (PL = 3, NF = false):
//  PL = 2  the launch's queries carry two digit planes (ScanArgs::planes): G images of 2 * r16 * 16 bytes in LDS.
//  NF      the rows' norms are resident (ScanArgs::row_norm): a row's norm is loaded a whole row ahead, in front of the
//          load of the row's first piece -- loads return in order, so the ring's counted wait for that piece covers it
//          and no wait changes -- and sits in the ring slot's own register (nring) until the piece is consumed.
template <int QBITS, int METRIC, int D, bool COLLECT, bool MASKED, bool NT, int LL = 0, int PP = 0, int G = 1, int PL = 3,
          bool NF = false>
__global__ __launch_bounds__(256, G > 1 ? kGroupMinBlocks : SZG_MIN_BLOCKS) void scan_kernel(const ScanArgs a)
{
    static_assert((LL == 0) == (PP == 0), "shape is fixed as a whole or not at all");
    static_assert(G == 1 || (QBITS == 8 && !COLLECT && !MASKED), "groups: unmasked 8-bit top-k sweeps only");
    static_assert(G > 1 || (PL == 3 && !NF), "the kernel without groups has one form");
    using Acc = std::conditional_t<G == 1, RowAcc<QBITS, METRIC>, RowAccGroup8<METRIC, G, PL, NF>>;
    extern __shared__ __align__(16) uint8_t smem[];

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wave = tid >> 6;
    const int nwaves = blockDim.x >> 6;
    const int r16 = LL ? LL * PP : a.map.r16;
    const int qbytes = PL == 2 ? 2 * r16 * 16 : (int)query_lds_bytes(QBITS, r16);  // an image in LDS; multiple of 16
    const int qskip = PL == 2 ? r16 * 16 : 0;  // two planes: the (all-zero) h plane in front of the image stays behind

    // LDS: G query images | G x nwaves wave lists ([query of the group][wave][kp]) | step lists
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem + G * qbytes);
    uint64_t *mylist = lists + (size_t)wave * a.kp;
    [[maybe_unused]] uint32_t *steplist =
        reinterpret_cast<uint32_t *>(smem + G * qbytes + (size_t)G * nwaves * (COLLECT ? 0 : a.kp) * sizeof(uint64_t)) +
        (size_t)wave * kStepList;
    const int L = LL ? LL : a.map.L, P = PP ? PP : a.map.P, gpw = LL ? kWave / LL : a.map.gpw;
    const int grp = lane / L;
    const int lig = lane - grp * L;
    const bool active = grp < gpw;
    const uint64_t stride = (uint64_t)gridDim.x * nwaves * gpw;
    const uint64_t row_first = ((uint64_t)blockIdx.x * nwaves + wave) * gpw;

    // Query-major batch: one launch walks the corpus once per query, back to
    // back.  Blocks move from query to query on their own (block-level barriers
    // only), so there is no chip-wide tail or launch gap between queries.
    // (G > 1: qi is the group's first query; slot x of the group holds query min(qi + x, n_queries - 1) -- the idle
    // slots of the launch's last group score its last query again and write no lists)
    for (int qi = 0; qi < a.n_queries; qi += G) {
    if (qi) __syncthreads();  // the previous query's lists have been merged
    auto slot_query = [&](int x) -> int { return G == 1 ? qi : min(qi + x, a.n_queries - 1); };
#pragma unroll
    for (int x = 0; x < G; x++) {   // stage the query into LDS (it is L2-resident after the first block)
        const uint4 *src = reinterpret_cast<const uint4 *>(
            reinterpret_cast<const uint8_t *>(a.query) + (size_t)slot_query(x) * a.query_stride + qskip);
        uint4 *dst = reinterpret_cast<uint4 *>(smem + x * qbytes);
        for (int i = tid; i < qbytes / 16; i += blockDim.x) dst[i] = src[i];
    }
    WaveList wls[G];
    QConst qcs[G];
#pragma unroll
    for (int x = 0; x < G; x++) {
        wls[x].init(mylist + (size_t)x * nwaves * a.kp, COLLECT ? 0 : a.kp, lane);
        const int q = slot_query(x);
        qcs[x] = QConst{a.qscale[q], a.qconst[q], a.qnorm2[q], (float)a.norm_bias};
        if (a.qmeta) scan_qmeta(a.qmeta, q, &qcs[x].qscale, &qcs[x].qconst, &qcs[x].qnorm2);  // (prepared on the card)
    }
    [[maybe_unused]] WaveList &wl = wls[0];
    [[maybe_unused]] const QConst &qc = qcs[0];
    __syncthreads();
    const uint64_t *allow_bits = a.allow_bits ? a.allow_bits + (size_t)qi * a.allow_stride : nullptr;

    // is the row of this lane's group at wave-row `row0` to be scanned?
    auto row_valid = [&](uint64_t row0) -> bool {
        const uint64_t r = row0 + grp;
        bool v = active && r < a.n_rows;
        if (MASKED && v) {
            const uint32_t rr = (uint32_t)r;
            if (a.live_bits) v = (a.live_bits[rr >> 6] >> (rr & 63)) & 1;         // removed
            if (v && allow_bits) v = (allow_bits[rr >> 6] >> (rr & 63)) & 1;      // filter
        }
        return v;
    };

    // Dense phase under masks (a.mask_dense: most rows pass, so every row is read and the masks
    // only decide at the row finish).  The wave's rows [row0, row0 + gpw) sit in one 64-bit
    // word of each bitmap; row0 is wave-uniform, so the words come through scalar loads and
    // never enter the vector-memory queue the ring is counting.
    auto dense_valid = [&](uint64_t row0) -> bool {
        if (!MASKED) return true;
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)row0);
        uint64_t w = ~0ull;
        if (a.live_bits) w &= a.live_bits[r0 >> 6];
        if (allow_bits) w &= allow_bits[r0 >> 6];
        return (w >> ((r0 & 63u) + (uint32_t)grp)) & 1ull;
    };

    // One row is done: reduce the group's L lanes, form the key, select.
    const Grp grp_info{L, lig, LL ? true : a.map.pow2 != 0};
    // The common case after warm-up -- no row of the step can enter the list -- costs one float
    // compare and one wave-uniform branch; clamping, the ordered 64-bit candidate and the exact
    // comparison happen only behind it.
    [[maybe_unused]] const uint32_t thr_ukey = COLLECT ? a.thr_ukeys[qi] : 0u;  // per sweep: radius / escalation threshold
    [[maybe_unused]] const float thr_key = COLLECT ? key_from_ordered(thr_ukey) : 0.0f;
    [[maybe_unused]] uint64_t *const cbuf = COLLECT ? a.collect_buf + (size_t)qi * a.collect_cap : nullptr;
    [[maybe_unused]] uint32_t *const ccount = COLLECT ? a.collect_count + (size_t)qi * kCandCountStride : nullptr;
    [[maybe_unused]] float nring[NF ? D : 1];  // NF: the norm loaded with the piece in ring slot u (a row's first)
    [[maybe_unused]] float norm_cur = 0.0f;    // NF: the norm of the row being consumed
    auto finish_row = [&](uint64_t row0, bool valid, Acc &acc) {
        if constexpr (G > 1) {  // one norm for the row, then each query of the group: its key, its pre-filter, its list
            const bool leader = valid && lig == 0;
            float norm;
            if constexpr (NF) norm = norm_cur;
            else norm = acc.finish_norm(qcs[0], grp_info);
            const uint32_t row = (uint32_t)(row0 + grp);
#pragma unroll
            for (int x = 0; x < G; x++) {
                float key = acc.finish_key(x, norm, qcs[x], grp_info);
                key = fminf(key, 3.0e38f);
                const bool maybe = leader && !(key > wls[x].worst_key);
                if (!__ballot(maybe)) continue;
                wls[x].offer(maybe, ((uint64_t)ordered_key(key) << 32) | row, lane);
            }
        } else {
            float key;
            if constexpr (QBITS == 4 && LL != 0 && PP <= 12)
                key = acc.template finish<true>(qc, grp_info, valid && lig == 0);
            else
                key = acc.finish(qc, grp_info, valid && lig == 0);
            const bool leader = valid && lig == 0;
            key = fminf(key, 3.0e38f);              // +inf (overflow) and NaN (minNum returns the number): worst finite
            const bool maybe = leader && !(key > (COLLECT ? thr_key : wl.worst_key));
            if (!__ballot(maybe)) return;
            const uint32_t row = (uint32_t)(row0 + grp);
            const uint64_t c = ((uint64_t)ordered_key(key) << 32) | row;

            if (COLLECT) {
                const bool hit = maybe && (uint32_t)(c >> 32) <= thr_ukey;
                const uint64_t m = __ballot(hit);
                if (m) {
                    const int first = __ffsll((long long)m) - 1;
                    uint32_t base = 0;
                    if (lane == first) base = atomicAdd(ccount, (uint32_t)__popcll(m));
                    base = __shfl(base, first);
                    if (hit) {
                        const uint32_t idx = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        if (idx < a.collect_cap) cbuf[idx] = c;
                    }
                }
            } else {
                wl.offer(maybe, c, lane);
            }
        }
    };

    // The piece ring: every lane keeps D 16-byte loads in flight, walking its
    // rows piece by piece (row-major), whatever the row size.  Slot u is consumed
    // and immediately re-issued with the piece D steps ahead, so HBM requests
    // keep flowing while a finished row is reduced and selected.  Loads are
    // unconditional (idle lanes read a dummy address) and the steady-state loop
    // is branch-free apart from the row-finish, so the compiler can emit
    // counted s_waitcnt vmcnt(D-1) instead of draining the queue.
    u32x4 ring[D];
    const uint64_t n_it = row_first < a.n_rows ? (a.n_rows - row_first + stride - 1) / stride : 0;
    Acc acc;
    acc.reset();

// The rings are macros, not templates or lambdas: the counted waits depend on how the compiler sees these loops.
// The drain every ring ends with: the pieces left are consumed (and re-issued while any is left to issue) under guards
#define SZG_RING_DRAIN(ISSUE, CONSUME)                                                  \
        while (consumed_ < np_) {                                                       \
            _Pragma("unroll") for (int u = 0; u < D; u++)                               \
            {                                                                           \
                if (consumed_ < np_) {                                                  \
                    CONSUME(u)                                                          \
                    consumed_++;                                                        \
                    if (issued_ < np_) {                                                \
                        ISSUE(u)                                                        \
                        issued_++;                                                      \
                    }                                                                   \
                }                                                                       \
            }                                                                           \
        }
// the unconditional prologue of the two dense rings (at least 2*D pieces: every slot is filled)
#define SZG_RING_FILL(NPX, ISSUE)                                                       \
        const uint64_t np_ = (NPX);                                                     \
        uint64_t issued_ = D, consumed_ = 0;                                            \
        _Pragma("unroll") for (int u = 0; u < D; u++)                                   \
        {                                                                               \
            ISSUE(u)                                                                    \
            __builtin_amdgcn_sched_barrier(0);                                          \
        }

// prologue (fill the ring), steady state (every slot consumed is re-issued), drain
#define SZG_RUN_RING(NPX, ISSUE, CONSUME)                                               \
    {                                                                                   \
        const uint64_t np_ = (NPX);                                                     \
        uint64_t issued_ = 0, consumed_ = 0;                                            \
        _Pragma("unroll") for (int u = 0; u < D; u++)                                   \
        {                                                                               \
            if (issued_ < np_) {                                                        \
                ISSUE(u)                                                                \
                issued_++;                                                              \
            }                                                                           \
        }                                                                               \
        while (consumed_ + 2 * D <= np_) {                                              \
            _Pragma("unroll") for (int u = 0; u < D; u++)                               \
            {                                                                           \
                CONSUME(u)                                                              \
                ISSUE(u)                                                                \
            }                                                                           \
            consumed_ += D;                                                             \
            issued_ += D;                                                               \
        }                                                                               \
        SZG_RING_DRAIN(ISSUE, CONSUME)                                                  \
    }

// The dense phase's ring: at least 2*D pieces, so the prologue is unconditional and the
// compiler can see that slot u's load is always the oldest of D in flight (counted
// s_waitcnt vmcnt(D-1) instead of draining the queue; the sched barriers keep the issue
// order it is counting on).
#define SZG_RUN_RING_DENSE(NPX, ISSUE, CONSUME)                                         \
    {                                                                                   \
        SZG_RING_FILL(NPX, ISSUE)                                                       \
        while (consumed_ + 2 * D <= np_) {                                              \
            _Pragma("unroll") for (int u = 0; u < D; u++)                               \
            {                                                                           \
                CONSUME(u)                                                              \
                ISSUE(u)                                                                \
                __builtin_amdgcn_sched_barrier(0);                                      \
            }                                                                           \
            consumed_ += D;                                                             \
            issued_ += D;                                                               \
        }                                                                               \
        SZG_RING_DRAIN(ISSUE, CONSUME)                                                  \
    }

// Row-shape kernels whose ring depth divides the pieces per lane: the steady state is unrolled
// over one whole ROW (P pieces, slot = piece % D), so every slot sits at a fixed piece of the
// row -- the row-finish test, the row jump of the issue cursor and the query offsets are
// compile-time facts and no per-piece branch is left.  The rows left over (< D + P pieces
// from the end) drain through the guarded tail loop.
#define SZG_RUN_RING_ROWS(NPX, ISSUE, CONSUME)                                          \
    {                                                                                   \
        SZG_RING_FILL(NPX, ISSUE)                                                       \
        while (consumed_ + D + PP <= np_) {                                             \
            _Pragma("unroll") for (int p_ = 0; p_ < PP; p_++)                           \
            {                                                                           \
                CONSUME(p_ % D)                                                         \
                ISSUE(p_ % D)                                                           \
                __builtin_amdgcn_sched_barrier(0);                                      \
            }                                                                           \
            consumed_ += PP;                                                            \
            issued_ += PP;                                                              \
        }                                                                               \
        SZG_RING_DRAIN(ISSUE, CONSUME)                                                  \
    }

    // ---- dense phase: no masks, L*P == r16, gpw*L == 64, every group's row in
    // range.  No predicates at all: pointer-increment addressing, unconditional
    // accumulation.  Covers all but (at most) the wave's last row step.
    uint64_t it_dense = 0;
    if ((!MASKED || a.mask_dense) && (LL || a.map.dense) && row_first + (uint64_t)gpw <= a.n_rows)
        it_dense = (a.n_rows - (uint64_t)gpw - row_first) / stride + 1;
    if (it_dense * (uint64_t)P < 2 * D) it_dense = 0;  // too short for the ring: general phase
    uint64_t crow0 = row_first;
    if (it_dense) {
        // linear rows: the group's lanes walk their row L*16 bytes at a time.  Tiled rows (L = 4,
        // 16 rows per wave step): the wave reads one 1 KiB step of its tile per piece.
        const RowLayout lay{a.pitch, a.tiled, a.steps};
        const uint8_t *iptr = a.rows + piece_offset(lay, row_first + grp, (uint32_t)lig);
        const uint64_t piece_step = a.tiled ? 1024u : (uint64_t)L * 16;
        const uint64_t row_jump = (a.tiled ? (stride >> 4) * ((uint64_t)a.steps * 1024) : stride * (uint64_t)a.pitch) -
                                  (uint64_t)(P - 1) * piece_step;
        int ip = 0, cp = 0, jc = lig;
        acc.fetch(smem, lig, r16);
        [[maybe_unused]] const float *nptr = NF ? a.row_norm + row_first + grp : nullptr;  // (rows of the dense phase: in range)
#define SZG_DN_ISSUE(u)                                                                 \
    {                                                                                   \
        if constexpr (NF) {                                                             \
            if (ip == 0) {                                                              \
                nring[u] = *nptr;                                                       \
                nptr += stride;                                                         \
            }                                                                           \
        }                                                                               \
        ring[u] = load_piece<NT>(iptr);                                                     \
        if (++ip == P) {                                                                \
            ip = 0;                                                                     \
            iptr += row_jump;                                                           \
        } else {                                                                        \
            iptr += piece_step;                                                         \
        }                                                                               \
    }
#define SZG_DN_CONSUME(u)                                                               \
    {                                                                                   \
        if constexpr (NF) {                                                             \
            if (cp == 0) norm_cur = nring[u];                                           \
        }                                                                               \
        const u32x4 v_ = ring[u];                                                       \
        if constexpr (Acc::kPrefetch)                                                   \
            acc.piece_pf(make_uint4(v_.x, v_.y, v_.z, v_.w), smem, cp + 1 == P ? lig : jc + L, r16); \
        else                                                                            \
            acc.piece(make_uint4(v_.x, v_.y, v_.z, v_.w), smem, jc, r16, a.dim);        \
        if (++cp == P) {                                                                \
            finish_row(crow0, dense_valid(crow0), acc);                                 \
            acc.reset();                                                                \
            cp = 0;                                                                     \
            jc = lig;                                                                   \
            crow0 += stride;                                                            \
        } else {                                                                        \
            jc += L;                                                                    \
        }                                                                               \
    }
        if constexpr (LL != 0 && PP % D == 0)
            SZG_RUN_RING_ROWS(it_dense * (uint64_t)P, SZG_DN_ISSUE, SZG_DN_CONSUME)
        else
            SZG_RUN_RING_DENSE(it_dense * (uint64_t)P, SZG_DN_ISSUE, SZG_DN_CONSUME)
#undef SZG_DN_ISSUE
#undef SZG_DN_CONSUME
    }

    // ---- general phase: masks, partial groups, ragged tails.
    // Under selective masks (MASKED && !mask_dense) most row steps of a wave hold no row that
    // passes; the wave first compacts the steps that do into its LDS step list (each lane tests
    // one step: a shift and a mask on the bitmap words), then rings over those only -- the
    // cost follows the rows that pass, not the corpus.
    {
    const RowLayout glay{a.pitch, a.tiled, a.steps};
    // (the test needs a step's gpw rows inside one bitmap word: gpw a power of two)
    const bool compact = MASKED && !a.mask_dense && (gpw & (gpw - 1)) == 0;
    uint64_t it_next = it_dense;  // next row step of this wave still to be looked at
    while (it_next < n_it) {
    uint64_t n_steps;             // steps of this round
    const uint64_t it_base = it_next;
    if (compact) {
        int nl = 0;
        while (it_next < n_it && nl <= kStepList - kWave) {
            const uint64_t it = it_next + lane;
            bool v = false;
            if (it < n_it) {
                const uint64_t r0 = row_first + it * stride;  // gpw rows, inside one bitmap word
                if (r0 < a.n_rows) {
                    const uint32_t rr = (uint32_t)r0;
                    uint64_t w = ~0ull;
                    if (a.live_bits) w &= a.live_bits[rr >> 6];
                    if (allow_bits) w &= allow_bits[rr >> 6];
                    const uint64_t cnt = min((uint64_t)gpw, (uint64_t)a.n_rows - r0);
                    const uint64_t m = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull);
                    v = ((w >> (rr & 63u)) & m) != 0;
                }
            }
            const uint64_t bal = __ballot(v);
            if (v) steplist[nl + __popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)(it - it_base);
            nl += __popcll(bal);
            it_next += kWave;
        }
        if (it_next > n_it) it_next = n_it;
        n_steps = (uint64_t)nl;
        __builtin_amdgcn_wave_barrier();
    } else {
        n_steps = n_it - it_next;
        it_next = n_it;
    }
    auto step_row0 = [&](uint64_t i) -> uint64_t {  // first row of the round's i-th step
        const uint64_t it = compact ? it_base + (i < n_steps ? steplist[i] : 0u) : it_base + i;
        return row_first + it * stride;
    };
    uint32_t okmask = 0;
    const uint64_t NP = n_steps * (uint64_t)P;  // pieces of this round
    // issue cursor
    uint64_t istep = 0;
    uint64_t irow0 = step_row0(0);
    int ip = 0;
    bool ivalid = n_steps ? row_valid(irow0) : false;
    bool inext = (MASKED && n_steps > 1) ? row_valid(step_row0(1)) : false;
    uint64_t irow = (uint32_t)(irow0 + grp);
    // consume cursor
    uint64_t cstep = 0;
    crow0 = irow0;
    int cp = 0;
    bool cvalid = false;

#define SZG_ISSUE(u)                                                                    \
    {                                                                                   \
        const int j_ = ip * L + lig;                                                    \
        const bool ok_ = ivalid && j_ < r16;                                            \
        if constexpr (NF) {                                                             \
            if (ip == 0) nring[u] = a.row_norm[ivalid ? irow : 0]; /* (n_rows > 0) */   \
        }                                                                               \
        ring[u] = load_piece<NT>(ok_ ? a.rows + piece_offset(glay, irow, (uint32_t)j_) : a.rows); \
        okmask = (okmask & ~(1u << (u))) | ((uint32_t)ok_ << (u));                      \
        if (++ip == P) {                                                                \
            ip = 0;                                                                     \
            istep++;                                                                    \
            irow0 = step_row0(istep);                                                   \
            irow = (uint32_t)(irow0 + grp);                                             \
            if (MASKED) {                                                               \
                ivalid = inext;                                                         \
                inext = istep + 1 < n_steps ? row_valid(step_row0(istep + 1)) : false;  \
            } else {                                                                    \
                ivalid = active && irow0 + grp < a.n_rows;                              \
            }                                                                           \
        }                                                                               \
    }

#define SZG_CONSUME(u)                                                                  \
    {                                                                                   \
        const int j_ = cp * L + lig;                                                    \
        const bool ok_ = (okmask >> (u)) & 1u;                                          \
        if (cp == 0) cvalid = ok_; /* piece 0 of the group's first lane is in range */  \
        if constexpr (NF) {                                                             \
            if (cp == 0) norm_cur = nring[u];                                           \
        }                                                                               \
        if (ok_) {                                                                      \
            const u32x4 v_ = ring[u];                                                   \
            acc.piece(make_uint4(v_.x, v_.y, v_.z, v_.w), smem, j_, r16, a.dim);                 \
        }                                                                               \
        if (++cp == P) {                                                                \
            finish_row(crow0, cvalid, acc);                                             \
            acc.reset();                                                                \
            cp = 0;                                                                     \
            cstep++;                                                                    \
            crow0 = step_row0(cstep);                                                   \
        }                                                                               \
    }

    if (NP) SZG_RUN_RING(NP, SZG_ISSUE, SZG_CONSUME)
#undef SZG_ISSUE
#undef SZG_CONSUME
    }  // rounds
    }
#undef SZG_RING_DRAIN
#undef SZG_RING_FILL
#undef SZG_RUN_RING
#undef SZG_RUN_RING_DENSE
#undef SZG_RUN_RING_ROWS

    if (COLLECT) continue;

    // block-wide k-select over the waves' lists
#pragma unroll
    for (int x = 0; x < G; x++) wls[x].flush(lane);
    __syncthreads();
#pragma unroll
    for (int x = 0; x < G; x++)
        if (qi + x < a.n_queries)  // (block-uniform)
            block_merge_lists(lists + (size_t)x * nwaves * a.kp, nwaves, a.kp,
                              a.block_lists + ((size_t)(qi + x) * gridDim.x + blockIdx.x) * a.kp, tid, blockDim.x);
    // gfx9 counts loads and stores in one vmcnt and retires them out of order with respect
    // to each other: with the list stores above possibly pending at the top of the next
    // query's sweep, every ring wait would have to be vmcnt(0) -- which also waits for the
    // load just issued.  Drain here, once per query (group), so the ring gets counted waits.
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0); expcnt, lgkmcnt untouched
    }  // for qi
}

template <int QBITS, int METRIC, bool COLLECT, int LL, int PP, int D, int G = 1, int PL = 3, bool NF = false>
hipError_t launch_shaped(const ScanArgs &a, bool nt, dim3 g, dim3 b, size_t lds, hipStream_t stream)
{
    if (nt)
        hipLaunchKernelGGL((scan_kernel<QBITS, METRIC, D, COLLECT, false, true, LL, PP, G, PL, NF>), g, b, lds, stream, a);
    else
        hipLaunchKernelGGL((scan_kernel<QBITS, METRIC, D, COLLECT, false, false, LL, PP, G, PL, NF>), g, b, lds, stream, a);
    return hipGetLastError();
}

template <int QBITS, int METRIC, bool COLLECT, bool MASKED, int D, int G = 1, int PL = 3, bool NF = false>
hipError_t launch_any_shape(const ScanArgs &a, bool nt, dim3 g, dim3 b, size_t lds, hipStream_t stream)
{
    if (nt)  // whole lines per load instruction: stream past the caches
        hipLaunchKernelGGL((scan_kernel<QBITS, METRIC, D, COLLECT, MASKED, true, 0, 0, G, PL, NF>), g, b, lds, stream, a);
    else
        hipLaunchKernelGGL((scan_kernel<QBITS, METRIC, D, COLLECT, MASKED, false, 0, 0, G, PL, NF>), g, b, lds, stream, a);
    return hipGetLastError();
}

// the kernels of group size G (scan_variant's choice; G > 1 exists for unmasked 8-bit top-k sweeps with the short ring)
// in the form (PL digit planes, NF: resident norms) the launch's arguments ask for
template <int QBITS, int METRIC, bool COLLECT, bool MASKED, int G, int PL = 3, bool NF = false>
hipError_t launch_scan_group(const ScanArgs &a, const ScanVariant &v, dim3 g, dim3 b, size_t lds, hipStream_t stream)
{
    if constexpr (!MASKED) {
// (G > 1: the shape's kernel at the group ring's other depth, where it has one -- scan_group_ring_of, scan_plan.h)
#define SZG_TRY_SHAPE(l, p, d)                                                                 \
    if (v.shaped == l * 100 + p) {                                                             \
        if constexpr (G > 1 && scan_group_ring_of(p, SZG_SHAPE_RING(d), kGroupRingAlt) != SZG_SHAPE_RING(d)) {        \
            if (v.ring_depth == kGroupRingAlt)                                                 \
                return launch_shaped<QBITS, METRIC, COLLECT, l, p, kGroupRingAlt, G, PL, NF>(a, v.nontemporal != 0, g, b, lds, stream); \
        }                                                                                      \
        if (v.ring_depth != SZG_SHAPE_RING(d)) return hipErrorInvalidValue;                    \
        return launch_shaped<QBITS, METRIC, COLLECT, l, p, SZG_SHAPE_RING(d), G, PL, NF>(a, v.nontemporal != 0, g, b, lds, stream); \
    }
        if constexpr (QBITS == 4) {
            SZG_SHAPES_4(SZG_TRY_SHAPE)
        } else if constexpr (QBITS == 8) {
            SZG_SHAPES_8(SZG_TRY_SHAPE)
        } else if constexpr (QBITS == 16) {
            SZG_SHAPES_16(SZG_TRY_SHAPE)
        } else if constexpr (QBITS == 32) {
            SZG_SHAPES_32(SZG_TRY_SHAPE)
        } else {
            SZG_SHAPES_64(SZG_TRY_SHAPE)
        }
#undef SZG_TRY_SHAPE
    }
    if (v.shaped) return hipErrorInvalidValue;  // (scan_variant named a kernel this unit does not carry)
    if constexpr (G == 1) {
        if (v.deep)
            return launch_any_shape<QBITS, METRIC, COLLECT, MASKED, kRingDeep>(a, v.nontemporal != 0, g, b, lds, stream);
    } else if (v.deep) {
        return hipErrorInvalidValue;
    }
    return launch_any_shape<QBITS, METRIC, COLLECT, MASKED, kRingShort, G, PL, NF>(a, v.nontemporal != 0, g, b, lds, stream);
}

#ifndef SZG_GROUP_FORM

template <int QBITS, int METRIC, bool COLLECT, bool MASKED>
hipError_t launch_scan_qmcm(const ScanArgs &a, int grid, int block, hipStream_t stream)
{
    const dim3 g(grid), b(block);
    ScanPlanIn in = scan_plan_in(QBITS, a, block);
    in.collect = COLLECT;  // (the kernel this launcher instantiates: launch_scan_qm chose it from the same two facts)
    in.masked = MASKED;
    const ScanVariant v = scan_variant(in);
    const size_t lds = scan_lds_bytes(QBITS, a.map, COLLECT ? 0 : a.kp, block, v.group, a.planes, v.matrix_blocks());
    // (the per-query constants of every launch but the wide one are read up to kMaxSweepsPerLaunch queries)
    if (!v.wide && a.n_queries > kMaxSweepsPerLaunch) return hipErrorInvalidValue;
    if constexpr (QBITS == 8 && !COLLECT && !MASKED) {
        // the matrix sweep: up to kMatrixQueries queries per row read on the matrix cores (kernels_scan_mx.hip)
        if (v.matrix) return METRIC == kCosine ? launch_scan_mx_m1(a, v, grid, block, lds, stream) : launch_scan_mx_m0(a, v, grid, block, lds, stream);
        // G > 1: the form of the kernel -- two digit planes where the queries carry two (bit 0), resident norms where
        // the launch has them (bit 1); every form is an object of its own (SZG_GROUP_FORM)
        if (v.group > 1) return launch_scan_g8(METRIC, (a.planes == 2 ? 1 : 0) | (a.row_norm ? 2 : 0), a, v, grid, block, lds, stream);
    }
    if constexpr (QBITS == 8 && COLLECT && !MASKED) {
        // ... and its collect form (objects of their own: the top-k kernels' code does not change with it)
        if (v.matrix) return METRIC == kCosine ? launch_scan_mxc_m1(a, v, grid, block, lds, stream) : launch_scan_mxc_m0(a, v, grid, block, lds, stream);
    }
    if (v.group != 1) return hipErrorInvalidValue;
    return launch_scan_group<QBITS, METRIC, COLLECT, MASKED, 1>(a, v, g, b, lds, stream);
}

template <int QBITS, int METRIC>
hipError_t launch_scan_qm(const ScanArgs &a, int grid, int block, hipStream_t stream)
{
    const bool masked = scan_masked(a);
    if (a.collect) {
        if (masked) return launch_scan_qmcm<QBITS, METRIC, true, true>(a, grid, block, stream);
        return launch_scan_qmcm<QBITS, METRIC, true, false>(a, grid, block, stream);
    }
    if (masked) return launch_scan_qmcm<QBITS, METRIC, false, true>(a, grid, block, stream);
    return launch_scan_qmcm<QBITS, METRIC, false, false>(a, grid, block, stream);
}
#endif  // !SZG_GROUP_FORM

}  // namespace

}  // namespace szg

#define SZG_CAT2(a, b) a##b
#define SZG_CAT(a, b) SZG_CAT2(a, b)
#ifdef SZG_GROUP_FORM
// -DSZG_GROUP_FORM=0..3 (8-bit rows): the G = 2 and G = 4 kernels of ONE form and nothing else: bit 0 = two digit
// planes, bit 1 = resident norms.  Eight objects of twelve kernels: in one unit per metric they took five minutes.
hipError_t szg::SZG_CAT(SZG_CAT(launch_scan_g8m, SZG_SCAN_METRIC), SZG_CAT(f, SZG_GROUP_FORM))(const ScanArgs &a, const ScanVariant &v,
                                                                                           int grid, int block, size_t lds,
                                                                                           hipStream_t stream)
{
    static_assert(SZG_QBITS == 8, "groups: 8-bit rows");
    constexpr int PL = (SZG_GROUP_FORM & 1) ? 2 : 3;
    constexpr bool NF = (SZG_GROUP_FORM & 2) != 0;
    const dim3 g(grid), b(block);
    if (v.group == 4) return launch_scan_group<8, SZG_SCAN_METRIC, false, false, 4, PL, NF>(a, v, g, b, lds, stream);
    if (v.group == 2) return launch_scan_group<8, SZG_SCAN_METRIC, false, false, 2, PL, NF>(a, v, g, b, lds, stream);
    return hipErrorInvalidValue;
}
#else
// the scan kernels of ONE quantization and ONE metric (0 Euclidean / 1 cosine): ten objects of ~35 s instead of five of
// ~70 s, which is what a parallel build of the library waits for
hipError_t szg::SZG_CAT(SZG_CAT(launch_scan_q, SZG_QBITS), SZG_CAT(m, SZG_SCAN_METRIC))(const ScanArgs &a, int grid, int block,
                                                                                      hipStream_t stream)
{
    return launch_scan_qm<SZG_QBITS, SZG_SCAN_METRIC>(a, grid, block, stream);
}
#endif  // SZG_GROUP_FORM
