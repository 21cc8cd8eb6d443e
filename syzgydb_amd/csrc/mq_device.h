// mq_device.h -- the shared (multi-query) sweeps for gfx950: B queries per pass of the corpus.
//
// The single-query scan (kernels_scan.hip) is HBM-bound: every query costs one full sweep.  When the caller hands
// over a batch (szg_search_topk with n_queries > 1, the reference's concurrent Searches under RLock,
// collection.go:570), the sweep is shared: the corpus streams through once and the B query x row dot products go to
// the matrix cores.
//
//   mq_score_bf16s_kernel  64-, 32- and 16-bit rows: rows and queries rounded to bfloat16 on the fly,
//                          v_mfma_f32_16x16x32_bf16; the sweep only RANKS -- its candidates are scored again in
//                          float32, re-ranked in float64 and certified against the bfloat16 bound.
//   mq_score_bf16d(8)_kernel  16-bit rows with resident norms and 8-bit rows of more than 48 queries: the same
//                          arithmetic on codes that arrive in the MFMA operand layout (no LDS stage).
//   mq_score_i8(s)_kernel  8- and 4-bit rows: exact integer arithmetic, v_mfma_i32_16x16x64_i8 on the row bytes
//                          against int8 digit planes of the query.
//   mq_thr_radix_kernel, mq_select_kernel, cand_refine_kernel, cand_rescore_kernel, cand_select_kernel
//                          thresholds of the fused selection, per-query selection over a score matrix or over the
//                          collected candidates, the float32 re-score of a bfloat16 sweep's band.
//
// A wave owns a tile of 16 rows; the D layout of the 16x16 product is column = lane & 15 (the tile's row),
// row = (lane >> 4) * 4 + reg (the query inside its block of 16).  (Round 4 removed the float32 MFMA form,
// v_mfma_f32_16x16x4_f32 at 62 % of its matrix roof: every width has an HBM-bound sweep now.)
//
// One source per kernel family; the two large ones are built once per row width (-DSZG_ROW_BITS=..., as
// kernels_scan.hip's SZG_QBITS):
//   kernels_mq_bf16.hip   mq_score_bf16s_kernel                          32 | 16 | 64
//   kernels_mq_bf16d.hip  mq_score_bf16d_kernel, mq_score_bf16d8_kernel  (16- and 8-bit rows in one object)
//   kernels_mq_i8.hip     mq_score_i8_kernel, mq_score_i8s_kernel        8 | 4
//   kernels_mq.hip        the selection kernels, the image and LDS sizes, the two public dispatchers (kernels.h)
// This header holds what the sweeps share on the device, the one launch sequence and the families' entry points.
#pragma once
#include "kernels.h"
#include "device_lists.h"

#include <type_traits>

namespace szg {

// The families' entry points behind launch_mq_score_bf16 / launch_mq_score_i8 (kernels_mq.hip): each source defines
// the template and instantiates it for the width(s) it is built with.  lds = mq_bf16_lds_bytes / mq_i8_lds_bytes.
template <int ROW_BITS>  // 32, 16, 64: the LDS-staged bfloat16 sweep
hipError_t launch_mq_bf16s_rows(const MqArgs &a, int nb, int grid, size_t lds, hipStream_t stream);
template <int ROW_BITS>  // 16 (needs MqArgs::row_norm), 8 (tiled rows): the direct bfloat16 sweeps
hipError_t launch_mq_bf16d_rows(const MqArgs &a, int nb, int grid, size_t lds, hipStream_t stream);
template <int ROW_BITS>  // 8, 4: the exact integer sweeps
hipError_t launch_mq_i8_rows(const MqArgs &a, int nb, int grid, size_t lds, hipStream_t stream);

namespace {

// what the LDS size functions (kernels_mq.hip) must know of the kernels' blocks
#ifndef SZG_MQ8_WAVES
#define SZG_MQ8_WAVES 12  // waves per block (one block per CU) of the int8 sweeps (the 12-step shape kernel: 8)
#endif
#ifndef SZG_MQB_WAVES
#define SZG_MQB_WAVES 8  // waves per block (one block per CU) of the bfloat16 sweep: 8 x 2 steps x 2 KiB = 32 KiB in
#endif                    // flight per CU (16 waves or 3 steps: -3..-6 %, as on every streaming kernel here)
constexpr int kMq8TableRows = 6;  // 48-float rows after a group's image: qscale, qconst, qnorm2 | thresholds, pre-test s, w
typedef int v4i32b __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// plain (cacheable) loads: the MFMA operand layout makes every lane group read
// 64-byte segments, and the other half of each 128-byte line is wanted one step
// later -- a non-temporal hint evicts it first (measured 1.22x HBM over-fetch)
__device__ __forceinline__ u32x4 load_plain(const uint8_t *p)
{
    return *reinterpret_cast<const u32x4 *>(p);
}
// tiled rows (4- and 8-bit): a wave instruction reads one whole KiB that is used once per sweep -- stream it past
// the caches.  The hint is a template argument, not a run-time flag: `if (nt) nontemporal_load(p) else load(p)` is
// folded by the optimiser into ONE plain load before inlining (the two arms read the same address and the merged
// instruction keeps only the metadata both carry), which is how the int8 sweeps came to run without the hint.
template <bool NT>
__device__ __forceinline__ u32x4 load_stream(const uint8_t *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    else return *reinterpret_cast<const u32x4 *>(p);
}

// Stage n16 16-byte words of a query image into LDS.  Written as load-all / store-all groups of six: with the plain
// `dst[i] = src[i]` loop every iteration waited for its own load, i.e. 18 L2 round trips back to back for a 147 KiB
// image (~20 us at the head of EVERY sweep launch, the prefix pass included, with HBM idle).
__device__ __forceinline__ void stage_image(uint4 *dst, const uint4 *src, int n16, int tid, int nthreads)
{
    constexpr int U = 6;
    int i = tid;
    for (; i + (U - 1) * nthreads < n16; i += U * nthreads) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = src[i + u * nthreads];
#pragma unroll
        for (int u = 0; u < U; u++) dst[i + u * nthreads] = v[u];
    }
    for (; i < n16; i += nthreads) dst[i] = src[i];
}

// Fused selection.  A (query, row) pair whose key is at or below the query's threshold goes
// into the wave's own little hit buffer in LDS (wave-synchronous append: ballot + prefix
// popcount, no atomics); when 64 are waiting -- normally only at the end of the kernel --
// each lane takes one, checks the row's mask bits and claims a slot in the query's global
// candidate buffer.  (One returning global atomic per hit, issued where the hit occurs,
// stalls the wave for a full memory round trip each time: measured +40 % on the sweep.)
constexpr int kHitCap = 64;
struct HitBuf {
    uint64_t *cand;  // [kHitCap]
    uint8_t *query;  // [kHitCap]
    int n;           // wave-uniform
};

__device__ __forceinline__ void hit_flush(const MqArgs &a, HitBuf &hb, int lane)
{
    if (lane < hb.n) {
        const uint64_t c = hb.cand[lane];
        const int q = hb.query[lane];
        const uint32_t r = (uint32_t)c;
        bool ok = true;
        if (a.live_bits) ok = (a.live_bits[r >> 6] >> (r & 63)) & 1;
        if (ok && a.allow_bits) ok = (a.allow_bits[(size_t)q * a.allow_stride + (r >> 6)] >> (r & 63)) & 1;
        if (ok) {
            const uint32_t idx = atomicAdd(a.cand_count + q * kCandCountStride, 1u);
            if (idx < a.cand_cap) a.cand_buf[(size_t)q * a.cand_cap + idx] = c;
        }
    }
    // gfx9: loads, stores and atomics share one vmcnt and retire out of order among
    // themselves; leaving these pending would turn every later ring wait into vmcnt(0)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    hb.n = 0;
}

__device__ __forceinline__ void hit_offer(const MqArgs &a, HitBuf &hb, int lane, bool hit, int q, uint64_t row,
                                          float key)
{
    const uint64_t m = __ballot(hit);
    if (!m) return;
    const int cnt = __popcll(m);
    if (hb.n + cnt > kHitCap) hit_flush(a, hb, lane);
    if (hit) {
        const int pos = hb.n + __popcll(m & ((1ull << lane) - 1ull));
        hb.cand[pos] = ((uint64_t)ordered_key(key) << 32) | (uint32_t)row;
        hb.query[pos] = (uint8_t)q;
    }
    hb.n += cnt;
}

// OR of a 32-bit value over the wave (uniform result): four DPP steps inside each row of 16
// lanes, then the four rows through scalar registers
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t v)
{
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) | (uint32_t)__builtin_amdgcn_readlane((int)v, 16) |
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

// The tile finish of the fused-selection sweeps.  A tile yields NB x 4 (query, row) keys per lane;
// almost none of them is at or below its query's threshold.  All keys are formed first (pure
// VALU work), the lanes' hit bits are OR-ed over the wave, and only the (query block, register)
// slots that hold a hit somewhere go through hit_offer: one wave-uniform branch per tile in the
// common case instead of one ballot and branch per slot.
template <int NB>
__device__ __forceinline__ void offer_tile_hits(const MqArgs &a, HitBuf &hb, int lane, int c, uint32_t hm,
                                                const float (&keys)[NB][4], uint64_t row, int qoff = 0)
{
    if (!__ballot(hm != 0)) return;
    // ONE copy of the offer (and of the flush inside it), walked over the slots that hold a hit somewhere in the wave:
    // `un` is wave-uniform, so the loop and the slot's key select are scalar-controlled.  (Round 3 unrolled the NB x 4
    // slots -- 24 inlined offers with a flush each, thousands of instructions in the middle of every sweep's loop: the
    // register allocator split the load ring's live ranges around them and copied freshly loaded registers at the
    // loop's end, which waits for every load in flight.)
    uint32_t un = wave_or_u32(hm);
    // (the keys as ONE register vector, indexed by the scalar slot number: v_movrels / s_set_gpr_idx, no memory.  A
    // chain of selects over the array was turned into a table in scratch memory, written by every tile.)
    typedef float keyvec __attribute__((ext_vector_type(NB <= 2 ? 8 : (NB <= 4 ? 16 : 32))));
    keyvec kv;
#pragma unroll
    for (int i = 0; i < NB * 4; i++) kv[i] = keys[i >> 2][i & 3];
    while (un) {
        const int s = __builtin_ctz(un);
        un &= un - 1u;
        const float key = kv[s];
        hit_offer(a, hb, lane, (hm >> s) & 1u, qoff + (s >> 2) * 16 + c * 4 + (s & 3), row, key);
    }
}

// ---- host side: the one launch sequence and the fan-outs over a launch's compile-time parameters ----------------------

// a kernel whose dynamic LDS may exceed the default limit: raise the limit, launch, report
template <typename... P, typename... Args>
hipError_t launch_lds(void (*kern)(P...), int grid, int threads, size_t lds, hipStream_t stream, const Args &...args)
{
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, args...);
    return hipGetLastError();
}

// f(metric, collect) with the batch's metric and selection form as std::integral_constants
template <typename F>
hipError_t with_metric_collect(const MqArgs &a, F &&f)
{
    using cosine = std::integral_constant<int, kCosine>;
    using euclid = std::integral_constant<int, kEuclidean>;
    if (a.collect) {
        if (a.metric == kCosine) return f(cosine{}, std::true_type{});
        return f(euclid{}, std::true_type{});
    }
    if (a.metric == kCosine) return f(cosine{}, std::false_type{});
    return f(euclid{}, std::false_type{});
}

// f(nb) with the query blocks of a bfloat16 sweep (1..6) as a std::integral_constant
template <typename F>
hipError_t with_query_blocks6(int nb, F &&f)
{
    switch (nb) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

}  // namespace szg
