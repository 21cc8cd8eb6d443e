// kernels_scan_merge.hip -- what a one-sweep call runs around its sweeps: the kernels that merge the blocks' sorted
// candidate lists (tournament, rank merge, the short-list merge of the sketch sweep) with their launchers, and
// launch_scan, which hands a launch to the object of its row width and metric (kernels_scan.hip; scan_plan.cpp decides).
#include "kernels.h"
#include "device_lists.h"

namespace szg {

namespace {

constexpr int kWave = 64;

// ---- merge of sorted candidate lists ----------------------------------------

// minimum of a 64-bit value over the wave, returned in every lane: four DPP
// steps reduce each row of 16 lanes, four readlanes finish across rows.
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v)
{
#define SZG_DPP_MIN(ctrl)                                                                  \
    {                                                                                      \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(                        \
            (int)(uint32_t)v, (int)(uint32_t)v, ctrl, 0xF, 0xF, false);                    \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(                        \
            (int)(uint32_t)(v >> 32), (int)(uint32_t)(v >> 32), ctrl, 0xF, 0xF, false);    \
        const uint64_t o_ = ((uint64_t)hi_ << 32) | lo_;                                   \
        v = o_ < v ? o_ : v;                                                               \
    }
    SZG_DPP_MIN(0xB1)   // quad_perm [1,0,3,2]
    SZG_DPP_MIN(0x4E)   // quad_perm [2,3,0,1]
    SZG_DPP_MIN(0x141)  // row_half_mirror
    SZG_DPP_MIN(0x140)  // row_mirror
#undef SZG_DPP_MIN
    uint64_t m = kInvalidCand;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, r * 16);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), r * 16);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        m = o < m ? o : m;
    }
    return m;
}

// Tournament merge: one wave per group of up to 64 sorted lists, one list per
// lane; kp rounds of "take the smallest head".  Lists are staged in LDS with
// coalesced loads first, so each round is a DPP reduction plus one LDS read.
__global__ __launch_bounds__(256) void merge_heads_kernel(const uint64_t *in, int n_lists, int kp,
                                                          uint64_t *out, int out_stride)
{
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);
    const int lane = threadIdx.x & 63;
    const int first = blockIdx.x * kWave;
    const int mine = min(kWave, n_lists - first);
    const int total = mine * kp;
    in += (size_t)blockIdx.y * n_lists * kp;     // blockIdx.y = query of the batch
    out += (size_t)blockIdx.y * (out_stride ? (size_t)out_stride : (size_t)gridDim.x * kp);
    for (int i = threadIdx.x; i < total; i += blockDim.x) lists[i] = in[(size_t)first * kp + i];
    __syncthreads();
    if (threadIdx.x >= kWave) return;  // the other waves only helped staging
    int pos = 0;
    uint64_t head = lane < mine ? lists[(size_t)lane * kp] : kInvalidCand;
    uint64_t *o = out + (size_t)blockIdx.x * kp;
    uint64_t keep = kInvalidCand;  // lane i keeps output i (+64 per round of 64)
    for (int r = 0; r < kp; r++) {
        const uint64_t m = wave_min_u64(head);
        if (head == m && m != kInvalidCand) {  // entries are unique: exactly one lane advances
            pos++;
            head = pos < kp ? lists[(size_t)lane * kp + pos] : kInvalidCand;
        }
        if ((r & 63) == lane) keep = m;
        if ((r & 63) == 63 || r == kp - 1) {
            const int idx = (r & ~63) + lane;
            if (idx <= r) o[idx] = keep;
            keep = kInvalidCand;
        }
    }
}

// minimum of a 32-bit value over the wave (lanes 0..15 only: ROW0), wave-uniform: four DPP steps reduce each row of
// 16 lanes, readlanes finish across rows
template <bool ROW0>
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
    uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    if (!ROW0) {
        m = min(m, (uint32_t)__builtin_amdgcn_readlane((int)v, 16));
        m = min(m, (uint32_t)__builtin_amdgcn_readlane((int)v, 32));
        m = min(m, (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
    }
    return m;
}

// the smallest candidate of the wave (lanes 0..15 only: ROW0; the others hold kInvalidCand), wave-uniform: the
// minimum of the ordered keys (high words), then -- only when several lanes hold that key -- of their rows.  Half the
// work of a 64-bit reduction per tournament round.
template <bool ROW0>
__device__ __forceinline__ uint64_t wave_min_cand(uint64_t v)
{
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t mhi = wave_min_u32<ROW0>(hi);
    const uint64_t tie = __ballot(hi == mhi);
    uint32_t mlo;
    if (__popcll(tie) == 1)
        mlo = (uint32_t)__builtin_amdgcn_readlane((int)lo, __ffsll((long long)tie) - 1);
    else
        mlo = wave_min_u32<ROW0>(hi == mhi ? lo : 0xFFFFFFFFu);
    return ((uint64_t)mhi << 32) | mlo;
}

// Short-list merge (the sketch sweep): ONE block per query (blockIdx.y) selects the kp best of the
// n_lists sorted block lists of m entries each (m < kp) and writes them, sorted, to out[0, kp); out[kp] gets the drop
// bound -- the smallest m-th entry of a FULL block list (kInvalidCand if no list is full): every row a block did not
// output is above its list's m-th entry.
// By selection: let h be the kp-th smallest of the lists' FIRST entries (kInvalidCand with fewer than kp non-empty
// lists).  kp lists start at or below h, so at least kp entries are <= h and the kp best are among the entries <= h --
// typically little more than kp of them, since the best rows fall to the blocks almost one each.  Every thread finds
// the rank of its list's first entry among all first entries (the one of rank kp - 1 publishes h), the entries <= h
// are compacted into LDS in any order, wave 0 sorts them with one bitonic network and writes the first kp.  Entries
// are unique, so the sorted result does not depend on the order of the compaction.
// By tournament, when more entries are <= h than the network's buffer holds (the sel array below, less two words):
// stage 1: wave w runs a tournament over lists [64w, 64w + 64), one list per lane, each lane's next head fetched one
// advance ahead; stage 2: wave 0 runs one over the <= 16 results.
// Needs n_lists <= 1024 and merge_short_lds(n_lists, m, kp) <= 64 KiB (merge_short_fits).
__global__ __launch_bounds__(1024) void merge_short_kernel(const uint64_t *in, int n_lists, int m, int kp,
                                                           uint64_t *out, int out_stride)
{
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);  // [n_lists][m]
    const int ngroups = (n_lists + kWave - 1) / kWave;
    uint64_t *sel = lists + (size_t)n_lists * m;           // [ngroups][kp]: each group's kp best
    uint64_t *drops = sel + (size_t)ngroups * kp;          // [ngroups]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    in += (size_t)blockIdx.y * n_lists * m;
    out += (size_t)blockIdx.y * out_stride;
    const int total = n_lists * m;
    for (int i = tid; i < total; i += blockDim.x) lists[i] = in[i];
    // the selection's words in sel: the entries <= h from the front, h and their count in its last two
    const int cap = merge_short_cap(n_lists, kp);
    uint64_t *h_word = sel + cap;
    uint32_t *count_word = reinterpret_cast<uint32_t *>(sel + cap + 1);
    if (tid == 0) {
        *h_word = kInvalidCand;
        *count_word = 0u;
    }
    __syncthreads();
    {
        const bool have = tid < n_lists;
        const uint64_t *my = lists + (size_t)(have ? tid : 0) * m;
        // (kInvalidCand is the largest value: lists that are not full drop out of the minimum by themselves)
        const uint64_t drop = wave_min_cand<false>(have ? my[m - 1] : kInvalidCand);
        if (lane == 0 && wave < ngroups) drops[wave] = drop;
        const uint64_t first = have ? my[0] : kInvalidCand;
        if (first != kInvalidCand) {
            int rank = 0;
            for (int j = 0; j < n_lists; j++) rank += lists[(size_t)j * m] < first ? 1 : 0;
            if (rank == kp - 1) *h_word = first;  // (unique entries: one thread at most)
        }
        __syncthreads();
        const uint64_t h = *h_word;
        int c = 0;
        if (have)
            while (c < m && my[c] <= h && my[c] != kInvalidCand) c++;
        if (c) {
            const int at = (int)atomicAdd(count_word, (uint32_t)c);
            if (at + c <= cap)
                for (int i = 0; i < c; i++) sel[at + i] = my[i];
        }
        __syncthreads();
        const int found = (int)*count_word;
        int S = 1;
        while (S < found) S <<= 1;
        if (S <= cap) {
            if (wave != 0) return;
            for (int i = found + lane; i < S; i += kWave) sel[i] = kInvalidCand;
            __builtin_amdgcn_wave_barrier();
            // one wave: its LDS accesses complete in program order, a step's exchanges touch disjoint pairs
            for (int k = 2; k <= S; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int p = lane; p < S / 2; p += kWave) {
                        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                        const int l = i | j;
                        const uint64_t a = sel[i], b = sel[l];
                        if ((a > b) == ((i & k) == 0)) {
                            sel[i] = b;
                            sel[l] = a;
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            for (int i = lane; i < kp; i += kWave) out[i] = i < found ? sel[i] : kInvalidCand;
            const uint64_t dmin = wave_min_cand<true>(lane < ngroups ? drops[lane] : kInvalidCand);
            if (lane == 0) out[kp] = dmin;
            return;
        }
        __syncthreads();  // (every thread has read the count: the tournament takes sel and drops over)
    }
    if (wave < ngroups) {
        const int l = wave * kWave + lane;
        const bool have = l < n_lists;
        const uint64_t *my = lists + (size_t)(have ? l : 0) * m;
        // (kInvalidCand is the largest value: lists that are not full drop out of the minimum by themselves)
        const uint64_t drop = wave_min_cand<false>(have ? my[m - 1] : kInvalidCand);
        uint64_t head = have ? my[0] : kInvalidCand;
        uint64_t next = have && m > 1 ? my[1] : kInvalidCand;
        int pos = 1;  // of `next`
        uint64_t *o = sel + (size_t)wave * kp;
        for (int r = 0; r < kp; r++) {
            const uint64_t w = wave_min_cand<false>(head);
            if (head == w && w != kInvalidCand) {  // entries are unique: exactly one lane advances
                head = next;
                pos++;
                next = pos < m ? my[pos] : kInvalidCand;
            }
            if (lane == 0) o[r] = w;
        }
        if (lane == 0) drops[wave] = drop;
    }
    __syncthreads();
    if (wave != 0) return;
    const uint64_t *my = sel + (size_t)(lane < ngroups ? lane : 0) * kp;
    uint64_t head = lane < ngroups ? my[0] : kInvalidCand;
    uint64_t next = lane < ngroups && kp > 1 ? my[1] : kInvalidCand;
    int pos = 1;
    uint64_t keep = kInvalidCand;  // lane i keeps output i (+64 per round of 64)
    for (int r = 0; r < kp; r++) {
        const uint64_t w = wave_min_cand<true>(head);
        if (head == w && w != kInvalidCand) {
            head = next;
            pos++;
            next = pos < kp ? my[pos] : kInvalidCand;
        }
        if ((r & 63) == lane) keep = w;
        if ((r & 63) == 63 || r == kp - 1) {
            const int idx = (r & ~63) + lane;
            if (idx <= r) out[idx] = keep;
            keep = kInvalidCand;
        }
    }
    const uint64_t drop = wave_min_cand<true>(lane < ngroups ? drops[lane] : kInvalidCand);
    if (lane == 0) out[kp] = drop;
}

// Rank merge (any kp): every entry finds its rank by binary searches in the
// other lists.  More work, fully parallel; used when kp is large.
__global__ __launch_bounds__(1024) void merge_kernel(const uint64_t *in, int n_lists, int kp,
                                                     int fan, uint64_t *out, int out_stride)
{
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);
    const int first = blockIdx.x * fan;
    const int mine = min(fan, n_lists - first);
    const int total = mine * kp;
    in += (size_t)blockIdx.y * n_lists * kp;     // blockIdx.y = query of the batch
    out += (size_t)blockIdx.y * (out_stride ? (size_t)out_stride : (size_t)gridDim.x * kp);
    for (int i = threadIdx.x; i < total; i += blockDim.x) lists[i] = in[(size_t)first * kp + i];
    uint64_t *o = out + (size_t)blockIdx.x * kp;
    for (int i = threadIdx.x; i < kp; i += blockDim.x) o[i] = kInvalidCand;
    __syncthreads();
    for (int it = threadIdx.x; it < total; it += blockDim.x) {
        const int w = it / kp;
        const int i = it - w * kp;
        const uint64_t c = lists[it];
        if (c == kInvalidCand) continue;
        int rank = i;
        for (int w2 = 0; w2 < mine; w2++) {
            if (w2 == w) continue;
            rank += lower_count(lists + (size_t)w2 * kp, kp, c);
            if (rank >= kp) break;
        }
        if (rank < kp) o[rank] = c;
    }
}

}  // namespace

hipError_t launch_scan(int qbits, int metric, const ScanArgs &a, int grid, int block, hipStream_t stream)
{
    static_assert(kEuclidean == 0 && kCosine == 1, "the scan objects are named by the metric's number");
    const bool cosine = metric == kCosine;
    switch (qbits) {
    case 4: return (cosine ? launch_scan_q4m1 : launch_scan_q4m0)(a, grid, block, stream);
    case 8: return (cosine ? launch_scan_q8m1 : launch_scan_q8m0)(a, grid, block, stream);
    case 16: return (cosine ? launch_scan_q16m1 : launch_scan_q16m0)(a, grid, block, stream);
    case 32: return (cosine ? launch_scan_q32m1 : launch_scan_q32m0)(a, grid, block, stream);
    case 64: return (cosine ? launch_scan_q64m1 : launch_scan_q64m0)(a, grid, block, stream);
    default: return hipErrorInvalidValue;
    }
}

// the matrix sweep's shared launch: scan_variant must name the shared form for exactly this launch
hipError_t launch_scan_share(int qbits, int metric, const ScanArgs &a, const ScanShareHi &hi, int grid, int block,
                             hipStream_t stream)
{
    if (qbits != 8 || (metric != kCosine && metric != kEuclidean) || a.collect || scan_masked(a)) return hipErrorInvalidValue;
    const ScanVariant v = scan_variant(scan_share_plan_in(qbits, a, hi, block));
    if (!v.matrix || !v.share) return hipErrorInvalidValue;
    const size_t lds = scan_lds_bytes(qbits, a.map, a.kp, block, v.group, a.planes, v.matrix_blocks());
    ScanShareArgs s;
    s.a = a;
    s.hi = hi;
    return (metric == kCosine ? launch_scan_mxs_m1 : launch_scan_mxs_m0)(s, v, grid, block, lds, stream);
}

// the matrix sweep's masked launch (option sketch_masked): scan_variant must name the masked form for exactly this launch
hipError_t launch_scan_masked(int qbits, int metric, const ScanArgs &a, const ScanShareHi &hi, int masked_opt, int grid, int block,
                              hipStream_t stream)
{
    if (qbits != 8 || (metric != kCosine && metric != kEuclidean) || a.collect || !scan_masked(a) || masked_opt != 1)
        return hipErrorInvalidValue;
    const ScanVariant v = scan_variant(scan_masked_plan_in(qbits, a, hi.share, masked_opt, block));
    if (!v.matrix || !v.masked) return hipErrorInvalidValue;
    const size_t lds = scan_lds_bytes(qbits, a.map, a.kp, block, v.group, a.planes, v.matrix_blocks());
    ScanMaskedArgs s;
    s.a = a;
    s.hi = hi;
    s.masked = masked_opt;
    if (v.share) return (metric == kCosine ? launch_scan_mxms_m1 : launch_scan_mxms_m0)(s, v, grid, block, lds, stream);
    return (metric == kCosine ? launch_scan_mxm_m1 : launch_scan_mxm_m0)(s, v, grid, block, lds, stream);
}

hipError_t launch_merge(const uint64_t *in, int n_lists, int kp, int n_queries, uint64_t *out,
                        hipStream_t stream, int out_stride)
{
    const int fan = merge_fan(kp);
    const dim3 grid((n_lists + fan - 1) / fan, n_queries);
    if (out_stride && (grid.x != 1 || out_stride < kp)) return hipErrorInvalidValue;  // (one output list per query only)
    const size_t lds = (size_t)fan * kp * sizeof(uint64_t);
    if (kp <= 128) {
        hipLaunchKernelGGL(merge_heads_kernel, grid, dim3(256), lds, stream, in, n_lists, kp, out, out_stride);
        return hipGetLastError();
    }
    int block = fan * kp;
    if (block > 1024) block = 1024;
    block = (block + 63) & ~63;
    hipLaunchKernelGGL(merge_kernel, grid, dim3(block), lds, stream, in, n_lists, kp, fan, out, out_stride);
    return hipGetLastError();
}

hipError_t launch_merge_short(const uint64_t *in, int n_lists, int m, int kp, int n_queries, uint64_t *out,
                              int out_stride, hipStream_t stream)
{
    if (!merge_short_fits(n_lists, m, kp) || out_stride < kp + 1) return hipErrorInvalidValue;
    const int block = (n_lists + kWave - 1) / kWave * kWave;  // one wave per group of 64 lists
    hipLaunchKernelGGL(merge_short_kernel, dim3(1, n_queries), dim3(block), merge_short_lds(n_lists, m, kp), stream,
                       in, n_lists, m, kp, out, out_stride);
    return hipGetLastError();
}

}  // namespace szg
