// kernels_mq.hip -- the selection kernels of the shared (multi-query) sweeps, the sizes of their LDS images and the
// two dispatchers into the sweep families (mq_device.h has the overview and the file list).
#include "mq_device.h"

#include <algorithm>
#include <cstdlib>

namespace szg {

namespace {

#ifndef SZG_RESCORE_BLOCKS
#define SZG_RESCORE_BLOCKS 64  // blocks (of 4 waves) per query of the float32 re-score
#endif

// ---- per-query selection over the score matrix ----------------------------------

// grid (blocks per query, queries).  Each lane reads 4 keys at a time (16 bytes);
// a key that beats the wave's current kp-th best is inserted into the wave's list.
__global__ __launch_bounds__(1024) void mq_select_kernel(const float *keys, size_t key_stride,
                                                        uint32_t n_rows, const uint64_t *live_bits,
                                                        const uint64_t *allow_bits,
                                                        uint32_t allow_stride, int kp,
                                                        uint64_t *block_lists, float *thr_out,
                                                        uint32_t *count_zero)
{
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t *lists = reinterpret_cast<uint64_t *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int q = blockIdx.y;
    WaveList wl;
    wl.init(lists + (size_t)wave * kp, kp, lane);
    __syncthreads();
    const float *kq = keys + (size_t)q * key_stride;
    const uint64_t *allow = allow_bits ? allow_bits + (size_t)q * allow_stride : nullptr;
    const uint32_t n4 = (n_rows + 3) / 4;  // key_stride is a multiple of 4, the tail holds +inf
    const uint32_t stride = gridDim.x * blockDim.x;
    constexpr int U = 4;  // loads in flight per thread (one block per query walks its keys: latency-bound)
    for (uint32_t i0 = blockIdx.x * blockDim.x + tid; i0 < ((n4 + stride - 1) / stride) * stride; i0 += U * stride) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = i0 + u * stride;
            v[u] = make_float4(3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f);
            if (i < n4) v[u] = reinterpret_cast<const float4 *>(kq)[i];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = i0 + u * stride;
            if (i >= ((n4 + stride - 1) / stride) * stride) break;  // (uniform over the block)
            const float kk[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t row = i * 4 + e;
                bool ok = i < n4 && row < n_rows;
                if (ok && live_bits) ok = (live_bits[row >> 6] >> (row & 63)) & 1;
                if (ok && allow) ok = (allow[row >> 6] >> (row & 63)) & 1;
                const uint64_t cnd = ((uint64_t)ordered_key(kk[e]) << 32) | row;
                wl.offer(ok, cnd, lane);
            }
        }
    }
    wl.flush(lane);
    __syncthreads();
    uint64_t *out = block_lists + ((size_t)q * gridDim.x + blockIdx.x) * kp;
    block_merge_lists(lists, nwaves, kp, out, tid, blockDim.x);
    if (thr_out) {  // one block per query: its kp-th key is the query's collect threshold
        __syncthreads();
        if (tid == 0) {
            const uint64_t c = out[kp - 1];
            thr_out[q] = c == kInvalidCand ? 3.0e38f : key_from_ordered((uint32_t)(c >> 32));
            count_zero[q * kCandCountStride] = 0;
        }
    }
}

// one block per query: the kp best of the query's candidate buffer, sorted ascending
__global__ __launch_bounds__(256) void cand_select_kernel(const uint64_t *cand_buf, const uint32_t *cand_count,
                                                          uint32_t cand_cap, int kp, uint64_t *lists)
{
    extern __shared__ __align__(16) uint8_t smem[];
    uint64_t *wl_lds = reinterpret_cast<uint64_t *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int q = blockIdx.x;
    WaveList wl;
    wl.init(wl_lds + (size_t)wave * kp, kp, lane);
    __syncthreads();
    const uint32_t n = min(cand_count[q * kCandCountStride], cand_cap);
    const uint64_t *src = cand_buf + (size_t)q * cand_cap;
    for (uint32_t i = tid; i < ((n + blockDim.x - 1) / blockDim.x) * blockDim.x; i += blockDim.x) {
        const bool ok = i < n;
        const uint64_t c = ok ? src[i] : kInvalidCand;
        wl.offer(ok, c, lane);
    }
    wl.flush(lane);
    __syncthreads();
    block_merge_lists(wl_lds, nwaves, kp, lists + (size_t)q * kp, tid, blockDim.x);
}


// Second stage of the bfloat16 sweep: the (few thousand) candidates it collected are scored again in
// float32 -- one wave per (query, candidate), the query as float32 in LDS -- and the key inside the
// candidate word is replaced, so that the selection and the certification that follow work with
// float32 keys (bound: key_eps, mq branch).  grid (blocks, queries); 32-bit rows, any dim.
// One 16-byte piece of a 32- or 16-bit row against the float32 query staged in LDS: 4 floats, or 8 codes decoded to
// n = 2v - 65535.  COS: dot, norm and the zero-row bits; else the squared difference (into dot).
template <bool COS>
__device__ __forceinline__ void rescore_use(const uint4 w, const float *qf, int piece, int row_bits, int dim,
                                            float &dot, float &nrm, uint32_t &nz)
{
    if (row_bits == 8) {  // sixteen codes, n = 2v - 255 (exact); the last piece's padding codes are not part of the row
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
        const int n8 = min(16, dim - piece * 16);
        const float *y8 = qf + (size_t)piece * 16;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (i < n8) {
                const float xv = fmaf((float)((ww[i >> 2] >> (8 * (i & 3))) & 0xFFu), 2.0f, -255.0f);
                if (COS) {
                    dot = fmaf(xv, y8[i], dot);
                    nrm = fmaf(xv, xv, nrm);
                } else {
                    const float d = xv - y8[i];
                    dot = fmaf(d, d, dot);
                }
            }
        }
        nz |= 1u;
        return;
    }
    float x[8];
    int n;
    if (row_bits == 16) {
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[2 * i] = fmaf((float)(ww[i] & 0xFFFFu), 2.0f, -65535.0f);
            x[2 * i + 1] = fmaf((float)(ww[i] >> 16), 2.0f, -65535.0f);
        }
        n = min(8, dim - piece * 8);  // (the last piece's padding codes decode to -65535: not part of the row)
        nz |= 1u;
    } else if (row_bits == 64) {  // two float64 elements, narrowed to float32 as the sweep narrows them
        x[0] = (float)__hiloint2double((int)w.y, (int)w.x);
        x[1] = (float)__hiloint2double((int)w.w, (int)w.z);
        x[2] = x[3] = x[4] = x[5] = x[6] = x[7] = 0.f;
        n = 2;
        nz |= ((w.y | w.w) & 0x7FFFFFFFu) | w.x | w.z;
    } else {
        x[0] = __uint_as_float(w.x); x[1] = __uint_as_float(w.y); x[2] = __uint_as_float(w.z); x[3] = __uint_as_float(w.w);
        x[4] = x[5] = x[6] = x[7] = 0.f;
        n = 4;
        nz |= (w.x | w.y | w.z | w.w) & 0x7FFFFFFFu;
    }
    const float *y = qf + (size_t)piece * (row_bits == 16 ? 8 : (row_bits == 64 ? 2 : 4));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (i < n) {
            if (COS) {
                dot = fmaf(x[i], y[i], dot);
                nrm = fmaf(x[i], x[i], nrm);
            } else {
                const float d = x[i] - y[i];
                dot = fmaf(d, d, dot);
            }
        }
    }
}
__device__ __forceinline__ int rescore_epp(int row_bits)  // elements per 16-byte piece
{
    return row_bits == 8 ? 16 : (row_bits == 16 ? 8 : (row_bits == 64 ? 2 : 4));
}
template <bool COS>
__device__ __forceinline__ void rescore_piece(const uint8_t *rows, const RowLayout &lay, uint32_t row, const float *qf, int piece,
                                              int row_bits, int dim, float &dot, float &nrm, uint32_t &nz)
{
    rescore_use<COS>(*reinterpret_cast<const uint4 *>(rows + piece_offset(lay, row, (uint32_t)piece)), qf, piece, row_bits, dim,
                     dot, nrm, nz);
}

template <int METRIC>
__global__ __launch_bounds__(256) void cand_rescore_kernel(const uint8_t *rows, RowLayout lay, int dim,
                                                           const double *q64, const double *qscale,
                                                           uint64_t *cand_buf, const uint32_t *cand_count,
                                                           uint32_t cand_cap, int row_bits)
{
    extern __shared__ __align__(16) uint8_t smem[];
    float *qf = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.y;
    const uint32_t n = min(cand_count[q * kCandCountStride], cand_cap);
    const double sc = qscale[q];
    // whole 16-byte pieces: a 32-bit row's padding is stored as zeros, the query's staged as zeros (16-bit rows come
    // here with whole pieces only)
    const int epp = rescore_epp(row_bits), pieces = (dim + epp - 1) / epp;
    for (int i = tid; i < epp * pieces; i += blockDim.x) qf[i] = i < dim ? (float)(q64[(size_t)q * dim + i] * sc) : 0.0f;
    __syncthreads();
    uint64_t *cb = cand_buf + (size_t)q * cand_cap;
    for (uint32_t ci = blockIdx.x * 4 + wave; ci < n; ci += gridDim.x * 4) {
        const uint32_t row = (uint32_t)cb[ci];
        float dot = 0.f, nrm = 0.f;
        uint32_t nz = 0;
        for (int i = lane; i < pieces; i += 64) rescore_piece<METRIC == kCosine>(rows, lay, row, qf, i, row_bits, dim, dot, nrm, nz);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            dot += __shfl_xor(dot, o);
            if (METRIC == kCosine) {
                nrm += __shfl_xor(nrm, o);
                nz |= __shfl_xor(nz, o);
            }
        }
        float key;
        if (METRIC == kCosine) {
            key = -dot * __frsqrt_rn(nrm);
            if (nrm == 0.f) key = nz ? -2.0f : 1.0f;
            if (!(nrm <= 3.0e38f)) key = -2.0f;  // norm overflow: forced in (see RowAcc::finish)
        } else {
            key = dot;
        }
        if (!(key == key)) key = 3.0e38f;
        if (key > 3.0e38f) key = 3.0e38f;
        if (lane == 0) cb[ci] = ((uint64_t)ordered_key(key) << 32) | row;
    }
}


// ---- thresholds of the fused selection: a radix select, not a sort ----------------------------------------------------
//
// The threshold pass only needs ONE number per query: a key thr such that at least kp eligible prefix rows have
// key <= thr, as small as cheaply possible.  Two histogram rounds over the ordered key's top 12 + 12 bits (LDS
// atomics, one block of 1024 threads per query) give the kp-th smallest key to 2^-16 relative -- rounded UP, so the
// kp-th key itself always passes.  The sorted-list selection this replaces (mq_select_kernel, one block per query)
// spent ~50 us per 96-query batch inserting into lists nobody read.
__global__ __launch_bounds__(1024) void mq_thr_radix_kernel(const float *keys, size_t key_stride, uint32_t n_rows,
                                                            const uint64_t *live_bits, const uint64_t *allow_bits,
                                                            uint32_t allow_stride, int kp, float *thr_out,
                                                            uint32_t *count_zero)
{
    __shared__ uint32_t hist[4096];
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t sel_bin, sel_below;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const float4 *kq = reinterpret_cast<const float4 *>(keys + (size_t)q * key_stride);
    const uint64_t *allow = allow_bits ? allow_bits + (size_t)q * allow_stride : nullptr;
    const uint32_t n4 = (n_rows + 3) / 4;  // key_stride is a multiple of 4
    uint32_t prefix_bits = 0;              // the bins chosen so far (top bits of the ordered key)
    uint32_t below = 0;                    // eligible keys below the chosen bins
    for (int round = 0; round < 2; round++) {
        for (int i = tid; i < 4096; i += 1024) hist[i] = 0;
        __syncthreads();
        const int shift = round == 0 ? 20 : 8;
        for (uint32_t i = tid; i < n4; i += 1024) {
            const float4 v = kq[i];
            const float kk[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t row = i * 4 + e;
                bool ok = row < n_rows;
                if (ok && live_bits) ok = (live_bits[row >> 6] >> (row & 63)) & 1;
                if (ok && allow) ok = (allow[row >> 6] >> (row & 63)) & 1;
                const uint32_t u = ordered_key(kk[e]);
                if (ok && (round == 0 || (u >> 20) == prefix_bits)) atomicAdd(&hist[(u >> shift) & 0xFFFu], 1u);
            }
        }
        __syncthreads();
        // the bin where the running count reaches kp: 4 bins per thread, scan over the wave, then over the 16 waves
        const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
        const uint32_t mine = h0 + h1 + h2 + h3;
        uint32_t incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wave] = incl;
        if (tid == 0) sel_bin = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t before = below;
        for (int w = 0; w < wave; w++) before += wsum[w];
        const uint32_t excl = before + incl - mine;  // eligible keys before this thread's 4 bins (chosen bins included)
        if (excl < (uint32_t)kp && excl + mine >= (uint32_t)kp) {  // exactly one thread
            uint32_t acc = excl;
            const uint32_t hh[4] = {h0, h1, h2, h3};
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (acc < (uint32_t)kp && acc + hh[b] >= (uint32_t)kp) {
                    sel_bin = 4 * tid + b;
                    sel_below = acc;
                }
                acc += hh[b];
            }
        }
        __syncthreads();
        if (sel_bin == 0xFFFFFFFFu) break;  // fewer than kp eligible keys: everything passes
        prefix_bits = round == 0 ? sel_bin : ((prefix_bits << 12) | sel_bin);
        below = sel_below;
        __syncthreads();
    }
    if (tid == 0) {
        float thr = 3.0e38f;
        if (sel_bin != 0xFFFFFFFFu) {
            thr = key_from_ordered((prefix_bits << 8) | 0xFFu);  // the top of the chosen 24-bit bin
            if (!(thr <= 3.0e38f)) thr = 3.0e38f;                // (NaN patterns sort last: keys are clamped anyway)
        }
        thr_out[q] = thr;
        count_zero[q * kCandCountStride] = 0;
    }
}

// ---- the tail of a fused-selection batch in ONE launch ---------------------------------------------------------------
//
// One block of 1024 threads per query, the query's collected candidates (<= kRefineMaxCands) in LDS:
//   1. the kp best by the sweep's key (per-wave lists + block rank-merge, as everywhere);
//   2. MODE > 0, bfloat16 sweeps: the sweep's key b of a candidate is within eps_b of its real-number key, so only
//      candidates with b <= t_kp + W (t_kp = the kp-th best sweep key, W = 2 eps_b) can be among the kp best by a
//      better key.  Those -- a few dozen of the ~1 000 collected -- are scored again in float32 (one wave per
//      candidate, the float32 query in LDS) and the kp best of THEM by float32 key are the list; the band's edge
//      E = t_kp + W goes to the host: every collected candidate outside the band has sweep key > E, which
//      certification needs (scan_topk.cpp: gather_topk).  Re-scoring every candidate, as the first form of this
//      stage did, cost 64 us per 96-query batch; the band costs a tenth.
//   3. the query's sentinel rows (its first k eligible rows in visit order, whatever their key: DESIGN.md 2) are
//      appended behind the list, so ONE rerank launch computes the float64 distances of both.
// MODE 0: selection only (int8 / float32 sweeps: the collected keys are final).  1: cosine band, 2: euclid band.
// A band that does not fit kRefineMaxBand (duplicate-heavy corpora) reports overflow through the hit counter, which
// sends the batch down the score-matrix path like an overflowing candidate buffer.
constexpr int kRefineThreads = 1024;
constexpr int kRefineMaxCands = 8192;
constexpr int kRefineMaxBand = 1024;
constexpr int kRefineMaxKp = 256;

template <int MODE>
__global__ __launch_bounds__(kRefineThreads) void cand_refine_kernel(const uint8_t *rows, RowLayout lay, int dim,
                                                                     const double *q64, const double *qscale,
                                                                     const double *qnorm2, const uint64_t *cand_buf,
                                                                     uint32_t *cand_count, uint32_t cand_cap, int kp,
                                                                     const uint64_t *sent, int n_sent, uint64_t *lists,
                                                                     float *band_edge, int row_bits)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int NW = kRefineThreads / 64;
    const int q = blockIdx.x;
    const uint32_t n = min(cand_count[q * kCandCountStride], cand_cap);
    uint64_t *cand = reinterpret_cast<uint64_t *>(smem);                  // [kRefineMaxCands]
    uint64_t *wl_lds = cand + kRefineMaxCands;                            // [NW][kp]
    uint64_t *top = wl_lds + (size_t)NW * kp;                             // [kp]
    uint64_t *band = top + kp;                                            // [kRefineMaxBand]
    float *qf = reinterpret_cast<float *>(band + kRefineMaxBand);         // [dim] (MODE > 0)
    __shared__ uint32_t n_band;
    const uint64_t *src = cand_buf + (size_t)q * cand_cap;
    uint64_t *out = lists + (size_t)q * (kp + n_sent);

    for (uint32_t i = tid; i < n; i += kRefineThreads) cand[i] = src[i];
    if (MODE > 0) {
        const double sc = qscale[q];
        const int epp0 = rescore_epp(row_bits);
        for (int i = tid; i < epp0 * ((dim + epp0 - 1) / epp0); i += kRefineThreads)
            qf[i] = i < dim ? (float)(q64[(size_t)q * dim + i] * sc) : 0.0f;  // (padding: zeros, as in the rows)
    }
    if (tid == 0) n_band = 0;
    float edge = 3.0e38f;  // fewer than kp candidates: everything collected is in the band
    if (MODE == 0) {
        WaveList wl;
        wl.init(wl_lds + (size_t)wave * kp, kp, lane);
        __syncthreads();
        for (uint32_t i = tid; i < ((n + kRefineThreads - 1) / kRefineThreads) * kRefineThreads; i += kRefineThreads) {
            const bool ok = i < n;
            wl.offer(ok, ok ? cand[i] : kInvalidCand, lane);
        }
        wl.flush(lane);
        __syncthreads();
        block_merge_lists(wl_lds, NW, kp, out, tid, kRefineThreads);
        for (int i = tid; i < n_sent; i += kRefineThreads) out[kp + i] = sent[(size_t)q * n_sent + i];
        return;
    }
    for (int i = tid; i < n_sent; i += kRefineThreads) out[kp + i] = sent[(size_t)q * n_sent + i];
    // The band needs ONE number of the sweep's keys: the kp-th smallest, t_kp (any value at or above it serves: the band
    // only grows).  Two histogram rounds over the ordered key's top 12 + 12 bits (as mq_thr_radix_kernel) instead of
    // round 3's sixteen sorted per-wave lists and their rank merge, which nothing else read: 60 -> ~30 us per batch.
    {
        uint32_t *hist = reinterpret_cast<uint32_t *>(qf + ((dim + 15) & ~15));  // [4096]
        __shared__ uint32_t wsum[NW];
        __shared__ uint32_t sel_bin, sel_below;
        uint32_t prefix_bits = 0, below = 0;
        bool found = n >= (uint32_t)kp;
        for (int round = 0; round < 2 && found; round++) {
            for (int i = tid; i < 4096; i += kRefineThreads) hist[i] = 0;
            __syncthreads();
            const int shift = round == 0 ? 20 : 8;
            for (uint32_t i = tid; i < n; i += kRefineThreads) {
                const uint32_t u = (uint32_t)(cand[i] >> 32);
                if (round == 0 || (u >> 20) == prefix_bits) atomicAdd(&hist[(u >> shift) & 0xFFFu], 1u);
            }
            __syncthreads();
            const uint32_t h0 = hist[4 * tid], h1 = hist[4 * tid + 1], h2 = hist[4 * tid + 2], h3 = hist[4 * tid + 3];
            const uint32_t mine = h0 + h1 + h2 + h3;
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            if (lane == 63) wsum[wave] = incl;
            if (tid == 0) sel_bin = 0xFFFFFFFFu;
            __syncthreads();
            uint32_t before = below;
            for (int w = 0; w < wave; w++) before += wsum[w];
            const uint32_t excl = before + incl - mine;
            if (excl < (uint32_t)kp && excl + mine >= (uint32_t)kp) {  // exactly one thread
                uint32_t acc = excl;
                const uint32_t hh[4] = {h0, h1, h2, h3};
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    if (acc < (uint32_t)kp && acc + hh[b] >= (uint32_t)kp) {
                        sel_bin = 4 * tid + b;
                        sel_below = acc;
                    }
                    acc += hh[b];
                }
            }
            __syncthreads();
            if (sel_bin == 0xFFFFFFFFu) {
                found = false;  // (cannot happen with n >= kp; uniform over the block)
            } else {
                prefix_bits = round == 0 ? sel_bin : ((prefix_bits << 12) | sel_bin);
                below = sel_below;
            }
            __syncthreads();
        }
        if (found) {
            float t = key_from_ordered((prefix_bits << 8) | 0xFFu);  // the top of the kp-th key's 24-bit bin
            if (!(t <= 3.0e38f)) t = 3.0e38f;
            const float c = 1.01f * 0x1p-7f, nu = ((float)dim + (row_bits == 64 ? 20.0f : 16.0f)) * 0x1p-24f;  // key_eps (scan_query.cpp), bfloat16 branch
            float eps;
            if (MODE == 1) {
                eps = c + 4.0f * nu + 1e-6f;
            } else {  // key_eps (scan_query.cpp), bfloat16 euclid branch
                const float qn = sqrtf((float)qnorm2[q]), rt = sqrtf(fmaxf(t, 0.0f));
                const float s2 = 2.0f * qn + rt;
                eps = 2.0f * c * qn * (1.1f * qn + rt) + c * c * qn * qn + 3.0f * nu * s2 * s2;
            }
            edge = t + 2.02f * eps;
            if (!(edge < 3.0e38f)) edge = 3.0e38f;
        }
    }
    const uint32_t uedge = ordered_key(edge);
    for (uint32_t i = tid; i < n; i += kRefineThreads) {
        if ((uint32_t)(cand[i] >> 32) <= uedge) {
            const uint32_t at = atomicAdd(&n_band, 1u);
            if (at < (uint32_t)kRefineMaxBand) band[at] = cand[i];
        }
    }
    __syncthreads();
    const uint32_t nb = n_band;
    if (nb > (uint32_t)kRefineMaxBand) {  // (uniform over the block)
        if (tid == 0) cand_count[q * kCandCountStride] = 0xFFFFFFFFu;  // the host redoes the batch (score matrix)
        for (int i = tid; i < kp; i += kRefineThreads) out[i] = kInvalidCand;
        return;
    }
    // float32 keys for the band: one wave per candidate, four candidates' row gathers in flight per wave (the rows were
    // streamed past the caches by the sweep: every gather is a full HBM round trip, and a wave that walked its ~7
    // candidates one after the other paid seven of them in a row)
    const int epp = rescore_epp(row_bits), pieces = (dim + epp - 1) / epp;
    constexpr int U = 4;
    for (uint32_t c0 = (uint32_t)wave * U; c0 < nb; c0 += NW * U) {
        uint32_t rowv[U];
        float dot[U], nrm[U];
        uint32_t nz[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            rowv[u] = (uint32_t)band[min(c0 + u, nb - 1)];  // (past the band's end: the last candidate again, not written)
            dot[u] = nrm[u] = 0.f;
            nz[u] = 0;
        }
        // ALL the loads of a trip first (4 candidates x up to 4 pieces per lane: a 768-dim float32 row is 3), then the
        // arithmetic: the form that used each piece as it came paid one HBM round trip per 64 pieces of a row --
        // 12.5 us per trip, 25-50 us of the kernel's 33-60
        constexpr int PI = 4;
        for (int i0 = lane; i0 < pieces; i0 += 64 * PI) {
            uint4 w[U][PI];
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int pi = 0; pi < PI; pi++)
                    w[u][pi] = *reinterpret_cast<const uint4 *>(rows + piece_offset(lay, rowv[u], (uint32_t)min(i0 + 64 * pi, pieces - 1)));
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int pi = 0; pi < PI; pi++)
                    if (i0 + 64 * pi < pieces)
                        rescore_use<MODE == 1>(w[u][pi], qf, i0 + 64 * pi, row_bits, dim, dot[u], nrm[u], nz[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                dot[u] += __shfl_xor(dot[u], o);
                if (MODE == 1) {
                    nrm[u] += __shfl_xor(nrm[u], o);
                    nz[u] |= __shfl_xor(nz[u], o);
                }
            }
            float key;
            if (MODE == 1) {  // exactly cand_rescore_kernel's key (the certification bound is the float32 sweeps')
                key = -dot[u] * __frsqrt_rn(nrm[u]);
                if (nrm[u] == 0.f) key = nz[u] ? -2.0f : 1.0f;
                if (!(nrm[u] <= 3.0e38f)) key = -2.0f;  // norm overflow: forced in (see RowAcc::finish)
            } else {
                key = dot[u];
            }
            if (!(key == key)) key = 3.0e38f;
            if (key > 3.0e38f) key = 3.0e38f;
            if (lane == 0 && c0 + u < nb) band[c0 + u] = ((uint64_t)ordered_key(key) << 32) | rowv[u];
        }
    }
    __syncthreads();
    // the kp best of the band by float32 key: rank by counting (entries are unique: the row is part of the word)
    for (int i = tid; i < kp; i += kRefineThreads) out[i] = kInvalidCand;
    __syncthreads();
    for (uint32_t i = tid; i < nb; i += kRefineThreads) {
        const uint64_t mine = band[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nb; j++) rank += band[j] < mine ? 1u : 0u;
        if (rank < (uint32_t)kp) out[rank] = mine;
    }
    if (tid == 0) band_edge[q] = edge;
}

}  // namespace

hipError_t launch_cand_select(const uint64_t *cand_buf, const uint32_t *cand_count, uint32_t cand_cap,
                              int kp, int n_queries, uint64_t *lists, hipStream_t stream)
{
    const size_t lds = (size_t)4 * kp * sizeof(uint64_t);
    hipLaunchKernelGGL(cand_select_kernel, dim3(n_queries), dim3(256), lds, stream, cand_buf, cand_count,
                       cand_cap, kp, lists);
    return hipGetLastError();
}

hipError_t launch_cand_rescore(int metric, const uint8_t *rows, RowLayout lay, int dim, const double *q64,
                               const double *qscale, uint64_t *cand_buf, const uint32_t *cand_count,
                               uint32_t cand_cap, int n_queries, int row_bits, hipStream_t stream)
{
    if (row_bits != 32 && row_bits != 16 && row_bits != 64 && row_bits != 8) return hipErrorInvalidValue;
    const dim3 grid(SZG_RESCORE_BLOCKS, n_queries);  // x 4 waves: one candidate per wave and trip
    const size_t lds = (size_t)((dim + 15) & ~15) * sizeof(float);
    if (metric == kCosine)
        hipLaunchKernelGGL(cand_rescore_kernel<kCosine>, grid, dim3(256), lds, stream, rows, lay, dim, q64, qscale,
                           cand_buf, cand_count, cand_cap, row_bits);
    else
        hipLaunchKernelGGL(cand_rescore_kernel<kEuclidean>, grid, dim3(256), lds, stream, rows, lay, dim, q64,
                           qscale, cand_buf, cand_count, cand_cap, row_bits);
    return hipGetLastError();
}

bool cand_refine_applies(int kp, uint32_t cand_cap, int dim, bool rescore)
{
    return kp <= kRefineMaxKp && cand_cap <= (uint32_t)kRefineMaxCands && (!rescore || dim <= 4096);
}

hipError_t launch_cand_refine(int mode, const uint8_t *rows, RowLayout lay, int dim, const double *q64,
                              const double *qscale, const double *qnorm2, const uint64_t *cand_buf, uint32_t *cand_count,
                              uint32_t cand_cap, int kp, int n_queries, const uint64_t *sent, int n_sent,
                              uint64_t *lists, float *band_edge, int row_bits, hipStream_t stream)
{
    if (!cand_refine_applies(kp, cand_cap, dim, mode > 0)) return hipErrorInvalidValue;
    if (mode > 0 && row_bits != 32 && row_bits != 16 && row_bits != 64 && row_bits != 8) return hipErrorInvalidValue;
    const size_t lds = ((size_t)kRefineMaxCands + (size_t)(kRefineThreads / 64) * kp + kp + kRefineMaxBand) * sizeof(uint64_t) +
                       (mode > 0 ? (size_t)((dim + 15) & ~15) * sizeof(float) + 4096 * sizeof(uint32_t) : 0);
    auto go = [&](auto kern) {
        return launch_lds(kern, n_queries, kRefineThreads, lds, stream, rows, lay, dim, q64, qscale, qnorm2, cand_buf, cand_count,
                          cand_cap, kp, sent, n_sent, lists, band_edge, row_bits);
    };
    if (mode == 0) return go(&cand_refine_kernel<0>);
    if (mode == 1) return go(&cand_refine_kernel<1>);
    return go(&cand_refine_kernel<2>);
}

size_t mq_i8_image_bytes(int row_bits, int r16, int nb)
{
    return (size_t)((r16 + 3) / 4) * kMqPlanes * (row_bits == 4 ? 2 : 1) * nb * 1024;
}
size_t mq_i8_lds_bytes(int row_bits, int r16, int nb, int groups)
{   // per group: image + constants + thresholds; + the 12 waves' hit buffers
    return (size_t)groups * (mq_i8_image_bytes(row_bits, r16, nb) + kMq8TableRows * 48 * sizeof(float)) + (size_t)SZG_MQ8_WAVES * 64 * 9;
}
size_t mq_bf16_image_bytes(int row_bits, int r16, int nb)
{   // a KiB per 32-element K-step and query block; a 128-byte step of a row holds one (32-bit rows), two (16-bit) or
    // half a one (64-bit)
    if (row_bits == 8) return (size_t)((r16 + 3) / 4) * 2 * nb * 1024;  // (tiled rows: two K-steps per 64-byte step)
    const size_t steps = (size_t)((r16 + 7) / 8);
    return (row_bits == 64 ? (steps + 1) / 2 : steps * (row_bits == 16 ? 2 : 1)) * nb * 1024;
}
size_t mq_bf16_lds_bytes(int row_bits, int r16, int nb)
{   // + thresholds, |q|^2 table and the waves' hit buffers
    // (16-bit rows -- the direct kernel -- run 12 waves without a staging KiB; the staged kernels 8 with one each)
    return mq_bf16_image_bytes(row_bits, r16, nb) + 3 * kMqMaxQueries * sizeof(float) +  // (the third table: 8-bit rows' sum g)
           std::max((size_t)SZG_MQB_WAVES * (kHitCap * 9 + 1024), (size_t)12 * kHitCap * 9);
}
hipError_t launch_mq_score_bf16(int row_bits, const MqArgs &a, int nb, int grid, hipStream_t stream)
{
    const size_t lds = mq_bf16_lds_bytes(row_bits, a.r16, nb);
    if (row_bits == 32) return launch_mq_bf16s_rows<32>(a, nb, grid, lds, stream);
    if (row_bits == 16) {
        static const bool staged16 = getenv("SZG_BF16_STAGED16") != nullptr;  // (A/B: the LDS-staged form for 16-bit rows)
        // (no resident norms -- an allocation failed, SZG_NO_ROW_NORMS: the staged form sums its own)
        if (!staged16 && a.row_norm) return launch_mq_bf16d_rows<16>(a, nb, grid, lds, stream);
        return launch_mq_bf16s_rows<16>(a, nb, grid, lds, stream);
    }
    if (row_bits == 64) return launch_mq_bf16s_rows<64>(a, nb, grid, lds, stream);
    if (row_bits == 8) return launch_mq_bf16d_rows<8>(a, nb, grid, lds, stream);
    return hipErrorInvalidValue;
}
hipError_t launch_mq_score_i8(int row_bits, const MqArgs &a, int nb, int grid, hipStream_t stream)
{
    const size_t lds = mq_i8_lds_bytes(row_bits, a.r16, nb, a.n_groups > 0 ? a.n_groups : 1);
    if (row_bits == 8) return launch_mq_i8_rows<8>(a, nb, grid, lds, stream);
    if (row_bits == 4) return launch_mq_i8_rows<4>(a, nb, grid, lds, stream);
    return hipErrorInvalidValue;
}

hipError_t launch_mq_select(const float *keys, size_t key_stride, uint32_t n_rows,
                            const uint64_t *live_bits, const uint64_t *allow_bits,
                            uint32_t allow_stride, int kp, int n_queries, int blocks_per_query,
                            uint64_t *block_lists, hipStream_t stream, float *thr_out, uint32_t *count_zero)
{
    if (thr_out && blocks_per_query != 1) return hipErrorInvalidValue;
    if (thr_out && kp >= 1) {  // the threshold pass: radix select (no lists)
        hipLaunchKernelGGL(mq_thr_radix_kernel, dim3(n_queries), dim3(1024), 0, stream, keys, key_stride, n_rows,
                           live_bits, allow_bits, allow_stride, kp, thr_out, count_zero);
        return hipGetLastError();
    }
    // the threshold pass walks a query's prefix keys with ONE block (it publishes the threshold): latency-bound, so
    // it gets 16 waves instead of 4 when their lists fit (50 -> ~15 us for a 96-query batch)
    const int threads = thr_out && (size_t)16 * kp * sizeof(uint64_t) <= 48u * 1024u ? 1024 : 256;
    const size_t lds = (size_t)(threads / 64) * kp * sizeof(uint64_t);
    hipLaunchKernelGGL(mq_select_kernel, dim3(blocks_per_query, n_queries), dim3(threads), lds, stream, keys,
                       key_stride, n_rows, live_bits, allow_bits, allow_stride, kp, block_lists, thr_out,
                       count_zero);
    return hipGetLastError();
}

}  // namespace szg
