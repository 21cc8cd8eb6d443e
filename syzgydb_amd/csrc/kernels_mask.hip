// kernels_mask.hip -- device-resident filter masks (szg_mask, scan_mask.cpp): the words of ONE shard per launch.
//
// A shard's mask is `n_pairs` 16-byte pairs of words (its ceil(n_rows / 64) words rounded up to an even count); bits
// at positions >= n_rows -- the tail of the last word, the padding word -- are stored as 0.  Plain C++ and vector
// memory operations only.
#include "kernels.h"

namespace szg {

// One lane per listed row: rows are numbered as searches return them; those outside [first, first + n_rows) belong
// to another shard.  Duplicates and rows that share a word meet in the atomic OR.
__global__ __launch_bounds__(256) void mask_from_rows_kernel(const uint64_t *__restrict__ rows, uint64_t n_listed,
                                                             uint64_t first, uint64_t n_rows,
                                                             unsigned long long *__restrict__ words)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_listed) return;
    const uint64_t r = rows[i];
    if (r < first || r - first >= n_rows) return;
    const uint64_t l = r - first;
    atomicOr(&words[l >> 6], 1ull << (l & 63));
}

// the bits of word w that stand for rows < n_rows
__device__ __forceinline__ uint64_t valid_bits(uint64_t w, uint64_t n_rows)
{
    const uint64_t lo = w * 64;
    if (lo >= n_rows) return 0ull;
    const uint64_t left = n_rows - lo;
    return left >= 64 ? ~0ull : ((1ull << left) - 1ull);
}

// out = a op b over 16-byte pairs of words, the tail cleared; the block's popcount goes to *count in one atomic add.
// (out may be a: every lane reads its pair before it writes it.  b is null for SZG_MASK_NOT.)
__global__ __launch_bounds__(256) void mask_combine_kernel(int op, const ulonglong2 *a, const ulonglong2 *b,
                                                           ulonglong2 *out, uint64_t n_pairs, uint64_t n_rows,
                                                           unsigned long long *__restrict__ count)
{
    __shared__ unsigned int part[4];
    unsigned int ones = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += stride) {
        const ulonglong2 x = a[i];
        ulonglong2 y = make_ulonglong2(0ull, 0ull);
        if (b) y = b[i];
        ulonglong2 r;
        switch (op) {
        case 0: r.x = x.x & y.x, r.y = x.y & y.y; break;      // SZG_MASK_AND
        case 1: r.x = x.x | y.x, r.y = x.y | y.y; break;      // SZG_MASK_OR
        case 2: r.x = x.x & ~y.x, r.y = x.y & ~y.y; break;    // SZG_MASK_ANDNOT
        default: r.x = ~x.x, r.y = ~x.y; break;               // SZG_MASK_NOT
        }
        r.x &= valid_bits(2 * i, n_rows);
        r.y &= valid_bits(2 * i + 1, n_rows);
        out[i] = r;
        ones += (unsigned int)(__popcll(r.x) + __popcll(r.y));
    }
    for (int off = 32; off > 0; off >>= 1) ones += __shfl_down(ones, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ones;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = (unsigned long long)part[0] + part[1] + part[2] + part[3];
        if (sum) atomicAdd(count, sum);
    }
}

// Per-query slots of a batch from resident masks: slot q = the n_pairs pairs at dst + q * n_pairs, copied from
// t.src[q], or all ones where that is null (an unfiltered query).  grid.y = the batch's queries.
__global__ __launch_bounds__(256) void mask_gather_kernel(MaskGatherTable t, ulonglong2 *__restrict__ dst, uint64_t n_pairs)
{
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(t.src[blockIdx.y]);
    ulonglong2 *out = dst + (uint64_t)blockIdx.y * n_pairs;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += stride)
        out[i] = src ? src[i] : make_ulonglong2(~0ull, ~0ull);
}

// A mask carried across a compaction / reorder: new bit i = old bit list[i], i < n.  One thread per output word of
// the 2 * n_pairs; bits at positions >= n -- the tail of the last word, the padding word -- are stored as 0.
__global__ __launch_bounds__(256) void mask_gather_rows_kernel(const uint64_t *__restrict__ old_words,
                                                               const uint64_t *__restrict__ list, uint64_t n,
                                                               uint64_t *__restrict__ new_words, uint64_t n_words)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    uint64_t out = 0;
    const uint64_t lo = w * 64;
    const uint64_t hi = lo + 64 < n ? lo + 64 : n;
    for (uint64_t i = lo; i < hi; i++) {
        const uint64_t r = list[i];
        out |= ((old_words[r >> 6] >> (r & 63)) & 1ull) << (i - lo);
    }
    new_words[w] = out;
}

static unsigned blocks_for(uint64_t items, unsigned cap)
{
    const uint64_t g = (items + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

hipError_t launch_mask_from_rows(const uint64_t *rows, uint64_t n_listed, uint64_t first, uint64_t n_rows, uint64_t *words,
                                 hipStream_t stream)
{
    if (n_listed == 0 || n_rows == 0) return hipSuccess;
    const uint64_t grid = (n_listed + 255) / 256;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_from_rows_kernel, dim3((unsigned)grid), dim3(256), 0, stream, rows, n_listed, first, n_rows,
                       reinterpret_cast<unsigned long long *>(words));
    return hipGetLastError();
}

hipError_t launch_mask_combine(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n_pairs, uint64_t n_rows,
                               uint64_t *count, hipStream_t stream)
{
    if (n_pairs == 0) return hipSuccess;
    if (op < 0 || op > 3 || (op == 3) != (b == nullptr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_combine_kernel, dim3(blocks_for(n_pairs, 2048)), dim3(256), 0, stream, op,
                       reinterpret_cast<const ulonglong2 *>(a), reinterpret_cast<const ulonglong2 *>(b),
                       reinterpret_cast<ulonglong2 *>(out), n_pairs, n_rows, reinterpret_cast<unsigned long long *>(count));
    return hipGetLastError();
}

hipError_t launch_mask_gather(const MaskGatherTable &t, int n_queries, uint64_t *dst, uint64_t n_pairs, hipStream_t stream)
{
    if (n_pairs == 0 || n_queries <= 0) return hipSuccess;
    if (n_queries > kMqMaxQueries) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_gather_kernel, dim3(blocks_for(n_pairs, 256), (unsigned)n_queries), dim3(256), 0, stream, t,
                       reinterpret_cast<ulonglong2 *>(dst), n_pairs);
    return hipGetLastError();
}

hipError_t launch_mask_gather_rows(const uint64_t *old_words, const uint64_t *list, uint64_t n, uint64_t *new_words,
                                   uint64_t n_pairs, hipStream_t stream)
{
    if (n_pairs == 0) return hipSuccess;
    if (n > n_pairs * 128) return hipErrorInvalidValue;
    const uint64_t grid = (2 * n_pairs + 255) / 256;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_gather_rows_kernel, dim3((unsigned)grid), dim3(256), 0, stream, old_words, list, n, new_words,
                       2 * n_pairs);
    return hipGetLastError();
}

}  // namespace szg
