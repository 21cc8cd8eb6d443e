// kernels_column_carry.hip -- resident metadata columns carried across a compaction / reorder (scan_column_carry.cpp):
// ONE part of a column per launch.  New row i takes what old row list[i] held.
//
//   values      out[at[i]] = values[list[i]], 8- and 4-byte elements, one lane per element (at null: out[i], the
//               stores then coalesced; list null: values[i], the placement of a dense stage by at[])
//   text heap   the references are gathered by the list; an exclusive prefix sum of their lengths gives every row's
//               64-bit start among the carried bytes -- three plain launches (the sum of each block of 256 rows, ONE
//               wave that scans the block sums 64 at a time over any count, the add): no block ever waits for another
//               one; the bytes then move one lane per 16-byte piece of the NEW bytes (column_carry.h: a binary search
//               over the starts, aligned dword fetches of the old heap, funnel shifts, one 16-byte store), so the
//               stores are coalesced and a long value costs no more per byte than a short one
//
// The present bits go through kernels_mask.hip's launch_mask_gather_rows.  Plain C++ and vector memory operations only.
#include "kernels.h"
#include "column_carry.h"

namespace szg {

namespace {

constexpr unsigned kBlock = 256;   // threads of every block here, and the rows whose lengths one block sums

template <typename T>
__global__ __launch_bounds__(256) void carry_gather_kernel(const T *__restrict__ values, const uint64_t *__restrict__ list,
                                                           const uint64_t *__restrict__ at, T *__restrict__ out, uint64_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[at ? at[i] : i] = values[list ? list[i] : i];
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, unsigned delta)
{
    const unsigned lo = __shfl_up((unsigned)v, delta), hi = __shfl_up((unsigned)(v >> 32), delta);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int lane)
{
    const unsigned lo = __shfl((unsigned)v, lane), hi = __shfl((unsigned)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// the inclusive prefix sum over the 64 lanes of a wave (every lane of the wave takes part)
__device__ __forceinline__ uint64_t wave_inclusive(uint64_t v, unsigned lane)
{
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) {
        const uint64_t t = shfl_up64(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// refs_out[i] = refs[list[i]] (list null: refs[i]); sums[b] = the lengths of block b's 256 rows added up
__global__ __launch_bounds__(256) void carry_ref_sums_kernel(const uint64_t *__restrict__ refs,
                                                             const uint64_t *__restrict__ list, uint64_t n,
                                                             uint64_t *__restrict__ refs_out, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t part[4];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned lane = threadIdx.x & 63;
    uint64_t ref = 0;
    if (i < n) {
        ref = refs[list ? list[i] : i];
        refs_out[i] = ref;
    }
    const uint64_t inc = wave_inclusive(ref >> 32, lane);
    if (lane == 63) part[threadIdx.x >> 6] = inc;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// ONE wave: sums[0 .. nb) become their exclusive prefix sums, 64 at a time with the running total carried along, and
// sums[nb] the total
__global__ __launch_bounds__(64) void carry_scan_sums_kernel(uint64_t *__restrict__ sums, uint64_t nb)
{
    const unsigned lane = threadIdx.x;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nb; base += 64) {   // (uniform over the wave)
        const uint64_t i = base + lane;
        const uint64_t v = i < nb ? sums[i] : 0ull;
        const uint64_t inc = wave_inclusive(v, lane);
        if (i < nb) sums[i] = carry + inc - v;
        carry += shfl64(inc, 63);
    }
    if (lane == 0) sums[nb] = carry;
}

// starts[i] = sums[block of i] + the lengths of the block's rows before i
__global__ __launch_bounds__(256) void carry_starts_kernel(const uint64_t *__restrict__ refs, uint64_t n,
                                                           const uint64_t *__restrict__ sums, uint64_t *__restrict__ starts)
{
    __shared__ uint64_t part[4];
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t len = i < n ? refs[i] >> 32 : 0ull;
    const uint64_t inc = wave_inclusive(len, lane);
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    uint64_t before = sums[blockIdx.x];
    for (unsigned w = 0; w < wave; w++) before += part[w];
    if (i < n) starts[i] = before + inc - len;
}

struct HeapDwords {
    const uint32_t *dwords;
    __device__ uint32_t operator()(uint32_t i) const { return dwords[i]; }
};

// dst piece g = piece piece0 + g of the group's new bytes (column_carry.h), g < n_pieces
__global__ __launch_bounds__(256) void carry_move_bytes_kernel(HeapDwords heap, const uint64_t *__restrict__ refs,
                                                               const uint64_t *__restrict__ starts, uint64_t n,
                                                               uint64_t total, uint64_t piece0, uint64_t n_pieces,
                                                               uint4 *__restrict__ dst)
{
    const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= n_pieces) return;
    uint32_t o[4];
    szgi::carry_piece(heap, refs, starts, n, total, piece0 + g, o);
    dst[g] = make_uint4(o[0], o[1], o[2], o[3]);
}

// out[at[i]] (at null: out[i]) = {base + starts[i], the length of refs[i]}
__global__ __launch_bounds__(256) void carry_new_refs_kernel(const uint64_t *__restrict__ refs,
                                                             const uint64_t *__restrict__ starts, uint64_t n, uint64_t base,
                                                             const uint64_t *__restrict__ at, uint64_t *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    out[at ? at[i] : i] = ((base + starts[i]) & 0xFFFFFFFFull) | (refs[i] & 0xFFFFFFFF00000000ull);
}

// blocks of 256 for `items`, or 0 when they do not fit a grid
unsigned grid_for(uint64_t items)
{
    const uint64_t g = (items + kBlock - 1) / kBlock;
    return g > 0x7FFFFFFFull ? 0u : (unsigned)g;
}

template <typename T>
hipError_t launch_gather(const T *values, const uint64_t *list, const uint64_t *at, T *out, uint64_t n, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const unsigned grid = grid_for(n);
    if (!values || !out || !grid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(carry_gather_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, values, list, at, out, n);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_carry_gather(const void *values, uint32_t elem, const uint64_t *list, const uint64_t *at, void *out,
                               uint64_t n, hipStream_t stream)
{
    if (elem == 8)
        return launch_gather(static_cast<const uint64_t *>(values), list, at, static_cast<uint64_t *>(out), n, stream);
    if (elem == 4)
        return launch_gather(static_cast<const uint32_t *>(values), list, at, static_cast<uint32_t *>(out), n, stream);
    return hipErrorInvalidValue;
}

uint64_t carry_scan_blocks(uint64_t n) { return (n + kBlock - 1) / kBlock; }

hipError_t launch_carry_ref_starts(const uint64_t *refs, const uint64_t *list, uint64_t n, uint64_t *refs_out,
                                   uint64_t *starts, uint64_t *sums, hipStream_t stream)
{
    if (!sums) return hipErrorInvalidValue;
    if (n == 0) return hipMemsetAsync(sums, 0, sizeof(uint64_t), stream);   // (the total)
    const unsigned grid = grid_for(n);
    if (!refs || !refs_out || !starts || !grid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(carry_ref_sums_kernel, dim3(grid), dim3(kBlock), 0, stream, refs, list, n, refs_out, sums);
    hipLaunchKernelGGL(carry_scan_sums_kernel, dim3(1), dim3(64), 0, stream, sums, (uint64_t)grid);
    hipLaunchKernelGGL(carry_starts_kernel, dim3(grid), dim3(kBlock), 0, stream, refs_out, n, sums, starts);
    return hipGetLastError();
}

hipError_t launch_carry_move_bytes(const uint8_t *old_heap, const uint64_t *refs, const uint64_t *starts, uint64_t n,
                                   uint64_t total, uint64_t piece0, uint64_t n_pieces, uint8_t *dst, hipStream_t stream)
{
    if (n_pieces == 0) return hipSuccess;
    const unsigned grid = grid_for(n_pieces);
    if (!dst || !grid || ((uintptr_t)dst & 15) || (total && (!old_heap || !refs || !starts || !n))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(carry_move_bytes_kernel, dim3(grid), dim3(kBlock), 0, stream,
                       HeapDwords{reinterpret_cast<const uint32_t *>(old_heap)}, refs, starts, n, total, piece0, n_pieces,
                       reinterpret_cast<uint4 *>(dst));
    return hipGetLastError();
}

hipError_t launch_carry_new_refs(const uint64_t *refs, const uint64_t *starts, uint64_t n, uint64_t base, const uint64_t *at,
                                 uint64_t *out, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const unsigned grid = grid_for(n);
    if (!refs || !starts || !out || !grid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(carry_new_refs_kernel, dim3(grid), dim3(kBlock), 0, stream, refs, starts, n, base, at, out);
    return hipGetLastError();
}

}  // namespace szg
