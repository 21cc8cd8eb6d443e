// kernels_bulk.hip -- the scatters of the bulk mutations (scan_bulk.cpp): entry i of a dense stage goes to position
// list[i] of what is resident.  The host has checked every list (bulk_plan.h: in range, and -- where two writers to one
// position would race -- listed once); each kernel still tests list[i] against the bound it is given and writes
// nothing for an entry that fails.
//
//   scatter_rows_kernel     the mirror image of gather_rows_kernel (kernels_exact.hip): row i of a linear stage ->
//                           row list[i] of the resident rows in the shard's own layout, 16 bytes per lane, groups of
//                           lanes per row.  No decode: a piece's bytes do not depend on its row's number.
//   column_scatter_kernel   4- and 8-byte elements, one lane each: out[list[i]] = in[i] (column values; the float32
//                           norms of overwritten rows, computed over the stage by launch_row_norms -- the same kernels,
//                           the same summation order, so the same bits as a norm taken in place)
//
// Plain C++ and vector memory operations only.
#include "kernels.h"

namespace szg {

namespace {

// Groups of G = 1 << g_shift lanes take one row each, lane s of a group the pieces s, s + G, ...: consecutive lanes
// move consecutive pieces, whole 64-byte segments of a tiled row.  The group's first lane reads list[i] and hands it
// to the others.
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint8_t *__restrict__ src, RowLayout src_lay,
                                                           uint8_t *__restrict__ dst, RowLayout dst_lay, uint32_t r16,
                                                           const uint64_t *__restrict__ list, uint64_t n, uint64_t dst_rows,
                                                           int g_shift)
{
    const uint32_t G = 1u << g_shift;
    const uint32_t sub = threadIdx.x & (G - 1);
    const uint64_t i = (uint64_t)blockIdx.x * (256u >> g_shift) + (threadIdx.x >> g_shift);
    const bool have = i < n;
    uint64_t v = 0;
    if (have && sub == 0) v = list[i];
    const int lead = (int)((threadIdx.x & 63u) & ~(G - 1));
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lead, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lead, 64);
    const uint64_t to = ((uint64_t)hi << 32) | lo;
    if (!have || to >= dst_rows) return;
    for (uint32_t j = sub; j < r16; j += G)
        *reinterpret_cast<uint4 *>(dst + piece_offset(dst_lay, to, j)) =
            *reinterpret_cast<const uint4 *>(src + piece_offset(src_lay, i, j));
}

template <typename T>
__global__ __launch_bounds__(256) void column_scatter_kernel(const T *__restrict__ in, const uint64_t *__restrict__ list,
                                                             uint64_t n, T *__restrict__ out, uint64_t out_n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t to = list[i];
    if (to < out_n) out[to] = in[i];
}

}  // namespace

hipError_t launch_scatter_rows(const uint8_t *src, RowLayout src_lay, uint8_t *dst, RowLayout dst_lay, uint32_t r16,
                               const uint64_t *list, uint64_t n, uint64_t dst_rows, hipStream_t stream)
{
    if (n == 0 || r16 == 0) return hipSuccess;
    if (!list) return hipErrorInvalidValue;
    int g_shift = 0;  // lanes per row: the power of two that covers r16, one wave at the most
    while (g_shift < 6 && (1u << g_shift) < r16) g_shift++;
    const uint64_t rows_per_block = 256u >> g_shift;
    const uint64_t grid = (n + rows_per_block - 1) / rows_per_block;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)grid), dim3(256), 0, stream, src, src_lay, dst, dst_lay, r16,
                       list, n, dst_rows, g_shift);
    return hipGetLastError();
}

hipError_t launch_column_scatter(const void *in, uint32_t elem, const uint64_t *list, uint64_t n, void *out, uint64_t out_n,
                                 hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (!list || (elem != 4 && elem != 8)) return hipErrorInvalidValue;
    const uint64_t grid = (n + 255) / 256;
    if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (elem == 8)
        hipLaunchKernelGGL(column_scatter_kernel<uint64_t>, dim3((unsigned)grid), dim3(256), 0, stream,
                           static_cast<const uint64_t *>(in), list, n, static_cast<uint64_t *>(out), out_n);
    else
        hipLaunchKernelGGL(column_scatter_kernel<uint32_t>, dim3((unsigned)grid), dim3(256), 0, stream,
                           static_cast<const uint32_t *>(in), list, n, static_cast<uint32_t *>(out), out_n);
    return hipGetLastError();
}

}  // namespace szg
