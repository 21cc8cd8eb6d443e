// where_kernel.hip -- the float64 compare kernel of the resident columns (kernels_column.hip) alone, timed with HIP events
// against its algorithmic bytes: 8 B/row of values, 2/8 B/row of present and base words read, 1/8 B/row of mask written.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 scripts/where_kernel/where_kernel.hip syzgydb_amd/csrc/kernels_column.hip \
//         -o scripts/where_kernel/where_kernel
//   scripts/where_kernel/where_kernel [rows = 100000000] [launches = 50]
//
// Prints one JSON line.  scripts/dev_where.py runs it when it has been built.
#include "../../syzgydb_amd/csrc/kernels.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__));                      \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

__global__ void fill_values(double *v, uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        v[i] = (double)((i * 2654435761ull) % 1000ull) * 0.1;   // 0.0 .. 99.9
}

int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 100000000ull;
    const int launches = argc > 2 ? atoi(argv[2]) : 50;
    if (n == 0 || launches <= 0) return 2;
    const uint64_t words = (n + 63) / 64, pairs = (words + 1) / 2;
    double *values;
    uint64_t *present, *base, *out, *count;
    CHECK(hipMalloc((void **)&values, n * sizeof(double)));
    CHECK(hipMalloc((void **)&present, 2 * pairs * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&base, 2 * pairs * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&out, 2 * pairs * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&count, 2 * sizeof(uint64_t)));
    hipLaunchKernelGGL(fill_values, dim3(4096), dim3(256), 0, nullptr, values, n);
    CHECK(hipGetLastError());
    CHECK(hipMemset(present, 0xFF, 2 * pairs * sizeof(uint64_t)));   // (the kernel clears the tail itself)
    CHECK(hipMemset(base, 0xAA, 2 * pairs * sizeof(uint64_t)));      // every second row
    const szg::ColumnWhere w{present, base, out, pairs, n, count};
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int i = 0; i < 5; i++) CHECK(szg::launch_column_cmp_f64(values, 2, 37.5 + i, w, nullptr));   // warm-up
    CHECK(hipMemset(count, 0, 2 * sizeof(uint64_t)));
    CHECK(szg::launch_column_cmp_f64(values, 2, 37.5, w, nullptr));
    uint64_t got = 0;
    CHECK(hipMemcpy(&got, count, sizeof(got), hipMemcpyDeviceToHost));
    uint64_t want = 0;   // value < 37.5 on the odd rows
    for (uint64_t i = 1; i < n; i += 2) want += ((i * 2654435761ull) % 1000ull) < 375ull;
    CHECK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < launches; i++) CHECK(szg::launch_column_cmp_f64(values, 2, 10.0 + i, w, nullptr));
    CHECK(hipEventRecord(e1, nullptr));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    const double per = ms / launches, bytes = (double)n * 8.0 + (double)pairs * 16.0 * 3.0;
    printf("{\"what\": \"column_where_kernel<CmpF64>\", \"rows\": %llu, \"launches\": %d, \"ms_per_launch\": %.4f, "
           "\"algorithmic_bytes\": %.0f, \"gb_per_s\": %.1f, \"count_ok\": %s}\n",
           (unsigned long long)n, launches, per, bytes, bytes / (per * 1e-3) / 1e9, got == want ? "true" : "false");
    return got == want ? 0 : 3;
}
