// where_text_kernel.hip -- the text compare kernel of the resident columns (kernels_column.hip, column_str.h) alone, timed
// with HIP events against the bytes it must read: 8 B/row of references, the rows' bytes in the heap, 1/8 B/row of present
// words read and 1/8 B/row of mask written.  The column is distinct per row, about 25 bytes: "user%07d@example%d.com".
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 scripts/where_kernel/where_text_kernel.hip \
//         syzgydb_amd/csrc/kernels_column.hip -o scripts/where_kernel/where_text_kernel
//   scripts/where_kernel/where_text_kernel [rows = 1000000] [launches = 50]
//
// Prints one JSON line per operator (CONTAINS, ENDS_WITH, ==, <): 5 warm-up launches, then `launches` timed ones with a
// new constant each, and the count of the last one against the host's.  scripts/dev_where_text.py runs it when it has
// been built.
#include "../../syzgydb_amd/csrc/kernels.h"
#include "../../syzgydb_amd/csrc/column_str.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CHECK(expr)                                                                          \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess) {                                                             \
            fprintf(stderr, "%s: %s\n", #expr, hipGetErrorString(e__));                      \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)

static bool host_verdict(int op, const std::string &v, const std::string &c)
{
    switch (op) {
    case 0: return v == c;
    case 2: return v < c;   // (ASCII only here: char order is byte order)
    case 7: return v.size() >= c.size() && v.compare(v.size() - c.size(), c.size(), c) == 0;
    default: return v.find(c) != std::string::npos;
    }
}

int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000ull;
    const int launches = argc > 2 ? atoi(argv[2]) : 50;
    if (n == 0 || n > 9999999ull || launches <= 0) return 2;
    const uint64_t words = (n + 63) / 64, pairs = (words + 1) / 2;
    // the column as the library lays it out: the strings back to back, one {start, len} per row, 16 zero bytes of slack
    std::vector<std::string> values((size_t)n);
    std::vector<uint64_t> refs((size_t)n);
    std::string bytes;
    for (uint64_t i = 0; i < n; i++) {
        char text[64];
        snprintf(text, sizeof(text), "user%07llu@example%llu.com", (unsigned long long)((i * 2654435761ull) % 10000000ull),
                 (unsigned long long)(i % 97));
        values[(size_t)i] = text;
        refs[(size_t)i] = (uint64_t)bytes.size() | ((uint64_t)strlen(text) << 32);
        bytes += text;
    }
    const uint64_t used = bytes.size(), cap = szgi::str_heap_capacity(used);
    uint8_t *heap;
    uint64_t *d_refs, *present, *out, *count;
    uint32_t *constant;
    CHECK(hipMalloc((void **)&heap, cap));
    CHECK(hipMalloc((void **)&d_refs, n * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&present, 2 * pairs * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&out, 2 * pairs * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&count, 2 * sizeof(uint64_t)));
    CHECK(hipMalloc((void **)&constant, szgi::kStrPatternMax));
    CHECK(hipMemset(heap, 0, cap));
    CHECK(hipMemcpy(heap, bytes.data(), used, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_refs, refs.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
    CHECK(hipMemset(present, 0xFF, 2 * pairs * sizeof(uint64_t)));   // (the kernel clears the tail itself)
    const szg::ColumnWhere w{present, nullptr, out, pairs, n, count};
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const struct { int op; const char *name, *format; } legs[] = {
        {8, "CONTAINS", "%03d@example"}, {7, "ENDS_WITH", "@example%d.com"}, {0, "==", "user%07d@example5.com"},
        {2, "<", "user%07d"}};
    int bad = 0;
    for (const auto &leg : legs) {
        // the constants of the timed launches, one buffer each (uploaded before the clock starts)
        std::vector<std::string> constants;
        for (int i = 0; i < launches + 5; i++) {
            char text[64];
            snprintf(text, sizeof(text), leg.format, leg.op == 0 ? (int)((i * 2654435761ull) % 10000000ull) : leg.op == 2 ? 1000 * i + 500 : i);
            constants.push_back(text);
        }
        uint32_t *all;
        CHECK(hipMalloc((void **)&all, constants.size() * 64));
        CHECK(hipMemset(all, 0, constants.size() * 64));
        for (size_t i = 0; i < constants.size(); i++)
            CHECK(hipMemcpy((uint8_t *)all + 64 * i, constants[i].data(), constants[i].size(), hipMemcpyHostToDevice));
        for (int i = 0; i < 5; i++)
            CHECK(szg::launch_column_str(d_refs, heap, leg.op, all + 16 * i, (uint32_t)constants[i].size(), w, nullptr));
        CHECK(hipEventRecord(e0, nullptr));
        for (int i = 5; i < launches + 5; i++)
            CHECK(szg::launch_column_str(d_refs, heap, leg.op, all + 16 * i, (uint32_t)constants[i].size(), w, nullptr));
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        // the last constant once more, counted
        const std::string &c = constants.back();
        CHECK(hipMemset(count, 0, 2 * sizeof(uint64_t)));
        CHECK(szg::launch_column_str(d_refs, heap, leg.op, all + 16 * (constants.size() - 1), (uint32_t)c.size(), w, nullptr));
        uint64_t got = 0, want = 0;
        CHECK(hipMemcpy(&got, count, sizeof(got), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; i++) want += host_verdict(leg.op, values[(size_t)i], c);
        const double per = ms / launches, must = (double)n * 8.0 + (double)used + (double)pairs * 16.0 * 2.0;
        printf("{\"what\": \"column_where_kernel<StrWhere> %s\", \"rows\": %llu, \"heap_bytes\": %llu, \"launches\": %d, "
               "\"ms_per_launch\": %.4f, \"bytes_it_must_read_and_write\": %.0f, \"gb_per_s\": %.1f, \"count\": %llu, "
               "\"count_ok\": %s}\n",
               leg.name, (unsigned long long)n, (unsigned long long)used, launches, per, must, must / (per * 1e-3) / 1e9,
               (unsigned long long)got, got == want ? "true" : "false");
        bad |= got != want;
        CHECK(hipFree(all));
    }
    return bad ? 3 : 0;
}
