// carry_kernel.hip -- the kernels that carry a number, a code and a text column across a compaction
// (kernels_column_carry.hip, column_carry.h; the present bits through kernels_mask.hip) alone, timed with HIP events
// against the bytes they must move.  The text column is distinct per row, about 25 bytes: "user%07d@example%d.com".
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 scripts/carry_kernel/carry_kernel.hip \
//         syzgydb_amd/csrc/kernels_column_carry.hip syzgydb_amd/csrc/kernels_mask.hip -o scripts/carry_kernel/carry_kernel
//   scripts/carry_kernel/carry_kernel [rows = 1000000] [dropped percent = 10] [repeats = 20]
//
// Every `100 / percent`-th row is dropped, the others keep their order (a compaction's list).  Prints one JSON line per
// column kind: 3 warm-up rounds, then `repeats` timed ones, and the text column's new bytes against the host's.
// "bytes_it_must_move" counts the list (8 B per kept row), the values or references read and written, the present
// words read and written, and for the text column the kept bytes read and the new heap written; what the kernels move
// on top of that -- the list read once per launch, the gathered references and the starts -- is their own overhead.
// scripts/dev_compact_columns.py runs it when it has been built.
#include "../../syzgydb_amd/csrc/kernels.h"
#include "../../syzgydb_amd/csrc/column_carry.h"

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

int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000ull;
    const int percent = argc > 2 ? atoi(argv[2]) : 10;
    const int repeats = argc > 3 ? atoi(argv[3]) : 20;
    if (n == 0 || n > 9999999ull || percent <= 0 || percent > 50 || repeats <= 0) return 2;
    const uint64_t every = 100 / (uint64_t)percent;
    std::vector<uint64_t> refs((size_t)n), list;
    std::string bytes, kept_bytes;
    for (uint64_t i = 0; i < n; i++) {
        char text[64];
        snprintf(text, sizeof(text), "user%07llu@example%llu.com", (unsigned long long)((i * 2654435761ull) % 10000000ull),
                 (unsigned long long)(i % 97));
        refs[(size_t)i] = (uint64_t)bytes.size() | ((uint64_t)strlen(text) << 32);
        bytes += text;
        if (i % every != 0) list.push_back(i), kept_bytes += text;
    }
    const uint64_t m = list.size(), used = bytes.size(), cap = szgi::str_heap_capacity(used);
    const uint64_t new_cap = szgi::carry_heap_capacity(kept_bytes.size()), cap_rows = szgi::carry_cap_rows(m);
    const uint64_t old_words = (n + 63) / 64, nb = szg::carry_scan_blocks(m);
    uint8_t *heap, *new_heap;
    uint64_t *d_refs, *d_list, *present, *new_present, *tmp_refs, *starts, *sums, *new_refs;
    CHECK(hipMalloc((void **)&heap, cap));
    CHECK(hipMalloc((void **)&new_heap, new_cap));
    CHECK(hipMalloc((void **)&d_refs, n * 8));
    CHECK(hipMalloc((void **)&d_list, m * 8));
    CHECK(hipMalloc((void **)&present, (old_words + 1) * 8));
    CHECK(hipMalloc((void **)&new_present, cap_rows / 8));
    CHECK(hipMalloc((void **)&tmp_refs, m * 8));
    CHECK(hipMalloc((void **)&starts, m * 8));
    CHECK(hipMalloc((void **)&sums, (nb + 1) * 8));
    CHECK(hipMalloc((void **)&new_refs, cap_rows * 8));
    CHECK(hipMemset(heap, 0, cap));
    CHECK(hipMemcpy(heap, bytes.data(), used, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_refs, refs.data(), n * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_list, list.data(), m * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(present, 0x5A, (old_words + 1) * 8));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const double present_bytes = (double)old_words * 8 + (double)cap_rows / 8, list_bytes = (double)m * 8;
    int bad = 0;
    for (int kind = 0; kind < 3; kind++) {   // 0: 8-byte values, 1: 4-byte codes, 2: text
        float ms = 0;
        for (int r = 0; r < repeats + 3; r++) {
            if (r == 3) CHECK(hipEventRecord(e0, nullptr));
            CHECK(szg::launch_mask_gather_rows(present, d_list, m, new_present, cap_rows / 128, nullptr));
            if (kind < 2) {
                CHECK(szg::launch_carry_gather(d_refs, kind == 0 ? 8 : 4, d_list, nullptr, new_refs, m, nullptr));
                continue;
            }
            uint64_t total = 0;
            CHECK(szg::launch_carry_ref_starts(d_refs, d_list, m, tmp_refs, starts, sums, nullptr));
            CHECK(hipMemcpy(&total, sums + nb, 8, hipMemcpyDeviceToHost));   // (the library reads it back here too)
            if (total != kept_bytes.size()) return 3;
            CHECK(szg::launch_carry_move_bytes(heap, tmp_refs, starts, m, total, 0, new_cap / 16, new_heap, nullptr));
            CHECK(szg::launch_carry_new_refs(tmp_refs, starts, m, 0, nullptr, new_refs, nullptr));
        }
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        double must = present_bytes + list_bytes;
        const char *name = kind == 0 ? "8-byte values" : kind == 1 ? "4-byte codes" : "text";
        if (kind < 2) must += 2.0 * (double)m * (kind == 0 ? 8 : 4);
        else must += 2.0 * (double)m * 8 + (double)kept_bytes.size() + (double)new_cap;
        bool ok = true;
        if (kind == 2) {
            std::vector<uint8_t> got((size_t)new_cap);
            std::vector<uint64_t> got_refs((size_t)m);
            CHECK(hipMemcpy(got.data(), new_heap, new_cap, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(got_refs.data(), new_refs, m * 8, hipMemcpyDeviceToHost));
            ok = memcmp(got.data(), kept_bytes.data(), kept_bytes.size()) == 0;
            for (uint64_t i = kept_bytes.size(); i < new_cap; i++) ok &= got[(size_t)i] == 0;
            uint64_t at = 0;
            for (uint64_t i = 0; i < m; i++) {
                ok &= got_refs[(size_t)i] == (at | (refs[(size_t)list[(size_t)i]] & 0xFFFFFFFF00000000ull));
                at += refs[(size_t)list[(size_t)i]] >> 32;
            }
        }
        const double per = ms / repeats;
        printf("{\"what\": \"carry kernels, %s\", \"rows\": %llu, \"kept_rows\": %llu, \"kept_heap_bytes\": %llu, \"repeats\": %d, "
               "\"ms_per_carry\": %.4f, \"bytes_it_must_move\": %.0f, \"gb_per_s\": %.1f, \"ok\": %s}\n",
               name, (unsigned long long)n, (unsigned long long)m, (unsigned long long)(kind == 2 ? kept_bytes.size() : 0),
               repeats, per, must, must / (per * 1e-3) / 1e9, ok ? "true" : "false");
        bad |= !ok;
    }
    return bad ? 3 : 0;
}
