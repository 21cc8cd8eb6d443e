// Stand-alone check of the host-only part of szg_index_reorder (syzgydb_amd/csrc/reorder_plan.h): the validation of a
// caller's row list and the split of the new rows over shards.  Plain C++, no HIP, its own main; tests/test_reorder_cpu.py
// builds it with -fsanitize=address,undefined and runs it: every list lives in an exactly-sized heap block, so a read
// or write past either end of a list, the live words or the output aborts the run.
#include "../../syzgydb_amd/csrc/reorder_plan.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

static int g_failures = 0;

#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_failures++;                                                       \
        }                                                                       \
    } while (0)

struct Result {
    int rc;
    std::string error;
    std::vector<uint64_t> local, counts;
};

// lists and live words in heap blocks of exactly their size
static Result plan(uint64_t n_rows, const std::vector<bool> *live, const std::vector<uint64_t> &list, size_t n_shards,
                   uint64_t base = 0)
{
    std::unique_ptr<uint64_t[]> rows(list.empty() ? nullptr : new uint64_t[list.size()]);
    for (size_t i = 0; i < list.size(); i++) rows[i] = list[i];
    const size_t words = (size_t)((n_rows + 63) / 64);
    std::unique_ptr<uint64_t[]> bits;
    if (live && words) {
        bits.reset(new uint64_t[words]);
        std::memset(bits.get(), 0, words * sizeof(uint64_t));
        for (uint64_t r = 0; r < n_rows; r++)
            if ((*live)[(size_t)r]) bits[(size_t)(r / 64)] |= 1ull << (r % 64);
    }
    Result out;
    const char *what = nullptr;
    out.rc = szgi::reorder_plan(n_rows, bits.get(), base, rows.get(), list.size(), n_shards, &out.local, &out.counts, &what);
    out.error = what ? what : "(null)";
    return out;
}

int main()
{
    // a good list: a permutation of a subset
    {
        const Result r = plan(100, nullptr, {99, 0, 64, 63, 5}, 1);
        EXPECT(r.rc == SZG_OK && r.error.empty());
        EXPECT((r.local == std::vector<uint64_t>{99, 0, 64, 63, 5}));
        EXPECT((r.counts == std::vector<uint64_t>{5}));
    }
    // the row base is taken off; rows below it are out of range
    {
        const Result r = plan(10, nullptr, {1003, 1000}, 1, 1000);
        EXPECT(r.rc == SZG_OK && (r.local == std::vector<uint64_t>{3, 0}));
        EXPECT(plan(10, nullptr, {999}, 1, 1000).rc == SZG_E_RANGE);
        EXPECT(plan(10, nullptr, {1010}, 1, 1000).rc == SZG_E_RANGE);
    }
    // duplicates: next to each other, far apart, at the ends of a word
    for (const std::vector<uint64_t> &l : {std::vector<uint64_t>{3, 3}, {0, 1, 2, 0}, {63, 64, 63}, {127, 5, 127}}) {
        const Result r = plan(128, nullptr, l, 2);
        EXPECT(r.rc == SZG_E_INVALID && r.error == "row listed twice");
    }
    // out of range: row == n_rows, far beyond, the largest value; with n_rows that is no multiple of 64
    for (uint64_t n_rows : {1ull, 63ull, 64ull, 65ull, 129ull})
        for (uint64_t bad : {n_rows, n_rows + 1, n_rows + 64, (uint64_t)1 << 40, UINT64_MAX}) {
            const Result r = plan(n_rows, nullptr, {0, bad}, 1);
            EXPECT(r.rc == SZG_E_RANGE && r.error == "row out of range");
        }
    // more entries than rows: out of range is reported where there is one, a duplicate otherwise
    EXPECT(plan(3, nullptr, {0, 1, 2, 7}, 1).rc == SZG_E_RANGE);
    EXPECT(plan(3, nullptr, {0, 1, 2, 1}, 1).rc == SZG_E_INVALID);
    EXPECT(plan(0, nullptr, {0}, 1).rc == SZG_E_RANGE);
    // dead rows
    {
        std::vector<bool> live(130, true);
        live[0] = live[64] = live[129] = false;
        for (uint64_t dead : {0ull, 64ull, 129ull}) {
            const Result r = plan(130, &live, {1, dead}, 3);
            EXPECT(r.rc == SZG_E_INVALID && r.error == "row is tombstoned");
        }
        EXPECT(plan(130, &live, {1, 63, 65, 128}, 3).rc == SZG_OK);
        EXPECT(plan(130, &live, {130}, 3).rc == SZG_E_RANGE);  // (the range is checked before the live word is read)
    }
    // empty lists; a null list with entries; no shards
    {
        const Result r = plan(50, nullptr, {}, 3);
        EXPECT(r.rc == SZG_OK && r.local.empty() && (r.counts == std::vector<uint64_t>{0, 0, 0}));
        EXPECT(plan(0, nullptr, {}, 1).rc == SZG_OK);
        std::vector<uint64_t> local, counts;
        const char *what = nullptr;
        EXPECT(szgi::reorder_plan(5, nullptr, 0, nullptr, 2, 1, &local, &counts, &what) == SZG_E_INVALID);
        EXPECT(szgi::reorder_plan(5, nullptr, 0, nullptr, 0, 0, &local, &counts, &what) == SZG_E_INVALID);
    }
    // the split: contiguous ranges whose boundaries are multiples of 64
    {
        struct Case {
            uint64_t n;
            size_t shards;
            std::vector<uint64_t> want;
        };
        const Case cases[] = {{1, 1, {1}},      {1, 2, {1, 0}},     {1, 3, {1, 0, 0}},     {64, 1, {64}},
                              {64, 2, {64, 0}}, {64, 3, {64, 0, 0}}, {65, 1, {65}},        {65, 2, {64, 1}},
                              {65, 3, {64, 1, 0}}, {129, 1, {129}},  {129, 2, {128, 1}},   {129, 3, {64, 64, 1}},
                              {0, 2, {0, 0}}};
        for (const Case &c : cases) {
            std::vector<uint64_t> list((size_t)c.n);
            for (uint64_t i = 0; i < c.n; i++) list[(size_t)i] = c.n - 1 - i;
            const Result r = plan(c.n, nullptr, list, c.shards);
            EXPECT(r.rc == SZG_OK && r.counts == c.want);
        }
    }
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::puts("reorder plan ok");
    return 0;
}
