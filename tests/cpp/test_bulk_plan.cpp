// Stand-alone check of the host-only part of the bulk mutations (syzgydb_amd/csrc/bulk_plan.h): the validation of a
// caller's row list and its split into per-shard lists with source positions and touched word ranges.  Plain C++, no
// HIP, its own main; tests/test_bulk_cpu.py builds it with -fsanitize=address,undefined and runs it: every list and
// every shard table lives in an exactly-sized heap block, so a read past either end aborts the run.
#include "../../syzgydb_amd/csrc/bulk_plan.h"
#include "../../syzgydb_amd/csrc/reorder_plan.h"

#include <cstdio>
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

using List = std::vector<uint64_t>;

struct Result {
    int rc;
    std::string error;
    szgi::BulkPlan plan;
};

// n_rows rows split over n_shards as a load splits them; the list and the shard tables in heap blocks of exactly their size
static Result plan(uint64_t n_rows, const List &list, size_t n_shards, uint64_t base = 0, int allow_duplicates = 0)
{
    std::unique_ptr<uint64_t[]> rows(list.empty() ? nullptr : new uint64_t[list.size()]);
    for (size_t i = 0; i < list.size(); i++) rows[i] = list[i];
    List counts;
    szgi::split_counts(n_shards, n_rows, &counts);
    std::unique_ptr<uint64_t[]> first(new uint64_t[n_shards ? n_shards : 1]), count(new uint64_t[n_shards ? n_shards : 1]);
    uint64_t at = 0;
    for (size_t s = 0; s < n_shards; s++) first[s] = at, count[s] = counts[s], at += counts[s];
    Result out;
    const char *what = nullptr;
    out.rc = szgi::bulk_plan(first.get(), count.get(), n_shards, base, rows.get(), list.size(), allow_duplicates, &out.plan, &what);
    out.error = what ? what : "(null)";
    return out;
}

int main()
{
    // a good list on one shard: the caller's order and positions survive
    {
        const Result r = plan(200, {199, 0, 64, 63, 5}, 1);
        EXPECT(r.rc == SZG_OK && r.error.empty());
        EXPECT((r.plan.local == std::vector<List>{{199, 0, 64, 63, 5}}));
        EXPECT((r.plan.source == std::vector<List>{{0, 1, 2, 3, 4}}));
        EXPECT(r.plan.word_lo[0] == 0 && r.plan.word_hi[0] == 3);
    }
    // 200 rows on 2 shards (128 + 72) and on 3 (128 + 72 + 0: ceil(200 / 3) rounded up to a multiple of 64 is 128)
    {
        const Result r = plan(200, {130, 5, 128, 127, 199, 0}, 2);
        EXPECT(r.rc == SZG_OK);
        EXPECT((r.plan.local == std::vector<List>{{5, 127, 0}, {2, 0, 71}}));
        EXPECT((r.plan.source == std::vector<List>{{1, 3, 5}, {0, 2, 4}}));
        EXPECT(r.plan.word_lo[0] == 0 && r.plan.word_hi[0] == 1 && r.plan.word_lo[1] == 0 && r.plan.word_hi[1] == 1);
        const Result t = plan(200, {130, 5}, 3);
        EXPECT(t.rc == SZG_OK && t.plan.local.size() == 3 && t.plan.local[2].empty());
        EXPECT(t.plan.word_lo[2] > t.plan.word_hi[2]);   // (an untouched shard)
    }
    // the row base is taken off; rows below it are out of range
    {
        const Result r = plan(10, {1003, 1000}, 1, 1000);
        EXPECT(r.rc == SZG_OK && (r.plan.local[0] == List{3, 0}));
        EXPECT(plan(10, {999}, 1, 1000).rc == SZG_E_RANGE);
        EXPECT(plan(10, {1010}, 1, 1000).rc == SZG_E_RANGE);
    }
    // duplicates: next to each other, far apart, at the ends of a word, across shards -- refused, or accepted by the
    // tombstone form
    for (const List &l : {List{3, 3}, {0, 1, 2, 0}, {63, 64, 63}, {127, 5, 127}, {199, 0, 199}}) {
        const Result r = plan(200, l, 2);
        EXPECT(r.rc == SZG_E_INVALID && r.error == "row listed twice");
        const Result t = plan(200, l, 2, 0, 1);
        EXPECT(t.rc == SZG_OK && t.plan.local[0].size() + t.plan.local[1].size() == l.size());
    }
    // out of range: row == n_rows, far beyond, the largest value; with n_rows that is no multiple of 64; both forms
    for (uint64_t n_rows : {1ull, 63ull, 64ull, 65ull, 129ull, 200ull})
        for (uint64_t bad : {n_rows, n_rows + 1, n_rows + 64, (uint64_t)1 << 40, UINT64_MAX})
            for (int dup : {0, 1})
                for (size_t shards : {(size_t)1, (size_t)3}) {
                    const Result r = plan(n_rows, {0, bad}, shards, 0, dup);
                    EXPECT(r.rc == SZG_E_RANGE && r.error == "row out of range");
                }
    // more entries than rows: out of range is reported where there is one, a duplicate otherwise
    EXPECT(plan(3, {0, 1, 2, 7}, 1).rc == SZG_E_RANGE);
    EXPECT(plan(3, {0, 1, 2, 1}, 1).rc == SZG_E_INVALID);
    EXPECT(plan(3, {0, 1, 2, 1}, 1, 0, 1).rc == SZG_OK);
    EXPECT(plan(0, {0}, 1).rc == SZG_E_RANGE);
    // the tombstone plan's word ranges
    {
        const Result r = plan(200, {0, 63, 64, 129}, 1, 0, 1);
        EXPECT(r.rc == SZG_OK && r.plan.word_lo[0] == 0 && r.plan.word_hi[0] == 2);
        const Result t = plan(200, {0, 63, 64, 129}, 2, 0, 1);
        EXPECT(t.rc == SZG_OK && t.plan.word_lo[0] == 0 && t.plan.word_hi[0] == 1);
        EXPECT(t.plan.word_lo[1] == 0 && t.plan.word_hi[1] == 0 && (t.plan.local[1] == List{1}));
        const Result u = plan(200, {129, 70}, 1, 0, 1);
        EXPECT(u.rc == SZG_OK && u.plan.word_lo[0] == 1 && u.plan.word_hi[0] == 2);
    }
    // empty lists; a null list with entries; no shards
    {
        const Result r = plan(50, {}, 3);
        EXPECT(r.rc == SZG_OK && r.plan.local.size() == 3 && r.plan.local[0].empty() && r.plan.word_lo[0] > r.plan.word_hi[0]);
        EXPECT(plan(0, {}, 1).rc == SZG_OK);
        szgi::BulkPlan p;
        const char *what = nullptr;
        const uint64_t first = 0, count = 5;
        EXPECT(szgi::bulk_plan(&first, &count, 1, 0, nullptr, 2, 0, &p, &what) == SZG_E_INVALID);
        EXPECT(szgi::bulk_plan(&first, &count, 0, 0, nullptr, 0, 0, &p, &what) == SZG_E_INVALID);
        EXPECT(szgi::bulk_plan(nullptr, nullptr, 1, 0, nullptr, 0, 0, &p, &what) == SZG_E_INVALID);
    }
    // shards that do not start where a load would put them (a handle that grew by appends): an empty shard in between
    {
        const uint64_t first[3] = {0, 0, 192}, count[3] = {192, 0, 8};
        std::unique_ptr<uint64_t[]> rows(new uint64_t[3]{199, 191, 192});
        szgi::BulkPlan p;
        const char *what = nullptr;
        EXPECT(szgi::bulk_plan(first, count, 3, 0, rows.get(), 3, 0, &p, &what) == SZG_OK);
        EXPECT((p.local == std::vector<List>{{191}, {}, {7, 0}}) && (p.source == std::vector<List>{{1}, {}, {0, 2}}));
        rows[0] = 200;
        EXPECT(szgi::bulk_plan(first, count, 3, 0, rows.get(), 3, 0, &p, &what) == SZG_E_RANGE);
    }
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::puts("bulk plan ok");
    return 0;
}
