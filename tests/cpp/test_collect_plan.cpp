// Stand-alone check of the buffer arithmetic of a radius batch (syzgydb_amd/csrc/collect_plan.h): the entries per query,
// the block-copy decision, the list layout in the pinned buffer and the cap a context carries from batch to batch.
// Plain C++, no HIP, its own main; tests/test_collect_plan_cpu.py builds it with -fsanitize=address,undefined and runs
// it: the "device" and "pinned" buffers are heap blocks of exactly the sizes the header computes, every list is written
// and read at the offsets the header gives, so an index past either end aborts the run.  Every expected number below
// is written out by hand from the rules (start at 1024; the smallest power of two >= most + most / 4; the ceiling
// 1 << 20; an eighth down per batch at most; 8M entries per limited batch; one block up to max(2 MiB, nq * 64 KiB)).
#include "../../syzgydb_amd/csrc/collect_plan.h"

#include <cstdio>
#include <cstring>
#include <memory>

static int g_failures = 0;

#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_failures++;                                                       \
        }                                                                       \
    } while (0)

struct Entry {  // one re-ranked hit, 16 bytes like the library's
    uint32_t row, ukey;
    double dist;
};
static_assert(sizeof(Entry) == szgi::kCollectEntryBytes, "the size the header counts with");

constexpr size_t kStride = 32;  // counters one 128-byte line apart, as the sweeps keep them

enum Counts { kZero, kOne, kCapLess1, kCap, kCapPlus1, kAllOver, kMixed };

static uint32_t count_of(Counts what, int j, size_t cap)
{
    switch (what) {
    case kZero: return 0;
    case kOne: return 1;
    case kCapLess1: return (uint32_t)(cap - 1);
    case kCap: return (uint32_t)cap;
    case kCapPlus1: return (uint32_t)(cap + 1);
    case kAllOver: return (uint32_t)(cap + 1 + 7 * (size_t)j);
    default: break;
    }
    const uint32_t mix[6] = {0, 1, (uint32_t)(cap - 1), (uint32_t)cap, (uint32_t)(cap + 1), 17};
    return mix[j % 6];
}

// One batch the way scan_radius.cpp runs it: buffers of the header's sizes, the heads staged, the sweeps' appends (never
// beyond cap: the kernels only count there), the counters, the tail per part [0, early) and [early, nq), the copy back
// in the form the header chose, and every list read where the layout says it is.
static void round_trip(size_t radius_cap, int nq, bool limited, size_t head_max, Counts what, int early)
{
    const size_t cap = szgi::collect_cap(radius_cap, nq, limited, head_max);
    EXPECT(cap >= 1024 && cap >= head_max + 1024);
    const size_t block = szgi::collect_block_entries(cap, nq);
    EXPECT(block == cap * (size_t)nq);
    std::unique_ptr<uint64_t[]> d_collect(new uint64_t[block]);
    std::unique_ptr<Entry[]> d_out(new Entry[block]);
    std::unique_ptr<uint32_t[]> counts(new uint32_t[(size_t)nq * kStride]);
    std::memset(counts.get(), 0xEE, sizeof(uint32_t) * (size_t)nq * kStride);
    for (int j = 0; j < nq; j++) {
        const size_t head = head_max ? head_max - (size_t)(j % 3) : 0;  // (the longest head is head_max)
        for (size_t i = 0; i < head; i++) d_collect[(size_t)j * cap + i] = 0xFFFFFFFF00000000ull | i;
        const uint32_t n = std::max<uint32_t>(count_of(what, j, cap), (uint32_t)head);  // (a counter starts at its head's count)
        counts[(size_t)j * kStride] = n;
        for (size_t i = head; i < std::min<size_t>(n, cap); i++) d_collect[(size_t)j * cap + i] = ((uint64_t)j << 32) | i;
    }
    // the tail, part by part: what the re-rank reads and writes for queries [q0, q1) lies inside the block
    for (int part = 0; part < 2; part++) {
        const int q0 = part ? early : 0, q1 = part ? nq : early;
        if (q0 == q1) continue;
        EXPECT((size_t)q0 * cap + szgi::collect_block_entries(cap, q1 - q0) <= block);
        for (int j = q0; j < q1; j++)
            for (size_t i = 0; i < std::min<size_t>(counts[(size_t)j * kStride], cap); i++)
                d_out[(size_t)j * cap + i] = Entry{(uint32_t)d_collect[(size_t)j * cap + i], (uint32_t)j, (double)i};
    }
    const bool copied = szgi::collect_block_copied(cap, nq);
    const size_t one_block = std::max<size_t>(2u << 20, (size_t)nq * (64u << 10));
    EXPECT(copied == (block * 16 <= one_block));
    szgi::CollectLayout at;
    szgi::collect_layout(counts.get(), kStride, nq, cap, copied, &at);
    EXPECT(at.cnt.size() == (size_t)nq && at.off.size() == (size_t)nq && at.over.size() == (size_t)nq);
    std::unique_ptr<Entry[]> h_out(new Entry[at.host_entries]);
    if (copied) {
        EXPECT(at.host_entries == block);
        std::memcpy(h_out.get(), d_out.get(), block * sizeof(Entry));  // (unwritten entries travel too: they are never read)
    }
    size_t most = 0, total = 0;
    for (int j = 0; j < nq; j++) {
        const size_t n = counts[(size_t)j * kStride];
        most = std::max(most, n);
        EXPECT(at.over[j] == (n > cap ? 1 : 0));
        EXPECT(at.cnt[j] == (n > cap ? 0 : n));
        EXPECT(at.off[j] == (copied ? (size_t)j * cap : total));
        EXPECT(at.off[j] + at.cnt[j] <= at.host_entries);
        if (!copied && at.cnt[j]) std::memcpy(h_out.get() + at.off[j], d_out.get() + (size_t)j * cap, at.cnt[j] * sizeof(Entry));
        total += at.cnt[j];
    }
    EXPECT(at.most == most);
    if (!copied) EXPECT(at.host_entries == total);
    for (int j = 0; j < nq; j++)
        for (size_t i = 0; i < at.cnt[j]; i++) {
            const Entry &e = h_out[at.off[j] + i];
            EXPECT(e.row == (uint32_t)i && e.ukey == (uint32_t)j && e.dist == (double)i);
        }
    if (what == kAllOver) EXPECT(total == 0 && (copied || at.host_entries == 0));
}

int main()
{
    const int nqs[5] = {1, 4, 16, 32, 96};
    // the cap where the block stops travelling whole: max(2 MiB, nq * 64 KiB) / (nq * 16 bytes)
    const size_t edge[5] = {131072, 32768, 8192, 4096, 4096};

    // every count pattern, every batch size, heads of 0 and of more than 1024, with and without an early part
    for (int q = 0; q < 5; q++)
        for (Counts what : {kZero, kOne, kCapLess1, kCap, kCapPlus1, kAllOver, kMixed})
            for (size_t head_max : {(size_t)0, (size_t)3000})
                for (size_t radius_cap : {(size_t)0, (size_t)1500, (size_t)4096})
                    round_trip(radius_cap, nqs[q], radius_cap != 1500, head_max, what, nqs[q] > 4 ? 4 : 0);

    // the copied / not-copied boundary, one entry on either side
    for (int q = 0; q < 5; q++) {
        EXPECT(szgi::collect_block_copied(edge[q], nqs[q]));
        EXPECT(!szgi::collect_block_copied(edge[q] + 1, nqs[q]));
        EXPECT(szgi::collect_cap(edge[q] + 1, nqs[q], true, 0) == edge[q] + 1);  // (a context carries any cap, not only powers of two)
        for (size_t cap : {edge[q] - 1, edge[q], edge[q] + 1})
            for (Counts what : {kMixed, kCap, kAllOver}) round_trip(cap, nqs[q], true, 0, what, 0);
    }

    // the cap of a batch
    EXPECT(szgi::collect_cap(0, 1, false, 0) == 1024);
    EXPECT(szgi::collect_cap(0, 96, true, 0) == 1024);
    EXPECT(szgi::collect_cap(1000, 16, true, 0) == 1024);
    EXPECT(szgi::collect_cap(57344, 4, true, 0) == 57344);
    EXPECT(szgi::collect_cap(57344, 96, true, 0) == 57344);    // 8M / 96 = 87381
    EXPECT(szgi::collect_cap(1048576, 96, true, 0) == 87381);
    EXPECT(szgi::collect_cap(1048576, 32, true, 0) == 262144);
    EXPECT(szgi::collect_cap(1048576, 16, true, 0) == 524288);
    EXPECT(szgi::collect_cap(1048576, 1, true, 0) == 1048576);  // (one query: 8M is beyond the ceiling)
    EXPECT(szgi::collect_cap(1048576, 16, false, 0) == 1048576);  // (no limit where every query has its own sweep)
    EXPECT(szgi::collect_cap(1048576, 96, false, 0) == 1048576);
    // room for the staged head and 1024 more, by doubling
    EXPECT(szgi::collect_cap(0, 4, true, 1) == 2048);
    EXPECT(szgi::collect_cap(0, 4, true, 1024) == 2048);
    EXPECT(szgi::collect_cap(0, 4, true, 1025) == 4096);
    EXPECT(szgi::collect_cap(0, 4, true, 3000) == 4096);
    EXPECT(szgi::collect_cap(1500, 4, true, 3000) == 6000);
    EXPECT(szgi::collect_cap(1048576, 96, true, 4096) == 87381);
    EXPECT(szgi::collect_cap(1048576, 96, true, 90000) == 174762);  // (the head outranks the batch limit)

    // the cap a context carries from batch to batch: {largest counter of the batch, radius_cap afterwards}
    const size_t seq[][2] = {
        {300, 1024},         // 375 -> 1024 (a fresh context: 0)
        {1000, 2048},        // 1250 -> 2048
        {30000, 65536},      // 37500 -> 65536
        {25, 57344},         // 1024, but an eighth down at most: 65536 - 8192
        {25, 50176},         // 57344 - 7168
        {25, 43904},         // 50176 - 6272
        {40000, 65536},      // 50000 -> 65536 (43904 - 5488 = 38416 is below)
        {900000, 1048576},   // 1125000 -> the ceiling
        {5000000, 1048576},  // ... and never beyond it
        {0, 917504},         // 1048576 - 131072
        {1638, 802816},      // 917504 - 114688 (2047 -> 2048 is below)
    };
    size_t cap = 0;
    for (const auto &step : seq) {
        cap = szgi::collect_next_cap(cap, step[0]);
        EXPECT(cap == step[1]);
    }
    // the powers of two's edges, and the floor
    EXPECT(szgi::collect_next_cap(0, 0) == 1024);
    EXPECT(szgi::collect_next_cap(0, 819) == 1024);   // 819 + 204 = 1023
    EXPECT(szgi::collect_next_cap(0, 820) == 2048);   // 820 + 205 = 1025
    EXPECT(szgi::collect_next_cap(0, 1638) == 2048);  // 1638 + 409 = 2047
    EXPECT(szgi::collect_next_cap(0, 1639) == 2048);  // 1639 + 409 = 2048
    EXPECT(szgi::collect_next_cap(0, 1640) == 4096);  // 1640 + 410 = 2050
    EXPECT(szgi::collect_next_cap(1100, 0) == 1024);  // 1100 - 137 = 963: the floor
    EXPECT(szgi::collect_next_cap(1024, 0) == 1024);
    EXPECT(szgi::collect_next_cap(1048576, 838860) == 1048576);  // 838860 + 209715 = 1048575
    EXPECT(szgi::collect_next_cap(1048576, 4294967295u) == 1048576);  // (a counter as high as it can go)

    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("collect plan ok\n");
    return 0;
}
