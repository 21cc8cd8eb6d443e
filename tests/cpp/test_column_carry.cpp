// Stand-alone check of syzgydb_amd/csrc/column_carry.h (no HIP, its own main): what the carry of a text column across a
// compaction / reorder computes -- the piece-to-row search and byte assembly the kernel runs, the grouping of a
// destination part's rows by source part, the staging windows and the capacity arithmetic.
//
// The byte mover runs on an OLD heap allocated EXACTLY as the library sizes it (str_heap_capacity: the used bytes
// rounded up to 16, plus 16 zero bytes), so a dword fetched past it is a heap overflow the address sanitizer reports;
// the fetch functor also refuses every dword that holds no byte of a carried row.  The new bytes are compared with a
// memcpy restatement piece by piece.  Build with -fsanitize=address,undefined (tests/test_column_carry_cpu.py does).
#include "../../syzgydb_amd/csrc/column_carry.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

using namespace szgi;

#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("%s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            exit(1);                                                \
        }                                                           \
    } while (0)

// an old heap: rows laid out with gaps (dead bytes) between them, every byte of the heap distinct from its neighbours
struct OldHeap {
    uint8_t *bytes = nullptr;   // malloc'ed with exactly `cap` bytes
    uint64_t used = 0, cap = 0;
    std::vector<uint64_t> refs;   // per old row {start, len}
    ~OldHeap() { free(bytes); }
};

// rows of the given lengths; row i starts `gap[i]` dead bytes behind the end of row i - 1 (the first at gap[0])
static void build_heap(const std::vector<uint32_t> &lens, const std::vector<uint32_t> &gaps, OldHeap *h)
{
    uint64_t at = 0;
    h->refs.clear();
    for (size_t i = 0; i < lens.size(); i++) {
        at += gaps[i];
        h->refs.push_back(at | ((uint64_t)lens[i] << 32));
        at += lens[i];
    }
    h->used = at;
    h->cap = str_heap_capacity(at);
    h->bytes = (uint8_t *)malloc(h->cap);
    memset(h->bytes, 0, h->cap);
    for (uint64_t i = 0; i < at; i++) h->bytes[i] = (uint8_t)(1 + (i * 7 + i / 251) % 255);   // never 0: dead bytes too
}

// the fetch of the old heap: aligned dword i, only while it holds a byte of a CARRIED row
struct CarriedFetch {
    const OldHeap *h;
    const std::vector<uint8_t> *carried;   // per byte of the heap: 1 = a byte of a carried row
    mutable long fetched = 0;
    uint32_t operator()(uint32_t i) const
    {
        bool ok = false;
        for (uint64_t b = 4ull * i; b < 4ull * i + 4 && b < carried->size(); b++) ok |= (*carried)[b] != 0;
        if (!ok) {
            printf("fetch of dword %u, which holds no byte of a carried row\n", i);
            exit(1);
        }
        fetched++;
        uint32_t v;
        memcpy(&v, h->bytes + 4ull * i, 4);   // (past the allocation: the sanitizer's report)
        return v;
    }
};

// the starts behind a pointer to exactly n entries, every read counted
struct CountedStarts {
    const uint64_t *at;
    mutable long reads = 0;
    uint64_t operator[](uint64_t j) const
    {
        reads++;
        return at[j];
    }
};

static long pieces_checked = 0;

// carry the rows `list` of the heap: starts by a host prefix sum, every piece (and `extra` pieces behind the last)
// against memcpy
static void check_carry(const OldHeap &h, const std::vector<uint64_t> &list, uint64_t extra)
{
    const uint64_t n = list.size();
    std::vector<uint64_t> refs(n), starts(n);
    std::vector<uint8_t> carried((size_t)h.cap, 0);
    uint64_t total = 0;
    for (uint64_t j = 0; j < n; j++) {
        refs[j] = h.refs[list[j]];
        starts[j] = total;
        total += refs[j] >> 32;
        for (uint64_t b = 0; b < (refs[j] >> 32); b++) carried[(uint32_t)refs[j] + b] = 1;
    }
    std::vector<uint8_t> want((size_t)(((total + 15) / 16 + extra) * 16), 0);
    for (uint64_t j = 0; j < n; j++)
        if (refs[j] >> 32) memcpy(want.data() + starts[j], h.bytes + (uint32_t)refs[j], refs[j] >> 32);
    CarriedFetch fetch{&h, &carried};
    // exactly n entries behind the pointers: an index past the rows is the sanitizer's report
    uint64_t *refs_exact = (uint64_t *)malloc(n ? n * 8 : 1), *starts_exact = (uint64_t *)malloc(n ? n * 8 : 1);
    if (n) memcpy(refs_exact, refs.data(), n * 8), memcpy(starts_exact, starts.data(), n * 8);
    // what a piece may read of the starts: the search for its first row, and per row that begins inside it (at most 15
    // of them hold a byte) kCarryWalk steps and one search more -- whatever the runs of empty rows between them
    uint64_t depth = 1;
    while ((1ull << depth) < n + 1) depth++;
    const long reads_allowed = (long)(16 * (depth + 1 + kCarryWalk + 1));
    CountedStarts counted{starts_exact};
    for (uint64_t p = 0; p < want.size() / 16; p++) {
        uint32_t out[4];
        const long before = fetch.fetched, reads_before = counted.reads;
        carry_piece(fetch, refs_exact, counted, n, total, p, out);
        CHECK(memcmp(out, want.data() + 16 * p, 16) == 0);
        CHECK(counted.reads - reads_before <= reads_allowed);
        CHECK(fetch.fetched - before <= 16);   // (at most one dword per byte, in fact at most 5 for a piece of one row)
        if (16 * p >= total) CHECK(fetch.fetched == before);
        pieces_checked++;
    }
    for (uint64_t pos = 0; pos < total; pos++) {   // the search alone: the row that holds byte pos
        const uint64_t j = carry_row_at(starts_exact, n, pos);
        CHECK(j < n && starts[j] <= pos && (j + 1 == n || starts[j + 1] > pos));
    }
    free(refs_exact);
    free(starts_exact);
}

static void test_byte_mover()
{
    const std::vector<uint32_t> kLens = {0, 1, 3, 4, 5, 15, 16, 17, 33, 300, 4998};
    for (uint32_t align = 0; align < 4; align++) {
        // every length at old start = align (mod 4), twice over so that rows of every length follow each other
        std::vector<uint32_t> lens, gaps;
        for (int rep = 0; rep < 2; rep++)
            for (size_t i = 0; i < kLens.size(); i++) {
                const uint32_t len = rep ? kLens[kLens.size() - 1 - i] : kLens[i];
                const uint64_t end = std::accumulate(lens.begin(), lens.end(), 0ull) + std::accumulate(gaps.begin(), gaps.end(), 0ull);
                lens.push_back(len);
                gaps.push_back((uint32_t)((align + 4 - end % 4) % 4));   // (dead bytes: the start lands on the alignment)
            }
        OldHeap h;
        build_heap(lens, gaps, &h);
        for (uint64_t r : h.refs) CHECK(((uint32_t)r & 3) == align);
        const uint64_t rows = lens.size();
        std::vector<uint64_t> all(rows), reversed, gapped, single;
        std::iota(all.begin(), all.end(), 0);
        reversed.assign(all.rbegin(), all.rend());
        for (uint64_t r = 0; r < rows; r += 2) gapped.push_back(rows - 1 - r);   // reversed AND with gaps
        check_carry(h, all, 2);
        check_carry(h, reversed, 1);
        check_carry(h, gapped, 1);
        for (uint64_t r = 0; r < rows; r += 3) single.push_back(r);
        check_carry(h, single, 0);
        for (uint64_t r = 0; r < rows; r++) check_carry(h, {r}, 1);   // one row alone, every length
        check_carry(h, {}, 2);                                        // no row at all: zeros, nothing fetched
        // the last old row ends exactly at the used bytes; carried alone and last in a list
        CHECK((uint32_t)h.refs[rows - 1] + (h.refs[rows - 1] >> 32) == h.used);
        check_carry(h, {0, 5, rows - 1}, 0);
    }
    // the last value ends exactly at the used bytes for every length and alignment, the heap holding nothing else but
    // the dead bytes in front of it: the mover's last dword is the heap's last used one
    for (uint32_t len : kLens)
        for (uint32_t align = 0; align < 4; align++) {
            OldHeap h;
            build_heap({len}, {align}, &h);
            check_carry(h, {0}, 1);
            OldHeap h2;
            build_heap({7, len}, {align, 0}, &h2);
            check_carry(h2, {1, 0}, 0);
            check_carry(h2, {1}, 0);
        }
    // runs of empty rows in front of, between and behind the others
    OldHeap h;
    build_heap({0, 0, 5, 0, 0, 0, 17, 0}, {0, 0, 0, 3, 0, 0, 1, 0}, &h);
    check_carry(h, {0, 1, 2, 3, 4, 5, 6, 7}, 1);
    check_carry(h, {7, 6, 5, 4, 3, 2, 1, 0}, 1);
    check_carry(h, {0, 1, 3, 4, 5, 7}, 1);   // nothing but empty rows: total 0
    // long runs of empty rows (a sparse field): a lane searches again, it does not walk the run (reads_allowed)
    std::vector<uint32_t> lens(5000, 0), gaps(5000, 0);
    for (size_t i : {0, 1, 2, 3, 1200, 1201, 1206, 1207, 4000, 4999}) lens[i] = 3;
    lens[4000] = 40;
    OldHeap sparse;
    build_heap(lens, gaps, &sparse);
    std::vector<uint64_t> every(lens.size()), back;
    std::iota(every.begin(), every.end(), 0);
    back.assign(every.rbegin(), every.rend());
    check_carry(sparse, every, 1);
    check_carry(sparse, back, 1);
}

static void test_grouping_and_windows()
{
    for (size_t parts = 1; parts <= 3; parts++) {
        // parts of 64, 128 and 37 rows; the list interleaves them row by row, from each part's last row down
        const uint64_t sizes[3] = {64, 128, 37};
        std::vector<uint64_t> first(parts), rows(parts);
        uint64_t total = 0;
        for (size_t s = 0; s < parts; s++) first[s] = total, rows[s] = sizes[s], total += sizes[s];
        std::vector<uint64_t> list;
        for (uint64_t i = 0; i < 128; i++)
            for (size_t s = 0; s < parts; s++)
                if (i < rows[s]) list.push_back(first[s] + rows[s] - 1 - i);
        CHECK(list.size() == total);
        std::vector<std::vector<uint64_t>> sub, at;
        CHECK(carry_group_rows(list.data(), list.size(), first.data(), rows.data(), parts, &sub, &at));
        std::vector<int> seen(list.size(), 0);
        for (size_t s = 0; s < parts; s++) {
            CHECK(sub[s].size() == rows[s] && at[s].size() == rows[s]);
            for (size_t j = 0; j < sub[s].size(); j++) {
                CHECK(sub[s][j] == rows[s] - 1 - j);                   // part-local, in the list's order
                CHECK(list[at[s][j]] == first[s] + sub[s][j]);         // and where it goes
                CHECK(j == 0 || at[s][j] > at[s][j - 1]);
                seen[at[s][j]]++;
            }
        }
        for (int v : seen) CHECK(v == 1);
        // a sub-list (a destination part's slice), and a row in no part
        CHECK(carry_group_rows(list.data() + 5, 20, first.data(), rows.data(), parts, &sub, &at));
        uint64_t got = 0;
        for (size_t s = 0; s < parts; s++) got += sub[s].size();
        CHECK(got == 20);
        const uint64_t outside = total;
        CHECK(!carry_group_rows(&outside, 1, first.data(), rows.data(), parts, &sub, &at));
        CHECK(carry_group_rows(list.data(), 0, first.data(), rows.data(), parts, &sub, &at) && sub.size() == parts);
    }
    // the windows: they tile [0, n) in order, none empty, none above the window size
    for (uint64_t n : {0ull, 1ull, 7ull, 8ull, 9ull, 64ull})
        for (uint64_t window : {1ull, 8ull, 100ull}) {
            uint64_t lo = 0, hi = 0, next = 0, w = 0;
            for (; carry_window(n, window, w, &lo, &hi); w++) {
                CHECK(lo == next && hi > lo && hi - lo <= window && hi <= n);
                next = hi;
            }
            CHECK(next == n && w == (n + window - 1) / window);
            CHECK(!carry_window(n, window, w + 1, &lo, &hi));
        }
    uint64_t lo, hi;
    CHECK(!carry_window(5, 0, 0, &lo, &hi));
    CHECK(carry_window_rows(kCarryStageBytes, 8) * 8 == kCarryStageBytes && carry_window_rows(kCarryStageBytes, 4) * 4 == kCarryStageBytes);
    CHECK(carry_window_pieces(kCarryStageBytes) * 16 == kCarryStageBytes);
    for (uint64_t stage : {16ull, 4096ull})   // the smallest windows the handle's test hook allows: none is empty
        CHECK(carry_window_rows(stage, 8) >= 1 && carry_window_rows(stage, 4) >= 1 && carry_window_pieces(stage) >= 1);
}

static void test_capacities()
{
    // a carried heap is sized as a fresh column's: str_heap_capacity(used), at least the first growth step
    CHECK(carry_heap_capacity(0) == 4096 && carry_heap_capacity(1) == 4096 && carry_heap_capacity(4080) == 4096);
    CHECK(carry_heap_capacity(4081) == 4112);
    for (uint64_t used : {0ull, 5ull, 4079ull, 4080ull, 4081ull, 100000ull, 24900000ull, (unsigned long long)kStrHeapLimit - 32}) {
        const uint64_t cap = carry_heap_capacity(used);
        CHECK(cap % 16 == 0 && cap >= str_heap_capacity(used) && cap >= used + 16 && cap <= kStrHeapLimit);
        CHECK(cap == std::max<uint64_t>(str_heap_capacity(used), 4096));
        CHECK(cap == str_heap_grow(0, used));   // what szg_column_create_str allocates for these bytes
    }
    // the 4 GiB limit, group by group
    CHECK(carry_heap_takes(0, 0) && carry_heap_takes(0, kStrHeapLimit - 32));
    CHECK(!carry_heap_takes(0, kStrHeapLimit - 15) && !carry_heap_takes(0, 1ull << 32) && !carry_heap_takes(0, ~0ull));
    CHECK(carry_heap_takes(1ull << 31, (1ull << 31) - 64) && !carry_heap_takes(1ull << 31, 1ull << 31));
    CHECK(!carry_heap_takes(kStrHeapLimit - 32, 17));
    // rows: part_reserve's rule for a part that starts empty
    CHECK(carry_cap_rows(0) == 0 && carry_cap_rows(1) == 1024 && carry_cap_rows(1024) == 1024);
    CHECK(carry_cap_rows(1025) == 1152 && carry_cap_rows(70000) == 70016);
    for (uint64_t n : {1ull, 1000ull, 1024ull, 1025ull, 99999ull}) CHECK(carry_cap_rows(n) % 128 == 0 && carry_cap_rows(n) >= n);
}

int main()
{
    test_byte_mover();
    test_grouping_and_windows();
    test_capacities();
    printf("column carry ok: %ld pieces\n", pieces_checked);
    return 0;
}
