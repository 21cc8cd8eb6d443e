// Stand-alone check of syzgydb_amd/csrc/column_str.h (no HIP, its own main): the predicate the text-column kernel runs,
// against a byte-by-byte restatement, and the size arithmetic of the byte heap.
//
// Every value of length 0..6 over {0x00, 'a', 0xff} against every constant of length 0..4 over the same bytes, for all
// nine operators, with the value at each of the 16 byte alignments of a heap that is allocated EXACTLY as the library
// sizes it (str_heap_capacity: the used bytes rounded up to 16, plus 16, the slack zero) -- a dword fetched past it is a
// heap overflow the address sanitizer reports, and the fetch functor also refuses every dword that holds no byte of the
// row.  The value is flanked on both sides by the constant itself, so a comparison that ignored the row's bounds would
// find a match there; constants of one repeated byte make such a false match straddle the bound at every depth.  Then a
// few long values and constants.  Build with -fsanitize=address,undefined (tests/test_text_columns_cpu.py does).
#include "../../syzgydb_amd/csrc/column_str.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using bytes = std::basic_string<uint8_t>;

// the fetch of a host heap: aligned dword i, only while it holds a byte of the row [lo, hi)
struct HostFetch {
    const uint8_t *heap;
    uint32_t lo, hi;
    mutable long fetched = 0;
    uint32_t operator()(uint32_t i) const
    {
        if (!(4ull * i < hi && 4ull * i + 4 > lo)) {
            printf("fetch of dword %u, which holds no byte of the row [%u, %u)\n", i, lo, hi);
            exit(1);
        }
        fetched++;
        uint32_t v;
        memcpy(&v, heap + 4ull * i, 4);   // (past the allocation: the sanitizer's report)
        return v;
    }
};

static int naive_compare(const bytes &a, const bytes &b)
{
    const size_t n = a.size() < b.size() ? a.size() : b.size();
    for (size_t i = 0; i < n; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return (a.size() > b.size()) - (a.size() < b.size());
}

static bool naive_at(const bytes &a, size_t at, const bytes &b)
{
    for (size_t i = 0; i < b.size(); i++)
        if (a[at + i] != b[i]) return false;
    return true;
}

static bool naive(int op, const bytes &a, const bytes &b)
{
    switch (op) {
    case 0: return naive_compare(a, b) == 0;
    case 1: return naive_compare(a, b) != 0;
    case 2: return naive_compare(a, b) < 0;
    case 3: return naive_compare(a, b) <= 0;
    case 4: return naive_compare(a, b) > 0;
    case 5: return naive_compare(a, b) >= 0;
    case 6: return a.size() >= b.size() && naive_at(a, 0, b);
    case 7: return a.size() >= b.size() && naive_at(a, a.size() - b.size(), b);
    default:
        for (size_t at = 0; at + b.size() <= a.size(); at++)
            if (naive_at(a, at, b)) return true;
        return false;
    }
}

// the constant as the library uploads it: exactly ceil(m / 4) dwords, the last one zero-padded
static std::vector<uint32_t> dwords_of(const bytes &c)
{
    std::vector<uint32_t> d((c.size() + 3) / 4, 0u);
    if (!c.empty()) memcpy(d.data(), c.data(), c.size());
    return d;
}

static long cases = 0, traps = 0;

// `value` at byte `start` of a heap of its own, the constant before and behind it; all nine operators
static int check(const bytes &value, uint32_t start, const bytes &constant)
{
    const uint64_t used = (uint64_t)start + value.size() + constant.size();
    const uint64_t cap = szgi::str_heap_capacity(used);
    uint8_t *heap = (uint8_t *)calloc(cap, 1);
    const size_t before = constant.size() < start ? constant.size() : start;
    if (before) memcpy(heap + start - before, constant.data() + constant.size() - before, before);
    if (!value.empty()) memcpy(heap + start, value.data(), value.size());
    if (!constant.empty()) memcpy(heap + start + value.size(), constant.data(), constant.size());
    const bytes around(heap + start - before, heap + start + value.size() + constant.size());
    const std::vector<uint32_t> c = dwords_of(constant);
    int bad = 0;
    for (int op = 0; op <= 8 && !bad; op++) {
        HostFetch fetch{heap, start, start + (uint32_t)value.size()};
        const bool got = szgi::str_predicate(op, fetch, start, (uint32_t)value.size(), c.data(), (uint32_t)constant.size());
        const bool want = naive(op, value, constant);
        if (op >= 6 && !want && naive(8, around, constant)) traps++;   // a match if the bounds were ignored
        if (got != want) {
            printf("wrong verdict: op %d start %u len %zu constant len %zu: got %d want %d\n", op, start, value.size(),
                   constant.size(), (int)got, (int)want);
            bad = 1;
        } else if (value.empty() && fetch.fetched) {
            printf("op %d read the heap for an empty row\n", op);
            bad = 1;
        } else if (value.size() < constant.size() && (op == 0 || op == 1 || op >= 6) && fetch.fetched) {
            printf("op %d read the heap where the lengths decide\n", op);
            bad = 1;
        }
        cases++;
    }
    free(heap);
    return bad;
}

static void all_strings(size_t max_len, std::vector<bytes> *out)
{
    const uint8_t alphabet[3] = {0x00, 'a', 0xff};
    out->push_back(bytes());
    for (size_t first = 0, len = 1; len <= max_len; len++) {
        const size_t end = out->size();
        for (size_t i = first; i < end; i++)
            for (uint8_t ch : alphabet) out->push_back((*out)[i] + ch);
        first = end;
    }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bytes random_bytes(size_t n)
{
    bytes b(n, 0);
    for (size_t i = 0; i < n; i++) b[i] = (uint8_t)(next() % 3 ? 'a' + next() % 2 : next());
    return b;
}

#define EXPECT(cond)                                             \
    do {                                                         \
        if (!(cond)) {                                           \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                            \
        }                                                        \
    } while (0)

static int check_sizes()
{
    using namespace szgi;
    // capacity: a multiple of 16, at least 16 bytes past the last used byte, and no more than that
    for (uint64_t used : {0ull, 1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 4095ull, 4096ull, (1ull << 32) - 48}) {
        const uint64_t cap = str_heap_capacity(used);
        EXPECT(cap % 16 == 0 && cap >= used + 16 && cap < used + 32);
    }
    EXPECT(str_heap_capacity(0) == 16 && str_heap_capacity(1) == 32 && str_heap_capacity(16) == 32);
    // the limit: the whole heap, slack included, below 4 GiB
    EXPECT(kStrHeapLimit < (1ull << 32) && kStrHeapLimit % 16 == 0);
    EXPECT(str_heap_fits(0) && str_heap_fits(kStrHeapLimit - 16) && !str_heap_fits(kStrHeapLimit - 15));
    EXPECT(!str_heap_fits(1ull << 32) && !str_heap_fits(~0ull) && !str_heap_fits(~0ull - 14));
    // growth: geometric, never past the limit, never below what is needed
    EXPECT(str_heap_grow(0, 0) == 4096 && str_heap_grow(4096, 4090) == 8192 && str_heap_grow(4096, 100000) == str_heap_capacity(100000));
    EXPECT(str_heap_grow(3ull << 30, (3ull << 30) + 1) == kStrHeapLimit);
    // the rows of a part that must grow: from nothing at least 1024, then at least twice the old room, a multiple of 128
    EXPECT(column_grow_rows(0, 1) == 1024 && column_grow_rows(0, 1024) == 1024 && column_grow_rows(0, 1025) == 1152);
    EXPECT(column_grow_rows(1024, 1025) == 2048 && column_grow_rows(1152, 1153) == 2304 && column_grow_rows(1024, 5000) == 5120);
    EXPECT(column_grow_rows(2048, 4097) == 4224 && column_grow_rows(0, 1000000) == 1000064);
    EXPECT(str_heap_grow(1ull << 20, kStrHeapLimit - 16) == kStrHeapLimit);

    // offsets
    const uint64_t good[] = {0, 0, 3, 3, 10}, not_zero[] = {1, 2, 3}, falls[] = {0, 5, 4, 6};
    EXPECT(str_offsets_valid(good, 4) && str_offsets_valid(good, 0));
    EXPECT(!str_offsets_valid(not_zero, 2) && !str_offsets_valid(falls, 3) && !str_offsets_valid(nullptr, 0));
    EXPECT(str_offsets_valid(falls, 1));

    // the split over 1 to 3 parts at row counts around 0, 1 and 128: rows in order, each part its slice of the bytes
    const uint64_t counts[] = {0, 1, 2, 127, 128, 129};
    for (size_t n_parts = 1; n_parts <= 3; n_parts++)
        for (uint64_t r0 : counts)
            for (uint64_t r1 : counts)
                for (uint64_t r2 : counts)
                    for (uint64_t n : counts) {
                        const uint64_t room[3] = {r0, r1, r2}, used[3] = {0, 7, 1000};
                        uint64_t total_room = 0;
                        for (size_t s = 0; s < n_parts; s++) total_room += room[s];
                        std::vector<uint64_t> offsets(n + 1, 0);
                        for (uint64_t i = 0; i < n; i++) offsets[i + 1] = offsets[i] + next() % 9;
                        uint64_t take[3] = {99, 99, 99}, nbytes[3] = {99, 99, 99};
                        const int rc = str_plan_append(offsets.data(), n, room, used, n_parts, take, nbytes);
                        EXPECT(rc == (n > total_room ? kStrPlanRows : kStrPlanOk));
                        if (rc) continue;
                        uint64_t row = 0, left = n;
                        for (size_t s = 0; s < n_parts; s++) {
                            EXPECT(take[s] == (left < room[s] ? left : room[s]));
                            EXPECT(nbytes[s] == offsets[row + take[s]] - offsets[row]);
                            row += take[s], left -= take[s];
                        }
                        EXPECT(row == n);
                    }
    // the 4 GiB refusal, by sizes alone: one call too large, and a small call onto a heap that is nearly full
    {
        const uint64_t offsets[] = {0, 10, 5000000000ull}, small[] = {0, 10, 20};
        const uint64_t room[2] = {1, 1}, empty[2] = {0, 0}, full[2] = {0, kStrHeapLimit - 16 - 9};
        uint64_t take[2], nbytes[2];
        EXPECT(str_plan_append(offsets, 2, room, empty, 2, take, nbytes) == kStrPlanHeap);
        EXPECT(str_plan_append(small, 2, room, full, 2, take, nbytes) == kStrPlanHeap);
        const uint64_t fits[2] = {0, kStrHeapLimit - 16 - 10};
        EXPECT(str_plan_append(small, 2, room, fits, 2, take, nbytes) == kStrPlanOk && nbytes[1] == 10);
        const uint64_t bad[] = {0, 10, 9};
        EXPECT(str_plan_append(bad, 2, room, empty, 2, take, nbytes) == kStrPlanOffsets);
        const uint64_t wraps[] = {0, 1, ~0ull};   // a length that would wrap a sum
        const uint64_t some[2] = {0, 100};
        EXPECT(str_plan_append(wraps, 2, room, some, 2, take, nbytes) == kStrPlanHeap);
    }
    return 0;
}

int main()
{
    std::vector<bytes> values, constants;
    all_strings(6, &values);
    all_strings(4, &constants);
    for (const bytes &v : values)
        for (uint32_t start = 0; start < 16; start++)
            for (const bytes &c : constants)
                if (check(v, start, c)) return 1;
    if (traps == 0) {
        printf("the flanks never completed a match: the bounds are not tested\n");
        return 1;
    }
    // long values and constants: a match at position 0, in the middle and ending on the last byte, none at all, and a
    // near-match that differs only in its last byte; the comparisons against the value itself and its neighbours
    for (size_t len : {255u, 256u, 257u, 5000u})
        for (size_t m : {255u, 256u})
            for (uint32_t start : {0u, 1u, 2u, 3u, 5u, 15u}) {
                const bytes c = random_bytes(m);
                bytes near = c;
                near[m - 1] ^= 0x80;
                std::vector<size_t> places;
                if (len >= m) places = {0, (len - m) / 2, len - m};
                bytes v = random_bytes(len);
                if (check(v, start, c)) return 1;   // no match planted
                for (size_t at : places) {
                    bytes w = v;
                    w.replace(at, m, c);
                    if (check(w, start, c) || check(w, start, near)) return 1;
                    if (!naive(8, w, c) || (at == 0) != naive(6, w, c) || (at == len - m) != naive(7, w, c)) {
                        printf("the planted match is not where it should be\n");
                        return 1;
                    }
                }
                // == and the ordering: the value against itself, a prefix, an extension and a last-byte change
                const bytes head = v.substr(0, len < m ? len : m);
                bytes last = head;
                last[last.size() - 1] ^= 0x01;
                if (check(head, start, head) || check(head, start, last) || check(head.substr(0, head.size() - 1), start, head) ||
                    check(v, start, head))
                    return 1;
            }
    if (check_sizes()) return 1;
    printf("column str ok: %ld cases, %ld of them with a match just outside the row\n", cases, traps);
    return 0;
}
