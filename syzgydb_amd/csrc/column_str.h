// column_str.h -- the text columns (SZG_COL_STR) of scan_column.cpp / kernels_column.hip: the per-row predicate and the
// size arithmetic of the byte heap.  A row is an 8-byte reference {uint32 start, uint32 len} into its part's heap; the
// predicate reads the heap through a functor `fetch(i)` = the aligned dword at byte 4 i, so the same code is the
// kernel's (a global load) and a host program's (tests/cpp/test_column_str.cpp runs it under the sanitizers on a heap
// sized exactly as the library sizes it).  No HIP runtime in here; plain C++ either way.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SZG_STR_HD __host__ __device__ __forceinline__
#else
#define SZG_STR_HD inline
#endif

namespace szgi {

// operators: SZG_CMP_EQ..SZG_CMP_GE = 0..5, then SZG_STR_STARTS_WITH / ENDS_WITH / CONTAINS (include/syzgy_scan.h)
constexpr int kStrOpEq = 0, kStrOpNe = 1, kStrOpLt = 2, kStrOpLe = 3, kStrOpGt = 4, kStrOpGe = 5;
constexpr int kStrOpStartsWith = 6, kStrOpEndsWith = 7, kStrOpContains = 8;
constexpr uint32_t kStrPatternMax = 256;                   // bytes of a constant
constexpr uint32_t kStrPatternDwords = kStrPatternMax / 4; // the constant as dwords, zero-padded behind its last byte

// ---- the predicate --------------------------------------------------------------------------------------------------

// Bytes [pos, pos + n) of the heap against the first n bytes of the constant c (dwords, little-endian): 0 when equal,
// else < 0 / > 0 as the heap's bytes sort before / after, bytes compared as unsigned.  Stops at the first differing
// dword.  Every dword it fetches holds at least one byte of [pos, pos + n); n == 0 fetches nothing.
template <class Fetch>
SZG_STR_HD int str_compare(const Fetch &fetch, uint32_t pos, uint32_t n, const uint32_t *c)
{
    if (n == 0) return 0;
    const uint32_t off = pos & 3, a = pos >> 2;
    uint32_t lo = fetch(a);
    for (uint32_t j = 0; 4 * j < n; j++) {
        const uint32_t rem = n - 4 * j;   // bytes of this unit onwards, > 0
        uint32_t hi = 0;
        if (rem > 4 || off + rem > 4) hi = fetch(a + j + 1);   // (the next unit's first dword, or this unit's spill)
        uint32_t u = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * off));   // funnel shift: 4 bytes from pos + 4 j
        uint32_t k = c[j];
        if (rem < 4) {
            const uint32_t keep = (1u << (8 * rem)) - 1u;
            u &= keep, k &= keep;
        }
        if (u != k) return __builtin_bswap32(u) < __builtin_bswap32(k) ? -1 : 1;   // the first byte decides
        lo = hi;
    }
    return 0;
}

// op(value, constant) for the value at [start, start + len) of the heap and the constant's m bytes in c[0 .. ceil(m/4))
// (c[m / 4]'s bytes behind the constant's last are 0).  Go's rules for strings (query/compiler.go:304-319, :393-418):
// unsigned, lexicographic, a proper prefix is the smaller; the string operators with "" hold for every value.  Reads
// only dwords that hold a byte of the value, and none where the lengths decide.
template <class Fetch>
SZG_STR_HD bool str_predicate(int op, const Fetch &fetch, uint32_t start, uint32_t len, const uint32_t *c, uint32_t m)
{
    switch (op) {
    case kStrOpEq: return len == m && str_compare(fetch, start, m, c) == 0;
    case kStrOpNe: return len != m || str_compare(fetch, start, m, c) != 0;
    case kStrOpStartsWith: return len >= m && str_compare(fetch, start, m, c) == 0;
    case kStrOpEndsWith: return len >= m && str_compare(fetch, start + (len - m), m, c) == 0;
    case kStrOpContains: {
        if (m == 0) return true;
        if (len < m) return false;
        // the constant's first min(m, 4) bytes against every position, the rest only where they match
        const uint32_t keep = m < 4 ? (1u << (8 * m)) - 1u : ~0u;
        const uint32_t first = c[0] & keep;
        const uint32_t last = start + (len - m);   // the last position a match can start at
        uint32_t lo = fetch(start >> 2), hi = 0;
        // dword (pos >> 2) + 1 is fetched while a candidate at pos needs it: it begins at most 4 bytes behind pos, and
        // a candidate spans m >= 1 bytes of the value, so when pos's 4-byte window spills over it the dword is either
        // part of the value or masked off below -- fetched only when it holds a byte of the value
        const uint32_t end = start + len;          // one past the value's last byte
        if (((start >> 2) + 1) * 4 < end) hi = fetch((start >> 2) + 1);
        for (uint32_t pos = start;; ) {
            const uint32_t u = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (pos & 3)));
            if ((u & keep) == first && (m <= 4 || str_compare(fetch, pos + 4, m - 4, c + 1) == 0)) return true;
            if (pos == last) return false;
            pos++;
            if ((pos & 3) == 0) {
                lo = hi, hi = 0;
                if (((pos >> 2) + 1) * 4 < end) hi = fetch((pos >> 2) + 1);
            }
        }
    }
    default: {
        const int r0 = str_compare(fetch, start, len < m ? len : m, c);
        const int r = r0 ? r0 : (len > m) - (len < m);
        return op == kStrOpLt ? r < 0 : op == kStrOpLe ? r <= 0 : op == kStrOpGt ? r > 0 : r >= 0;
    }
    }
}

// ---- sizes and limits (host) ----------------------------------------------------------------------------------------

// A part's heap stays below 4 GiB, its zero-filled slack included: starts and lengths are uint32.
constexpr uint64_t kStrHeapLimit = (1ull << 32) - 16;

// the smallest capacity for `used` bytes: a multiple of 16 that ends at least 16 bytes past the last used byte
inline uint64_t str_heap_capacity(uint64_t used) { return ((used + 15) & ~15ull) + 16; }

// whether a heap may hold `used` bytes at all
inline bool str_heap_fits(uint64_t used) { return used <= kStrHeapLimit && str_heap_capacity(used) <= kStrHeapLimit; }

// the capacity to allocate when `cap` bytes no longer hold `used` (str_heap_fits(used)): at least twice the old one
inline uint64_t str_heap_grow(uint64_t cap, uint64_t used)
{
    const uint64_t want = std::max<uint64_t>(std::max(str_heap_capacity(used), 2 * cap), 4096);
    return std::min(want, kStrHeapLimit);
}

// the rows to allocate when a part with room for `cap_rows` rows must hold `need` > cap_rows: at least twice the old
// capacity and at least 1024, a multiple of 128
inline uint64_t column_grow_rows(uint64_t cap_rows, uint64_t need)
{
    return (std::max<uint64_t>(std::max<uint64_t>(need, 2 * cap_rows), 1024) + 127) & ~127ull;
}

// offsets[0 .. n_rows]: starts at 0 and never decreases
inline bool str_offsets_valid(const uint64_t *offsets, uint64_t n_rows)
{
    if (!offsets || offsets[0] != 0) return false;
    for (uint64_t i = 0; i < n_rows; i++)
        if (offsets[i + 1] < offsets[i]) return false;
    return true;
}

// n rows over parts in order, part s taking at most room[s]: take[s] rows each; returns the rows left over
inline uint64_t split_rows(const uint64_t *room, size_t n_parts, uint64_t n, uint64_t *take)
{
    for (size_t s = 0; s < n_parts; s++) {
        take[s] = std::min(n, room[s]);
        n -= take[s];
    }
    return n;
}

enum { kStrPlanOk = 0, kStrPlanOffsets = 1, kStrPlanRows = 2, kStrPlanHeap = 3 };

// What an append of n_rows strings does to each part, before anything is allocated: part s takes take[s] rows (by
// split_rows over room[]) and bytes[s] bytes -- its rows' slice of the call's bytes, back to back -- behind the
// used[s] bytes its heap holds.  kStrPlanOffsets: bad offsets; kStrPlanRows: more rows than the parts have room for;
// kStrPlanHeap: a part's heap would reach the 4 GiB limit.
inline int str_plan_append(const uint64_t *offsets, uint64_t n_rows, const uint64_t *room, const uint64_t *used,
                           size_t n_parts, uint64_t *take, uint64_t *bytes)
{
    if (!str_offsets_valid(offsets, n_rows)) return kStrPlanOffsets;
    if (split_rows(room, n_parts, n_rows, take)) return kStrPlanRows;
    uint64_t row = 0;
    for (size_t s = 0; s < n_parts; s++) {
        bytes[s] = offsets[row + take[s]] - offsets[row];
        row += take[s];
        if (bytes[s] > kStrHeapLimit || !str_heap_fits(used[s] + bytes[s])) return kStrPlanHeap;
    }
    return kStrPlanOk;
}

}  // namespace szgi
