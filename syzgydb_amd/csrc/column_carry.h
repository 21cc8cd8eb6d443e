// column_carry.h -- columns carried across a compaction / reorder (scan_column_carry.cpp / kernels_column_carry.hip):
// the index arithmetic of the text heap's repack, the grouping of a destination part's rows by source part, the sizes of
// the staging windows and the heap's capacity afterwards.  Like column_str.h it is plain C++ either way: the kernel and a
// host program (tests/cpp/test_column_carry.cpp, under the sanitizers on heaps sized exactly as the library sizes them)
// run the same code.  The heaps are read through a functor `fetch(i)` = the aligned dword at byte 4 i.
//
// The repack of one group of rows: row j of the group has the reference refs[j] = {uint32 old start, uint32 len} into
// the OLD heap and the 64-bit new start starts[j] = len[0] + ... + len[j - 1] (an exclusive prefix sum: monotone); the
// group's bytes, back to back, are `total` bytes.  The new bytes are produced in 16-byte pieces: piece p holds the new
// bytes [16 p, 16 p + 16), those at or behind `total` as zero.
#pragma once
#include "column_str.h"

#include <vector>

namespace szgi {

// ---- the byte mover -------------------------------------------------------------------------------------------------

// The last row j < n with starts[j] <= pos (starts[0] == 0, so there is one): a binary search over the monotone starts.
// Rows of length 0 share their start with the row behind them; the last of such a run is returned.
template <class Starts>
SZG_STR_HD uint64_t carry_row_at(const Starts &starts, uint64_t n, uint64_t pos)
{
    uint64_t lo = 0, hi = n;   // starts[lo] <= pos < starts[hi] (starts[n] = +inf)
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (starts[mid] <= pos) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Rows that end at or before a position are stepped over one by one this many times, then searched for again: a run of
// empty rows (absent rows have length 0, so a sparse text field is full of them) costs a lane one more binary search,
// not a walk of the run's length.
constexpr uint32_t kCarryWalk = 4;

// Piece `piece` of the group's new bytes into out[0 .. 4) (little-endian dwords).  The rows that cover the piece are
// found by carry_row_at, then walked (kCarryWalk); each output dword takes its bytes of a row from one or two aligned
// dwords of the old heap through a funnel shift.  A dword of the old heap is fetched only when it holds a byte of a carried value (the
// rule of column_str.h: the heap's 16 zero bytes of slack are what makes the last dword of the last value legal), and
// at most once in a row of consecutive uses.  n == 0 or 16 piece >= total: zeros, nothing fetched.
template <class Fetch, class Refs, class Starts>
SZG_STR_HD void carry_piece(const Fetch &fetch, const Refs &refs, const Starts &starts, uint64_t n, uint64_t total,
                            uint64_t piece, uint32_t out[4])
{
    out[0] = out[1] = out[2] = out[3] = 0u;
    const uint64_t begin = piece * 16;
    if (n == 0 || begin >= total) return;
    const uint64_t end = begin + 16 < total ? begin + 16 : total;
    uint64_t j = carry_row_at(starts, n, begin);
    uint64_t row_start = starts[j], ref = refs[j];
    uint32_t cached_at = 0xFFFFFFFFu, cached = 0;   // the dword fetched last (no dword of a heap has this index)
    for (uint64_t pos = begin; pos < end;) {
        uint32_t walked = 0;
        while (row_start + (ref >> 32) <= pos) {   // rows that end at or before pos (pos < total: j stays < n)
            j = ++walked <= kCarryWalk ? j + 1 : carry_row_at(starts, n, pos);   // (the row that holds pos: the loop ends)
            row_start = starts[j], ref = refs[j];
        }
        const uint64_t row_end = row_start + (ref >> 32);
        const uint64_t seg_end = row_end < end ? row_end : end;   // bytes [pos, seg_end) come from row j
        // the output dword that holds byte pos, and its bytes [b0, b1) that row j fills
        const uint32_t k = (uint32_t)(pos - begin) >> 2;
        const uint32_t b0 = (uint32_t)(pos - begin) & 3;
        const uint64_t dword_end = begin + 4 * (uint64_t)k + 4;
        const uint32_t cnt = (uint32_t)((seg_end < dword_end ? seg_end : dword_end) - pos);   // 1 .. 4 - b0
        const uint32_t src = (uint32_t)ref + (uint32_t)(pos - row_start);   // the first of the cnt bytes in the old heap
        const uint32_t a = src >> 2, off = src & 3;
        uint32_t lo = cached;
        if (a != cached_at) lo = fetch(a), cached_at = a, cached = lo;
        uint32_t hi = 0;
        if (off + cnt > 4) hi = fetch(a + 1), cached_at = a + 1, cached = hi;   // (holds byte src + cnt - 1 of the value)
        uint32_t u = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * off));      // funnel shift: the bytes from src on
        if (cnt < 4) u &= (1u << (8 * cnt)) - 1u;
        out[k] |= u << (8 * b0);
        pos += cnt;
    }
}

// ---- sizes (host) ---------------------------------------------------------------------------------------------------

// What a heap holds after a carry left `used` bytes in it: the capacity a freshly created column of these rows has
// (str_heap_grow from nothing: str_heap_capacity(used), at least the first growth step).  str_heap_fits(used).
inline uint64_t carry_heap_capacity(uint64_t used) { return str_heap_grow(0, used); }

// Whether a destination part may take `more` bytes behind the `used` it has been given so far.
inline bool carry_heap_takes(uint64_t used, uint64_t more) { return more <= kStrHeapLimit && str_heap_fits(used + more); }

// The rows a part has room for after a carry of n_rows rows: column_grow_rows from nothing (no rows, no allocation).
inline uint64_t carry_cap_rows(uint64_t n_rows) { return n_rows ? column_grow_rows(0, n_rows) : 0; }

// Handles of several shards stage what travels between devices in windows: at most stage_bytes of values (or
// references), and at most stage_bytes of a group's bytes in whole pieces, at a time.  kCarryStageBytes unless the
// handle's test hook carry_stage_bytes says less (a multiple of 16, so no window is empty).
constexpr uint64_t kCarryStageBytes = 64ull << 20;
inline uint64_t carry_window_rows(uint64_t stage_bytes, uint64_t elem_bytes) { return stage_bytes / elem_bytes; }
inline uint64_t carry_window_pieces(uint64_t stage_bytes) { return stage_bytes / 16; }

// window w of `n` items in windows of `window`: [*lo, *hi); false once w is past the last
inline bool carry_window(uint64_t n, uint64_t window, uint64_t w, uint64_t *lo, uint64_t *hi)
{
    if (window == 0 || w > n / window || w * window >= n) return false;
    *lo = w * window;
    *hi = n - *lo < window ? n : *lo + window;
    return true;
}

// ---- grouping (host) ------------------------------------------------------------------------------------------------

// The rows of one destination part by the source part that holds them.  list[0 .. m) = the old rows (handle-level) that
// become the destination's rows 0 .. m - 1; part s of the source covers old rows [first[s], first[s] + rows[s]).
// sub[s] = the rows of part s among them, part-local, in the list's order; at[s] = where in the destination each goes.
// false: a listed row lies in no part.
inline bool carry_group_rows(const uint64_t *list, uint64_t m, const uint64_t *first, const uint64_t *rows, size_t n_parts,
                             std::vector<std::vector<uint64_t>> *sub, std::vector<std::vector<uint64_t>> *at)
{
    sub->assign(n_parts, {});
    at->assign(n_parts, {});
    size_t s = 0;   // (the part of the previous row: lists are mostly runs)
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t r = list[i];
        if (!(s < n_parts && r >= first[s] && r - first[s] < rows[s])) {
            for (s = 0; s < n_parts; s++)
                if (r >= first[s] && r - first[s] < rows[s]) break;
            if (s == n_parts) return false;
        }
        (*sub)[s].push_back(r - first[s]);
        (*at)[s].push_back(i);
    }
    return true;
}

}  // namespace szgi
