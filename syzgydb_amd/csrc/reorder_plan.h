// reorder_plan.h -- the host-only part of szg_index_reorder (scan_reorder.cpp): how rows split over shards, and the
// validation of a caller's row list -- the one place the library reads such a list unchecked.  Plain C++, no HIP:
// szg_debug_reorder_plan runs it without a device, and tests/cpp/test_reorder_plan.cpp compiles it on its own under
// the address and undefined-behaviour sanitizers.
#pragma once
#include "../../include/syzgy_scan.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace szgi {

// rows of an index are split over its shards in contiguous ranges whose boundaries are multiples of 64 (so filter
// words slice cleanly)
inline void split_counts(size_t n_shards, uint64_t n_rows, std::vector<uint64_t> *counts)
{
    counts->assign(n_shards, 0);
    if (n_shards == 0) return;
    uint64_t per = (n_rows + n_shards - 1) / n_shards;
    per = (per + 63) & ~63ull;
    uint64_t left = n_rows;
    for (size_t s = 0; s < n_shards; s++) {
        const uint64_t m = std::min(per, left);
        (*counts)[s] = m;
        left -= m;
    }
}

// The list of a reorder: src_rows[i] - row_base is the old row of new row i.  Every listed row must be one of the
// n_rows old rows (SZG_E_RANGE), live -- bit set in live_words, ceil(n_rows / 64) index-level words; null: every row
// is live -- and listed once (SZG_E_INVALID).  On SZG_OK *local holds the list without the row base and *counts the
// new rows of each shard; otherwise *error names the fault and neither is to be used.
inline int reorder_plan(uint64_t n_rows, const uint64_t *live_words, uint64_t row_base, const uint64_t *src_rows, uint64_t n,
                        size_t n_shards, std::vector<uint64_t> *local, std::vector<uint64_t> *counts, const char **error)
{
    *error = "";
    if (n_shards == 0) return *error = "no shards", SZG_E_INVALID;
    if (!src_rows && n) return *error = "null argument", SZG_E_INVALID;
    if (n > n_rows) {  // (more entries than rows: one is out of range or listed twice -- say which)
        for (uint64_t i = 0; i < n; i++)
            if (src_rows[i] < row_base || src_rows[i] - row_base >= n_rows) return *error = "row out of range", SZG_E_RANGE;
        return *error = "row listed twice", SZG_E_INVALID;
    }
    std::vector<uint64_t> seen((size_t)((n_rows + 63) / 64), 0ull);
    local->resize((size_t)n);
    for (uint64_t i = 0; i < n; i++) {
        if (src_rows[i] < row_base || src_rows[i] - row_base >= n_rows) return *error = "row out of range", SZG_E_RANGE;
        const uint64_t r = src_rows[i] - row_base;
        const uint64_t bit = 1ull << (r & 63);
        if (live_words && !(live_words[r >> 6] & bit)) return *error = "row is tombstoned", SZG_E_INVALID;
        if (seen[(size_t)(r >> 6)] & bit) return *error = "row listed twice", SZG_E_INVALID;
        seen[(size_t)(r >> 6)] |= bit;
        (*local)[(size_t)i] = r;
    }
    split_counts(n_shards, n, counts);
    return SZG_OK;
}

}  // namespace szgi
