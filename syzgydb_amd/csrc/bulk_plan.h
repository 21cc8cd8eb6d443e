// bulk_plan.h -- the host-only part of the bulk mutations (scan_bulk.cpp: szg_index_overwrite_rows, its _f64 form,
// szg_index_tombstone_rows, szg_column_set_rows): the validation of a caller's row list and its split into per-shard
// lists -- the one place the library reads such a list unchecked.  Plain C++, no HIP, like reorder_plan.h:
// szg_debug_bulk_plan runs it without a device, and tests/cpp/test_bulk_plan.cpp compiles it on its own under the
// address and undefined-behaviour sanitizers.
#pragma once
#include "../../include/syzgy_scan.h"

#include <cstddef>
#include <cstdint>
#include <vector>

namespace szgi {

// What a checked list becomes: per shard (or column part) the listed rows that fall into it, shard-local, in the
// caller's order, and beside each the position it had in the caller's list -- entry source[s][j] of the caller's data
// belongs to row local[s][j].  word_lo[s] .. word_hi[s]: the first and last 64-row word of the shard that holds a
// listed row (what a tombstone call uploads); word_lo[s] > word_hi[s]: the shard is not touched.
struct BulkPlan {
    std::vector<std::vector<uint64_t>> local, source;
    std::vector<uint64_t> word_lo, word_hi;
};

// rows[i] - row_base is a row of the n_shards contiguous ranges [first[s], first[s] + count[s]) (empty ranges are
// skipped; the rows they hold together are [0, sum of the counts)): SZG_E_RANGE ("row out of range") otherwise.  With
// allow_duplicates == 0 a row listed twice is SZG_E_INVALID ("row listed twice"): a scatter then never has two
// writers to one row.  On SZG_OK *out holds the split; otherwise *error names the fault and *out is not to be used.
inline int bulk_plan(const uint64_t *first, const uint64_t *count, size_t n_shards, uint64_t row_base, const uint64_t *rows,
                     uint64_t n, int allow_duplicates, BulkPlan *out, const char **error)
{
    *error = "";
    if (n_shards == 0 || !first || !count) return *error = "no shards", SZG_E_INVALID;
    if (!rows && n) return *error = "null argument", SZG_E_INVALID;
    uint64_t n_rows = 0;
    for (size_t s = 0; s < n_shards; s++)
        if (count[s]) n_rows = first[s] + count[s];
    for (uint64_t i = 0; i < n; i++)  // (all of the range check first: a list with both faults is out of range)
        if (rows[i] < row_base || rows[i] - row_base >= n_rows) return *error = "row out of range", SZG_E_RANGE;
    out->local.assign(n_shards, {});
    out->source.assign(n_shards, {});
    out->word_lo.assign(n_shards, UINT64_MAX);
    out->word_hi.assign(n_shards, 0);
    std::vector<uint64_t> seen;
    if (!allow_duplicates) {
        if (n > n_rows) return *error = "row listed twice", SZG_E_INVALID;
        seen.assign((size_t)((n_rows + 63) / 64), 0ull);
    }
    size_t s = 0;  // (lists are mostly sorted or clustered: start the search at the last entry's shard)
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t r = rows[i] - row_base;
        if (!allow_duplicates) {
            const uint64_t bit = 1ull << (r & 63);
            if (seen[(size_t)(r >> 6)] & bit) return *error = "row listed twice", SZG_E_INVALID;
            seen[(size_t)(r >> 6)] |= bit;
        }
        if (!(count[s] && r >= first[s] && r - first[s] < count[s])) {
            for (s = 0; s < n_shards; s++)
                if (count[s] && r >= first[s] && r - first[s] < count[s]) break;
            if (s == n_shards) return *error = "row out of range", SZG_E_RANGE;  // (a gap between the ranges)
        }
        const uint64_t l = r - first[s];
        out->local[s].push_back(l);
        out->source[s].push_back(i);
        if (l / 64 < out->word_lo[s]) out->word_lo[s] = l / 64;
        if (l / 64 > out->word_hi[s]) out->word_hi[s] = l / 64;
    }
    return SZG_OK;
}

}  // namespace szgi
