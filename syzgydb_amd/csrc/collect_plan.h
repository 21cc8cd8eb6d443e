// collect_plan.h -- the buffer arithmetic of a radius batch (scan_radius.cpp): how many entries each query's collect
// buffer gets, how that follows the hit counts a context has seen, whether the re-ranked hits travel as one block, and
// where each query's list lies in the pinned buffer once the counters are known: every index into d_collect, d_out,
// d_count and h_out of such a batch.  Plain C++, no HIP, like bulk_plan.h and reorder_plan.h:
// tests/cpp/test_collect_plan.cpp compiles it on its own under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace szgi {

constexpr size_t kRadiusCapMin = 1024;              // entries per query a batch's buffers start with
constexpr size_t kRadiusCapMax = 1u << 20;          // beyond this a query is answered on its own (run_collect, a hand-over)
constexpr size_t kRadiusBatchEntries = 8u << 20;    // a limited batch's buffers: this many entries at most
constexpr size_t kRadiusBlockCopyBytes = 2u << 20;  // a batch's re-ranked hits travel as one block up to this size,
constexpr size_t kRadiusListCopyBytes = 64u << 10;  // ... or this much per query: a copy call per hit list costs more
constexpr size_t kCollectEntryBytes = 16;           // one re-ranked hit (szg::RerankOut)

// Entries per query of a batch of nq queries on a context whose last batches left it at radius_cap.  limited: the batch
// keeps within kRadiusBatchEntries (a shared sweep's up to 96 queries, every batch through the sketch); a query with more
// hits than its share overflows.  head_max: the most entries staged ahead of the sweep in any query's buffer (the sketch
// path's rows without a sketch): there is room for them and kRadiusCapMin more.
inline size_t collect_cap(size_t radius_cap, int nq, bool limited, size_t head_max)
{
    size_t cap = std::max(kRadiusCapMin, radius_cap);
    if (limited) cap = std::min(cap, std::max(kRadiusCapMin, kRadiusBatchEntries / (size_t)nq));
    while (cap < head_max + kRadiusCapMin) cap <<= 1;
    return cap;
}
// entries of the batch's device buffers (d_collect, d_out): query j's list starts at j * cap
inline size_t collect_block_entries(size_t cap, int nq) { return cap * (size_t)nq; }
// the whole block of re-ranked hits is copied back at enqueue time; a larger one list by list once the counts are known
inline bool collect_block_copied(size_t cap, int nq)
{
    return collect_block_entries(cap, nq) * kCollectEntryBytes <= std::max(kRadiusBlockCopyBytes, (size_t)nq * kRadiusListCopyBytes);
}
// the context's next radius_cap after a batch whose largest counter was `most`: room for that and a quarter more, in
// powers of two up to kRadiusCapMax -- and an eighth down from the last value at most
inline size_t collect_next_cap(size_t radius_cap, size_t most)
{
    size_t want = kRadiusCapMin;
    while (want < most + most / 4 && want < kRadiusCapMax) want <<= 1;
    return std::max(want, radius_cap - radius_cap / 8);
}

// Where the lists of a finished batch lie in the pinned buffer.  counts[j * stride] is query j's counter: above cap the
// query overflowed (its list is not read: cnt 0).  copied: list j at j * cap, as on the device; otherwise the lists are
// packed back to back in query order.
struct CollectLayout {
    std::vector<size_t> cnt, off;  // per query
    std::vector<uint8_t> over;     // per query: more entries than cap
    size_t most = 0;               // the largest counter, overflowed ones included
    size_t host_entries = 0;       // what the pinned buffer must hold
};
inline void collect_layout(const uint32_t *counts, size_t stride, int nq, size_t cap, bool copied, CollectLayout *out)
{
    out->cnt.assign(nq, 0);
    out->off.assign(nq, 0);
    out->over.assign(nq, 0);
    out->most = 0;
    size_t packed = 0;
    for (int j = 0; j < nq; j++) {
        const size_t n = counts[(size_t)j * stride];
        out->most = std::max(out->most, n);
        out->over[j] = n > cap;
        out->cnt[j] = n > cap ? 0 : n;
        out->off[j] = copied ? (size_t)j * cap : packed;
        packed += out->cnt[j];
    }
    out->host_entries = copied ? collect_block_entries(cap, nq) : packed;
}

}  // namespace szgi
