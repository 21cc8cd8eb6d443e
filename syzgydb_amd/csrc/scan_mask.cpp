// scan_mask.cpp -- device-resident filter masks (include/syzgy_scan.h, szg_mask) and the searches that take them.
//
// A mask holds, per shard of its handle, the shard-local words on the shard's device -- laid out as a batch's d_allow
// slot is (shard starts are multiples of 64, so the index-level words slice cleanly), rounded up to an even number of
// words for the kernels' 16-byte accesses, with the device popcount counter behind them -- the exact count of allowed
// rows per shard, and ONE host copy of the index-level words for the host paths that read a filter (the first-k rows,
// the exact replay, the sketch pre-pass's exception rows).  Words and counts never change after creation, so any
// number of searches may read a mask side by side.
#include "scan_internal.h"

using namespace szgi;

namespace szgi {

// an empty mask shaped after the handle's shards, its device words allocated (not yet written)
int mask_alloc(szg_index *ix, szg_mask **out)
{
    szg_mask *m = new szg_mask();
    *out = m;
    m->owner = ix;
    m->epoch = ix->mask_epoch.load();
    m->rows = szg_index_rows(ix);
    m->host.assign(index_words(m->rows), 0ull);
    for (const Shard *sh : ix->shards) m->parts.emplace_back(sh->device);
    for (size_t s = 0; s < ix->shards.size(); s++) {
        const Shard *sh = ix->shards[s];
        szg_mask::Part &p = m->parts[s];
        p.first = sh->first;
        p.n_rows = sh->n_rows;
        if (sh->n_rows == 0) continue;
        p.pairs = mask_slot_words(sh) / 2;
        HIPCHK(hipSetDevice(sh->device));
        const int rc = p.words.ensure(2 * p.pairs + 2);
        if (rc) return rc;
        m->dev_bytes += p.words.capacity() * sizeof(uint64_t);
    }
    ix->mask_live++;
    ix->mask_dev_bytes += m->dev_bytes;
    m->counted = true;
    return SZG_OK;
}

void mask_free(szg_mask *m)
{
    if (!m) return;
    if (m->counted) {
        m->owner->mask_live--;
        m->owner->mask_dev_bytes -= m->dev_bytes;
    }
    delete m;
}

}  // namespace szgi

namespace {

// Part p's words are written (tail bits possibly set): clear the tail and count on the device -- a & a through the
// combine kernel, the one popcount code -- then bring the count (and, when `download`, the words) to the host.
int mask_finish_part(szg_mask *m, size_t s, bool download)
{
    szg_mask::Part &p = m->parts[s];
    if (p.n_rows == 0) return SZG_OK;
    uint64_t *cnt = p.words + 2 * p.pairs;
    HIPCHK(hipMemsetAsync(cnt, 0, 2 * sizeof(uint64_t), nullptr));
    HIPCHK(szg::launch_mask_combine(SZG_MASK_AND, p.words, p.words, p.words, p.pairs, p.n_rows, cnt, nullptr));
    HIPCHK(hipMemcpy(&p.count, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (download)
        HIPCHK(hipMemcpy(m->host.data() + p.first / 64, p.words, index_words(p.n_rows) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    m->count += p.count;
    return SZG_OK;
}

int stale(const char *what) { return fail(SZG_E_INVALID, what); }

// the handles of a masked call, one per query: masks == NULL / n_masks == 0 leaves `out` empty (unfiltered)
int resolve_masks(szg_index *ix, const szg_mask *const *masks, int n_masks, int n_queries, std::vector<const szg_mask *> *out)
{
    out->clear();
    if (!masks || n_masks == 0) return SZG_OK;
    if (n_masks != 1 && n_masks != n_queries) return fail(SZG_E_INVALID, "n_masks must be 0, 1 or n_queries");
    bool any = false;
    for (int i = 0; i < n_masks; i++) {
        if (!masks[i]) continue;
        const int rc = mask_check(ix, masks[i]);
        if (rc) return rc;
        any = true;
    }
    if (!any) return SZG_OK;
    out->resize(n_queries);
    for (int i = 0; i < n_queries; i++) (*out)[i] = masks[n_masks == 1 ? 0 : i];
    return SZG_OK;
}

}  // namespace

namespace szgi {

int mask_check(const szg_index *ix, const szg_mask *m)
{
    if (m->owner != ix) return stale("mask belongs to another handle");
    if (m->epoch != ix->mask_epoch.load() || m->rows != szg_index_rows(ix))
        return stale("stale mask: the handle's rows were loaded or appended to after the mask was made");
    return SZG_OK;
}
const uint64_t *mask_host_words(const szg_mask *m) { return m->host.data(); }
const uint64_t *mask_shard_words(const szg_mask *m, size_t shard) { return m->parts[shard].words.data(); }
uint64_t mask_shard_count(const szg_mask *m, size_t shard) { return m->parts[shard].count; }

}  // namespace szgi

extern "C" {

int szg_mask_create(szg_index *ix, const uint64_t *allow_bits, szg_mask **out)
{
    SZG_TRY
    if (out) *out = nullptr;
    if (!ix || !allow_bits || !out) return fail(SZG_E_INVALID, "null argument");
    MaskGuard guard;
    int rc = mask_alloc(ix, &guard.m);
    szg_mask *m = guard.m;
    if (rc == SZG_OK && !m->host.empty()) {
        memcpy(m->host.data(), allow_bits, m->host.size() * sizeof(uint64_t));
        if (m->rows % 64) m->host.back() &= (1ull << (m->rows % 64)) - 1ull;
    }
    for (size_t s = 0; s < m->parts.size() && rc == SZG_OK; s++) {
        szg_mask::Part &p = m->parts[s];
        if (p.n_rows == 0) continue;
        auto body = [&]() -> int {
            HIPCHK(hipSetDevice(p.device));
            const size_t words = index_words(p.n_rows);
            HIPCHK(hipMemsetAsync(p.words + 2 * p.pairs - 2, 0, 2 * sizeof(uint64_t), nullptr));  // (the padding word)
            HIPCHK(hipMemcpy(p.words, m->host.data() + p.first / 64, words * sizeof(uint64_t), hipMemcpyHostToDevice));
            return mask_finish_part(m, s, false);
        };
        rc = body();
    }
    if (rc) return rc;
    *out = guard.release();
    return SZG_OK;
    SZG_CATCH
}

int szg_mask_create_rows(szg_index *ix, const uint64_t *rows, uint64_t n_rows, szg_mask **out)
{
    SZG_TRY
    if (out) *out = nullptr;
    if (!ix || !out || (!rows && n_rows)) return fail(SZG_E_INVALID, "null argument");
    const uint64_t total = szg_index_rows(ix);
    for (uint64_t i = 0; i < n_rows; i++)
        if (rows[i] < ix->row_base || rows[i] - ix->row_base >= total) return fail(SZG_E_RANGE, "row out of range");
    MaskGuard guard;
    int rc = mask_alloc(ix, &guard.m);
    szg_mask *m = guard.m;
    for (size_t s = 0; s < m->parts.size() && rc == SZG_OK; s++) {
        szg_mask::Part &p = m->parts[s];
        if (p.n_rows == 0) continue;
        auto body = [&]() -> int {
            HIPCHK(hipSetDevice(p.device));
            HIPCHK(hipMemsetAsync(p.words, 0, 2 * p.pairs * sizeof(uint64_t), nullptr));
            if (n_rows) {
                DevBuf<uint64_t> list;  // the whole list on every shard's device: each keeps its own rows
                const int r2 = list.ensure((size_t)n_rows);
                if (r2) return r2;
                HIPCHK(hipMemcpy(list, rows, n_rows * sizeof(uint64_t), hipMemcpyHostToDevice));
                HIPCHK(szg::launch_mask_from_rows(list, n_rows, ix->row_base + p.first, p.n_rows, p.words, nullptr));
                const int r3 = mask_finish_part(m, s, true);  // (waits for the kernel before `list` goes)
                return r3;
            }
            return mask_finish_part(m, s, false);
        };
        rc = body();
    }
    if (rc) return rc;
    *out = guard.release();
    return SZG_OK;
    SZG_CATCH
}

int szg_mask_combine(int op, const szg_mask *a, const szg_mask *b, szg_mask **out)
{
    SZG_TRY
    if (out) *out = nullptr;
    if (!a || !out) return fail(SZG_E_INVALID, "null argument");
    if (op < SZG_MASK_AND || op > SZG_MASK_NOT) return fail(SZG_E_INVALID, "unknown mask operator");
    if ((op == SZG_MASK_NOT) != (b == nullptr)) return fail(SZG_E_INVALID, "SZG_MASK_NOT takes one mask, the other operators two");
    szg_index *ix = a->owner;
    int rc = mask_check(ix, a);
    if (rc == SZG_OK && b) rc = mask_check(ix, b);
    if (rc) return rc;
    MaskGuard guard;
    rc = mask_alloc(ix, &guard.m);
    szg_mask *m = guard.m;
    for (size_t s = 0; s < m->parts.size() && rc == SZG_OK; s++) {
        szg_mask::Part &p = m->parts[s];
        if (p.n_rows == 0) continue;
        auto body = [&]() -> int {
            HIPCHK(hipSetDevice(p.device));
            uint64_t *cnt = p.words + 2 * p.pairs;
            HIPCHK(hipMemsetAsync(cnt, 0, 2 * sizeof(uint64_t), nullptr));
            HIPCHK(szg::launch_mask_combine(op, a->parts[s].words, b ? b->parts[s].words.data() : nullptr, p.words, p.pairs,
                                            p.n_rows, cnt, nullptr));
            HIPCHK(hipMemcpy(&p.count, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(m->host.data() + p.first / 64, p.words, index_words(p.n_rows) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost));
            m->count += p.count;
            return SZG_OK;
        };
        rc = body();
    }
    if (rc) return rc;
    *out = guard.release();
    return SZG_OK;
    SZG_CATCH
}

uint64_t szg_mask_count(const szg_mask *m) { return m ? m->count : 0; }

int szg_mask_read(const szg_mask *m, uint64_t *out_bits)
{
    if (!m || (!out_bits && !m->host.empty())) return fail(SZG_E_INVALID, "null argument");
    if (!m->host.empty()) memcpy(out_bits, m->host.data(), m->host.size() * sizeof(uint64_t));
    return SZG_OK;
}

void szg_mask_destroy(szg_mask *m) { mask_free(m); }

int szg_index_mask_stats(szg_index *ix, szg_mask_stats *out)
{
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    out->live_masks = ix->mask_live.load();
    out->device_bytes = ix->mask_dev_bytes.load();
    out->h2d_bytes = ix->mask_h2d.load();
    out->d2d_bytes = ix->mask_d2d.load();
    out->shared_batches = ix->mask_shared.load();
    if (ix->sketch) {  // the sweeps of the sketch pre-pass count as this index's
        out->h2d_bytes += ix->sketch->mask_h2d.load();
        out->d2d_bytes += ix->sketch->mask_d2d.load();
        out->shared_batches += ix->sketch->mask_shared.load();
    }
    return SZG_OK;
}

int szg_search_radius_masked(szg_index *ix, const double *queries, int n_queries, const double *radii,
                             const szg_mask *const *masks, int n_masks, uint64_t *out_rows, double *out_dist,
                             uint64_t capacity, uint64_t *out_offsets)
{
    SZG_TRY
    if (!ix || !queries || !radii || !out_offsets) return fail(SZG_E_INVALID, "null argument");
    if (n_queries < 0 || n_masks < 0) return fail(SZG_E_INVALID, "n_queries < 0");
    std::vector<const szg_mask *> handles;
    int rc = resolve_masks(ix, masks, n_masks, n_queries, &handles);
    if (rc) return rc;
    if (handles.empty())
        return szg_search_radius_batch(ix, queries, n_queries, radii, nullptr, out_rows, out_dist, capacity, out_offsets);
    if (capacity && (!out_rows || !out_dist)) return fail(SZG_E_INVALID, "null output buffer");
    for (int i = 0; i < n_queries; i++)
        if (!(radii[i] > 0)) return fail(SZG_E_INVALID, "radius must be > 0 (collection.go:598)");
    for (int i = 0; i <= n_queries; i++) out_offsets[i] = 0;
    if (n_queries == 0 || szg_index_rows(ix) == 0) return SZG_OK;
    std::vector<std::vector<HeapItem>> hits;
    rc = search_radius_any(ix, queries, n_queries, radii, nullptr, &hits, handles.data());
    if (rc) return rc;
    uint64_t off = 0;
    for (int i = 0; i < n_queries; i++) {
        out_offsets[i] = off;
        for (const HeapItem &h : hits[i]) {
            if (off < capacity) {
                out_rows[off] = h.row + ix->row_base;
                out_dist[off] = h.priority;
            }
            off++;
        }
    }
    out_offsets[n_queries] = off;
    if (off > capacity) return fail(SZG_E_TRUNCATED, "radius search: capacity too small");
    return SZG_OK;
    SZG_CATCH
}

}  // extern "C"

namespace szgi {

// the part of szg_search_topk_masked that does not need the combiner (scan_api.cpp): every check, and the call itself
// unless it is a lone query that may be coalesced -- then *lone is its mask and nothing has been searched yet
int search_topk_masked_prepare(szg_index *ix, const double *queries, int n_queries, int k, const szg_mask *const *masks,
                               int n_masks, uint64_t *out_rows, double *out_dist, int32_t *out_count, const szg_mask **lone)
{
    *lone = nullptr;
    if (!ix || !queries || !out_rows || !out_dist) return fail(SZG_E_INVALID, "null argument");
    if (n_queries < 0 || n_masks < 0 || k <= 0) return fail(SZG_E_INVALID, "k must be > 0 (K==0 is listing mode, collection.go:633)");
    std::vector<const szg_mask *> handles;
    const int rc = resolve_masks(ix, masks, n_masks, n_queries, &handles);
    if (rc) return rc;
    if (handles.empty() || n_queries == 0 || szg_index_rows(ix) == 0)
        return szg_search_topk(ix, queries, n_queries, k, nullptr, out_rows, out_dist, out_count);
    if (ix->coalesce && n_queries == 1 && ix->multi_query) {
        *lone = handles[0];
        return SZG_OK;
    }
    return search_topk_any(ix, queries, n_queries, k, nullptr, out_rows, out_dist, out_count, nullptr, handles.data());
}

}  // namespace szgi
