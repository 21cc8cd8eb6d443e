// scan_reorder.cpp -- compaction and reorder of the resident rows on the device (szg_index_compact,
// szg_index_reorder, and their _carry forms that take columns along).
//
// New row i = old row list[i].  The list is checked on the host (reorder_plan.h) before anything moves; the rows then
// go OUT OF PLACE into allocations sized for the new row count -- one gather launch for a handle of one shard; for a
// handle of several, per destination shard in windows of at most 64 MiB: every source shard gathers its rows of the
// window into a linear stage, the stages are copied side by side into the destination device's stage, and one launch
// of the same kernel places the window into the resident layout by a list of stage rows.  The masks the caller wants
// carried get their new words on the device as well, and the columns their new parts (scan_column_carry.cpp).  Only when
// all of that has succeeded are the old allocations freed and the shards, the live bits, the carried masks and the
// carried columns switched over: an error before that point leaves the handle, its masks and ALL its columns as they were.
// Afterwards the handle looks as after szg_index_load of the same rows in the same order.
#include "scan_internal.h"
#include "column_carry.h"

using namespace szgi;

namespace {

struct NewMask {
    szg_mask *m = nullptr;
    std::vector<szg_mask::Part> parts;
    std::vector<uint64_t> host;
    uint64_t count = 0, dev_bytes = 0;
};

// the index-level live words of the handle (shard starts are multiples of 64)
void live_words_of(const szg_index *ix, std::vector<uint64_t> *out)
{
    out->assign(index_words(szg_index_rows(ix)), 0ull);
    for (const Shard *sh : ix->shards)
        for (size_t w = 0; w < index_words(sh->n_rows); w++) (*out)[(size_t)(sh->first / 64) + w] = sh->live_host[w];
}

int check_carry(szg_index *ix, szg_mask *const *carry, int n_carry, std::vector<szg_mask *> *out)
{
    if (n_carry < 0 || (!carry && n_carry)) return fail(SZG_E_INVALID, "null argument");
    for (int i = 0; i < n_carry; i++) {
        if (!carry[i]) return fail(SZG_E_INVALID, "null mask in carry");
        const int rc = mask_check(ix, carry[i]);
        if (rc) return rc;
        if (std::find(out->begin(), out->end(), carry[i]) == out->end()) out->push_back(carry[i]);
    }
    return SZG_OK;
}

// a handle of several shards: rows [w0, w0 + m) of the new allocation `to` of shard d (m rows fit one stage) = the old
// rows src[0, m) (index-level).  Per source shard that feeds the window: its rows of the window are gathered, in the
// window's order, into a linear stage (the shard's own, or -- for the rows shard d keeps -- straight into d's) and
// copied into d's stage behind the other sources' rows; ONE launch then places the whole window, new row w0 + i from
// stage row perm[i].  The cost does not depend on how the sources interleave.
int move_window(szg_index *ix, size_t d, const ShardRows &to, uint64_t w0, const uint64_t *src, uint64_t m,
                std::vector<DevMem<uint64_t>> *d_lists, DevMem<uint64_t> *d_perm)
{
    const size_t S = ix->shards.size();
    Shard *dst = ix->shards[d];
    const uint32_t r16 = ix->pitch / 16;
    const szg::RowLayout linear{ix->pitch, 0, 0};
    // per source shard: its rows of the window (shard-local), in window order, and where in the window each goes
    std::vector<std::vector<uint64_t>> sub, at;
    std::vector<uint64_t> old_first(S), old_n(S);
    for (size_t s = 0; s < S; s++) old_first[s] = ix->shards[s]->first, old_n[s] = ix->shards[s]->n_rows;
    if (!carry_group_rows(src, m, old_first.data(), old_n.data(), S, &sub, &at)) return fail(SZG_E_RANGE, "row out of range");
    std::vector<uint64_t> perm((size_t)m);
    uint8_t *stage_d = nullptr;
    std::lock_guard<std::mutex> lk_d(dst->stage_mu);
    HIPCHK(hipSetDevice(dst->device));
    int rc = shard_stage(dst, m * ix->pitch, &stage_d);
    if (rc) return rc;
    uint64_t base = 0;  // stage row of the current source's first row
    for (size_t s = 0; s < S; s++) {
        const uint64_t c = sub[s].size();
        if (c == 0) continue;
        for (uint64_t j = 0; j < c; j++) perm[(size_t)at[s][j]] = base + j;
        Shard *from = ix->shards[s];
        HIPCHK(hipSetDevice(from->device));
        rc = (*d_lists)[s].ensure((size_t)c);
        if (rc) return rc;
        HIPCHK(hipMemcpy((*d_lists)[s].data(), sub[s].data(), c * sizeof(uint64_t), hipMemcpyHostToDevice));
        if (s == d) {
            HIPCHK(szg::launch_gather_rows(from->rows, ix->layout, stage_d, linear, r16, (*d_lists)[s].data(), c, base, nullptr));
        } else {
            std::lock_guard<std::mutex> lk_s(from->stage_mu);
            uint8_t *stage_s = nullptr;
            rc = shard_stage(from, c * ix->pitch, &stage_s);
            if (rc) return rc;
            HIPCHK(szg::launch_gather_rows(from->rows, ix->layout, stage_s, linear, r16, (*d_lists)[s].data(), c, 0, nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
            HIPCHK(hipSetDevice(dst->device));
            HIPCHK(hipMemcpy(stage_d + base * ix->pitch, stage_s, c * ix->pitch, hipMemcpyDefault));
            HIPCHK(hipStreamSynchronize(nullptr));  // (the source's stage is free again)
        }
        base += c;
    }
    HIPCHK(hipSetDevice(dst->device));
    rc = d_perm->ensure((size_t)m);
    if (rc) return rc;
    HIPCHK(hipMemcpy(d_perm->data(), perm.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(szg::launch_gather_rows(stage_d, linear, to.rows, ix->layout, r16, d_perm->data(), m, w0, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));  // (the next window overwrites the stage and the lists)
    return SZG_OK;
}

// the body of both entry points: src = the checked list (index-level old rows), counts = the new rows per shard
int reorder_checked(szg_index *ix, const std::vector<uint64_t> &src, const std::vector<uint64_t> &counts,
                    const std::vector<szg_mask *> &carry, const std::vector<szg_column *> &columns)
{
    const size_t S = ix->shards.size();
    const uint64_t n = src.size(), old_rows = szg_index_rows(ix);
    for (Shard *sh : ix->shards) {
        HIPCHK(hipSetDevice(sh->device));
        HIPCHK(hipDeviceSynchronize());
    }
    // ---- the new allocations: shard_reserve's, for rows that start empty
    std::vector<ShardRows> fresh;
    fresh.reserve(S);
    std::vector<uint64_t> first(S, 0);
    for (size_t s = 0; s < S; s++) {
        fresh.emplace_back(ix->shards[s]->device);
        first[s] = s ? first[s - 1] + counts[s - 1] : 0;
        HIPCHK(hipSetDevice(ix->shards[s]->device));
        if (int rc = rows_reserve(ix->layout, &fresh[s], counts[s])) return rc;
        if (counts[s]) HIPCHK(szg::launch_fill_bits(fresh[s].live_bits, counts[s], fresh[s].bits_cap, nullptr));
    }
    // ---- the rows
    std::vector<DevMem<uint64_t>> d_lists;  // a source shard's list on its device
    for (const Shard *sh : ix->shards) d_lists.emplace_back(sh->device);
    if (S == 1) {  // old buffer -> new buffer, one launch
        if (n) {
            HIPCHK(hipSetDevice(ix->shards[0]->device));
            int rc = d_lists[0].ensure((size_t)n);
            if (rc) return rc;
            HIPCHK(hipMemcpy(d_lists[0].data(), src.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice));
            HIPCHK(szg::launch_gather_rows(ix->shards[0]->rows, ix->layout, fresh[0].rows, ix->layout, ix->pitch / 16,
                                           d_lists[0].data(), n, 0, nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
        }
    } else {
        const uint64_t window = std::max<uint64_t>(1, (64ull << 20) / ix->pitch);
        for (size_t d = 0; d < S; d++) {
            DevMem<uint64_t> d_perm(ix->shards[d]->device);
            for (uint64_t w0 = 0; w0 < counts[d]; w0 += window) {
                int rc = move_window(ix, d, fresh[d], w0, src.data() + first[d] + w0, std::min(window, counts[d] - w0),
                                     &d_lists, &d_perm);
                if (rc) return rc;
            }
        }
    }
    // ---- the carried masks: new bit i = old bit src[i], per destination shard
    std::vector<NewMask> masks(carry.size());
    for (size_t k = 0; k < carry.size(); k++) {
        masks[k].m = carry[k];
        for (const Shard *sh : ix->shards) masks[k].parts.emplace_back(sh->device);
        masks[k].host.assign(index_words(n), 0ull);
    }
    for (size_t d = 0; d < S && !carry.empty(); d++) {
        if (counts[d] == 0) continue;
        const int dev = ix->shards[d]->device;
        HIPCHK(hipSetDevice(dev));
        DevMem<uint64_t> list(dev), old_all(dev);
        int rc = list.ensure((size_t)counts[d]);
        if (rc == SZG_OK && S > 1) rc = old_all.ensure(index_words(old_rows));
        if (rc) return rc;
        HIPCHK(hipMemcpy(list.data(), src.data() + first[d], counts[d] * sizeof(uint64_t), hipMemcpyHostToDevice));
        for (NewMask &nm : masks) {
            const uint64_t *old_words = nm.m->parts[0].words.data();
            if (S > 1) {  // the old words of every shard, side by side on this device
                for (const szg_mask::Part &p : nm.m->parts)
                    if (p.n_rows)
                        HIPCHK(hipMemcpy(old_all.data() + p.first / 64, p.words.data(), index_words(p.n_rows) * sizeof(uint64_t),
                                         hipMemcpyDefault));
                old_words = old_all.data();
            }
            szg_mask::Part &p = nm.parts[d];
            p.first = first[d];
            p.n_rows = counts[d];
            p.pairs = mask_slot_words(counts[d]) / 2;
            rc = p.words.ensure(2 * p.pairs + 2);
            if (rc) return rc;
            nm.dev_bytes += p.words.capacity() * sizeof(uint64_t);
            uint64_t *cnt = p.words.data() + 2 * p.pairs;
            HIPCHK(szg::launch_mask_gather_rows(old_words, list.data(), counts[d], p.words.data(), p.pairs, nullptr));
            HIPCHK(hipMemsetAsync(cnt, 0, 2 * sizeof(uint64_t), nullptr));
            HIPCHK(szg::launch_mask_combine(SZG_MASK_AND, p.words.data(), p.words.data(), p.words.data(), p.pairs, p.n_rows,
                                            cnt, nullptr));
            HIPCHK(hipMemcpy(&p.count, cnt, sizeof(uint64_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(nm.host.data() + p.first / 64, p.words.data(), index_words(p.n_rows) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost));
            nm.count += p.count;
        }
        HIPCHK(hipStreamSynchronize(nullptr));  // (before `list` and `old_all` go)
    }
    // ---- the carried columns: new row i reads what old row src[i] read
    CarriedColumns cols;
    if (int rc = column_carry_build(ix, src, S == 1 ? d_lists[0].data() : nullptr, counts, first, columns, &cols)) return rc;
    for (const Shard *sh : ix->shards) {
        HIPCHK(hipSetDevice(sh->device));
        HIPCHK(hipDeviceSynchronize());
    }
    // ---- the swap: nothing below fails
    for (size_t s = 0; s < S; s++) {
        Shard *sh = ix->shards[s];
        fresh[s].n_rows = counts[s];
        static_cast<ShardRows &>(*sh) = std::move(fresh[s]);  // (the old rows and live bits go)
        sh->first = first[s];
        sh->n_live = counts[s];
        sh->has_dead = false;
        sh->norm_valid = 0;
        sh->live_host.resize((size_t)sh->bits_cap);
        live_host_fill(sh, counts[s]);   // (zero behind the rows)
    }
    ix->gen++;
    const uint64_t epoch = ++ix->mask_epoch;
    column_carry_switch(&cols, n, ++ix->col_epoch);  // (every other column is stale from here on)
    if (ix->sketch) {
        // the sketch index only ever grows its shards: it goes, with what it counted kept, and the next search that
        // wants a sketch builds one sized for the new rows -- so a compaction returns the sketch's memory as well
        szg_stats all{};
        szg_mask_stats ms{};
        (void)szg_get_stats(ix, &all);
        (void)szg_index_mask_stats(ix, &ms);
        szg_index_destroy(ix->sketch);
        ix->sketch = nullptr;
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->stats = all;
        ix->mask_h2d = ms.h2d_bytes;
        ix->mask_d2d = ms.d2d_bytes;
        ix->mask_shared = ms.shared_batches;
    }
    sketch_rearm(ix);
    ix->sk_live_dirty = true;
    for (NewMask &nm : masks) {
        szg_mask *m = nm.m;
        if (m->counted) ix->mask_dev_bytes += nm.dev_bytes - m->dev_bytes;
        m->parts = std::move(nm.parts);  // (the old words go, each on its own device)
        m->host = std::move(nm.host);
        m->count = nm.count;
        m->dev_bytes = nm.dev_bytes;
        m->rows = n;
        m->epoch = epoch;
    }
    return SZG_OK;
}

}  // namespace

extern "C" {

int szg_index_reorder_carry(szg_index *ix, const uint64_t *src_rows, uint64_t n_rows, szg_mask *const *carry, int n_carry,
                            szg_column *const *columns, int n_columns)
{
    SZG_TRY
    if (!ix || (!src_rows && n_rows)) return fail(SZG_E_INVALID, "null argument");
    std::vector<szg_mask *> masks;
    std::vector<szg_column *> cols;
    int rc = check_carry(ix, carry, n_carry, &masks);
    if (rc == SZG_OK) rc = column_carry_check(ix, columns, n_columns, &cols);
    if (rc) return rc;
    std::vector<uint64_t> live, local, counts;
    live_words_of(ix, &live);
    const char *what = "";
    rc = reorder_plan(szg_index_rows(ix), live.data(), ix->row_base, src_rows, n_rows, ix->shards.size(), &local, &counts,
                      &what);
    if (rc) return fail(rc, what);
    return reorder_checked(ix, local, counts, masks, cols);
    SZG_CATCH
}

int szg_index_reorder(szg_index *ix, const uint64_t *src_rows, uint64_t n_rows, szg_mask *const *carry, int n_carry)
{
    return szg_index_reorder_carry(ix, src_rows, n_rows, carry, n_carry, nullptr, 0);
}

int szg_index_compact_carry(szg_index *ix, uint64_t *out_new_of_old, uint64_t *out_rows, szg_mask *const *carry, int n_carry,
                            szg_column *const *columns, int n_columns)
{
    SZG_TRY
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    std::vector<szg_mask *> masks;
    std::vector<szg_column *> cols;
    int rc = check_carry(ix, carry, n_carry, &masks);
    if (rc == SZG_OK) rc = column_carry_check(ix, columns, n_columns, &cols);
    if (rc) return rc;
    const uint64_t old_rows = szg_index_rows(ix);
    std::vector<uint64_t> live_list;
    live_list.reserve((size_t)szg_index_live_rows(ix));
    for (const Shard *sh : ix->shards)
        for (uint64_t r = 0; r < sh->n_rows; r++)
            if (sh->live_host[r / 64] >> (r % 64) & 1ull) live_list.push_back(sh->first + r);
    if (live_list.size() != old_rows) {  // (no tombstones: nothing moves, no mask becomes stale)
        std::vector<uint64_t> counts;
        split_rows(ix, live_list.size(), &counts);
        rc = reorder_checked(ix, live_list, counts, masks, cols);
        if (rc) return rc;
    }
    if (out_new_of_old) {
        for (uint64_t r = 0; r < old_rows; r++) out_new_of_old[r] = UINT64_MAX;
        for (size_t i = 0; i < live_list.size(); i++) out_new_of_old[live_list[i]] = ix->row_base + i;
    }
    if (out_rows) *out_rows = live_list.size();
    return SZG_OK;
    SZG_CATCH
}

int szg_index_compact(szg_index *ix, uint64_t *out_new_of_old, uint64_t *out_rows, szg_mask *const *carry, int n_carry)
{
    return szg_index_compact_carry(ix, out_new_of_old, out_rows, carry, n_carry, nullptr, 0);
}

int szg_debug_reorder_plan(uint64_t n_rows, const uint64_t *live_words, const uint64_t *src_rows, uint64_t n, int n_shards,
                           uint64_t *out_counts)
{
    SZG_TRY
    if (n_shards <= 0) return fail(SZG_E_INVALID, "n_shards must be > 0");
    std::vector<uint64_t> local, counts;
    const char *what = "";
    const int rc = reorder_plan(n_rows, live_words, 0, src_rows, n, (size_t)n_shards, &local, &counts, &what);
    if (rc) return fail(rc, what);
    if (out_counts) std::copy(counts.begin(), counts.end(), out_counts);
    return SZG_OK;
    SZG_CATCH
}

}  // extern "C"
