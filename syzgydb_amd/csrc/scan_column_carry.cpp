// scan_column_carry.cpp -- columns carried across a compaction / reorder (szg_index_reorder_carry,
// szg_index_compact_carry; scan_reorder.cpp has the rows and the masks, and makes the switch).
//
// New row i of a carried column = what old row list[i] held: the value bit for bit, the present bit, and -- a text column
// -- the row's bytes, present or not.  Like the rows, every part is built OUT OF PLACE into allocations a freshly created
// column of the new rows would have (part_reserve / heap_reserve on parts that start empty); the old parts stay untouched until
// column_carry_switch, which cannot fail, so an error anywhere leaves every column as it was.
//
// A handle of one shard: one gather launch for the values; a text column's references are gathered, their lengths
// scanned into new starts, the total read back (it sizes the new heap and is checked against the 4 GiB limit), and the
// bytes moved piece by piece into the new heap, which then holds every carried row's bytes exactly once, back to back.
//
// A handle of several: per destination part the listed rows are grouped by the source part that holds them
// (column_carry.h).  The source device packs its group -- values dense, a text group's bytes through the same scan and
// byte mover into a linear stage -- in windows of at most kCarryStageBytes (the handle's carry_stage_bytes); one hipMemcpy takes a window to the
// destination, which places the values by at[] and copies the bytes behind those of the groups before it (references
// rebased to there).  Beside the old and the new parts the call holds, per destination part at a time: the lists
// (16 bytes per row), a text group's gathered references and starts (16 bytes per row), and two stages of at most
// kCarryStageBytes on each side.
#include "scan_internal.h"
#include "column_carry.h"

namespace szgi {

namespace {

int heap_limit() { return fail(SZG_E_UNSUPPORTED, "a part's text heap stays below 4 GiB"); }

// a text group on its source device: the references of the listed rows, their new starts, the bytes they hold in all
struct TextGroup {
    DevMem<uint64_t> refs, starts, sums;
    uint64_t n = 0, total = 0;
    explicit TextGroup(int device) : refs(device), starts(device), sums(device) {}
};

int text_group_scan(const szg_column::Part &old, const uint64_t *d_list, uint64_t n, TextGroup *g)
{
    g->n = n;
    g->total = 0;
    if (n == 0) return SZG_OK;
    const uint64_t nb = szg::carry_scan_blocks(n);
    int rc = g->refs.ensure((size_t)n);
    if (rc == SZG_OK) rc = g->starts.ensure((size_t)n);
    if (rc == SZG_OK) rc = g->sums.ensure((size_t)nb + 1);
    if (rc) return rc;
    HIPCHK(szg::launch_carry_ref_starts(old.values_as<const uint64_t>(), d_list, n, g->refs.data(), g->starts.data(),
                                        g->sums.data(), nullptr));
    HIPCHK(hipMemcpy(&g->total, g->sums.data() + nb, sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SZG_OK;
}

// part `np` (the only one) of a handle of one shard from `old`, by the list on the device
int carry_part_single(const szg_column *c, const szg_column::Part &old, const uint64_t *d_list, szg_column::Part &np)
{
    const uint64_t n = np.n_rows;
    if (c->kind != SZG_COL_STR) {
        HIPCHK(szg::launch_carry_gather(old.values, (uint32_t)c->elem(), d_list, nullptr, np.values, n, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return SZG_OK;
    }
    TextGroup g(np.device);
    int rc = text_group_scan(old, d_list, n, &g);
    if (rc) return rc;
    if (!carry_heap_takes(0, g.total)) return heap_limit();
    rc = heap_reserve(np, g.total, false);   // (the mover writes every piece of the new heap, the zero ones too)
    if (rc) return rc;
    np.heap_used = g.total;
    HIPCHK(szg::launch_carry_move_bytes(old.heap, g.refs.data(), g.starts.data(), n, g.total, 0, np.heap_cap / 16, np.heap, nullptr));
    HIPCHK(szg::launch_carry_new_refs(g.refs.data(), g.starts.data(), n, 0, nullptr, np.values_as<uint64_t>(), nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));   // (before the group's buffers go)
    return SZG_OK;
}

// what a destination part's rows need on the devices, whichever column is carried: per source part its rows of the list
// (part-local, on the source's device) and where each goes (on the destination's)
struct Groups {
    std::vector<std::vector<uint64_t>> sub, at;
    std::vector<DevMem<uint64_t>> d_sub, d_at;
};

// `n` elements of `elem` bytes, dense in `from` on device dev_s, to out[at[i]] on device dev_d, through the stages
int place_window(const void *from, int dev_s, uint32_t elem, uint64_t n, const uint64_t *d_at, void *out, int dev_d,
                 DevMem<uint64_t> *stage_d)
{
    HIPCHK(hipSetDevice(dev_s));
    HIPCHK(hipStreamSynchronize(nullptr));
    int rc = stage_d->ensure((size_t)((n * elem + 7) / 8));
    if (rc) return rc;
    HIPCHK(hipMemcpy(stage_d->data(), from, n * elem, hipMemcpyDefault));
    HIPCHK(szg::launch_carry_gather(stage_d->data(), elem, nullptr, d_at, out, n, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));   // (the next window overwrites both stages)
    return SZG_OK;
}

// part d of a handle of several shards
int carry_part_grouped(const szg_column *c, const Groups &gr, uint64_t stage_bytes, szg_column::Part &np)
{
    const size_t S = c->parts.size();
    const uint32_t elem = (uint32_t)c->elem();
    const uint64_t window = carry_window_rows(stage_bytes, elem), pieces = carry_window_pieces(stage_bytes);
    DevMem<uint64_t> stage_d(np.device);
    if (c->kind != SZG_COL_STR) {
        for (size_t s = 0; s < S; s++) {
            const szg_column::Part &old = c->parts[s];
            const uint64_t cnt = gr.sub[s].size();
            DevMem<uint64_t> stage_s(old.device);
            uint64_t lo = 0, hi = 0;
            for (uint64_t w = 0; carry_window(cnt, window, w, &lo, &hi); w++) {
                int rc = stage_s.ensure((size_t)(((hi - lo) * elem + 7) / 8));
                if (rc) return rc;
                HIPCHK(szg::launch_carry_gather(old.values, elem, gr.d_sub[s].data() + lo, nullptr, stage_s.data(), hi - lo, nullptr));
                rc = place_window(stage_s.data(), old.device, elem, hi - lo, gr.d_at[s].data() + lo, np.values, np.device, &stage_d);
                if (rc) return rc;
            }
        }
        return SZG_OK;
    }
    // a text column: every group's references and starts first -- their totals size the heap
    std::vector<TextGroup> groups;
    groups.reserve(S);
    uint64_t used = 0;
    for (size_t s = 0; s < S; s++) {
        groups.emplace_back(c->parts[s].device);
        int rc = text_group_scan(c->parts[s], gr.d_sub[s].data(), gr.sub[s].size(), &groups[s]);
        if (rc) return rc;
        if (!carry_heap_takes(used, groups[s].total)) return heap_limit();
        used += groups[s].total;
    }
    int rc = heap_reserve(np, used);
    if (rc) return rc;
    np.heap_used = used;
    uint64_t base = 0;   // where the group's bytes go in the new heap
    for (size_t s = 0; s < S; s++) {
        const szg_column::Part &old = c->parts[s];
        const TextGroup &g = groups[s];
        DevMem<uint64_t> stage_s(old.device);
        uint64_t lo = 0, hi = 0;
        for (uint64_t w = 0; carry_window((g.total + 15) / 16, pieces, w, &lo, &hi); w++) {   // the bytes
            rc = stage_s.ensure((size_t)(2 * (hi - lo)));
            if (rc) return rc;
            HIPCHK(szg::launch_carry_move_bytes(old.heap, g.refs.data(), g.starts.data(), g.n, g.total, lo, hi - lo,
                                                reinterpret_cast<uint8_t *>(stage_s.data()), nullptr));
            HIPCHK(hipStreamSynchronize(nullptr));
            HIPCHK(hipSetDevice(np.device));
            HIPCHK(hipMemcpy(np.heap + base + 16 * lo, stage_s.data(), std::min(16 * hi, g.total) - 16 * lo, hipMemcpyDefault));
            HIPCHK(hipStreamSynchronize(nullptr));   // (the source's stage is free again)
        }
        for (uint64_t w = 0; carry_window(g.n, window, w, &lo, &hi); w++) {   // the references, rebased
            rc = stage_s.ensure((size_t)(hi - lo));
            if (rc) return rc;
            HIPCHK(szg::launch_carry_new_refs(g.refs.data() + lo, g.starts.data() + lo, hi - lo, base, nullptr, stage_s.data(), nullptr));
            rc = place_window(stage_s.data(), old.device, 8, hi - lo, gr.d_at[s].data() + lo, np.values, np.device, &stage_d);
            if (rc) return rc;
        }
        base += g.total;
    }
    return SZG_OK;
}

}  // namespace

int column_carry_check(szg_index *ix, szg_column *const *columns, int n_columns, std::vector<szg_column *> *out)
{
    if (n_columns < 0 || (!columns && n_columns)) return fail(SZG_E_INVALID, "null argument");
    for (int i = 0; i < n_columns; i++) {
        const szg_column *c = columns[i];
        if (!c) return fail(SZG_E_INVALID, "null column in carry");
        if (int rc = column_complete_check(ix, c)) return rc;
        if (std::find(out->begin(), out->end(), columns[i]) == out->end()) out->push_back(columns[i]);
    }
    return SZG_OK;
}

int column_carry_build(szg_index *ix, const std::vector<uint64_t> &src, const uint64_t *d_src, const std::vector<uint64_t> &counts,
                       const std::vector<uint64_t> &first, const std::vector<szg_column *> &cols, CarriedColumns *out)
{
    const size_t S = ix->shards.size();
    const uint64_t old_rows = szg_index_rows(ix);
    const uint64_t stage_bytes = ix->carry_stage_bytes ? ix->carry_stage_bytes : kCarryStageBytes;
    out->cols = cols;
    out->parts.resize(cols.size());
    for (size_t k = 0; k < cols.size(); k++)
        for (size_t d = 0; d < S; d++) {   // what a fresh column of the new rows has: part_reserve on a part that starts empty
            out->parts[k].emplace_back(ix->shards[d]->device);
            szg_column::Part &np = out->parts[k][d];
            np.first = first[d];
            if (int rc = part_reserve(cols[k], np, counts[d])) return rc;
            np.n_rows = counts[d];
        }
    std::vector<uint64_t> old_first(S), old_n(S);
    for (size_t s = 0; s < S; s++) old_first[s] = ix->shards[s]->first, old_n[s] = ix->shards[s]->n_rows;
    for (size_t d = 0; d < S && !cols.empty(); d++) {
        const uint64_t m = counts[d];
        if (m == 0) continue;
        const int dev = ix->shards[d]->device;
        const uint64_t *list = src.data() + first[d];
        DevMem<uint64_t> own_list(dev), old_all(dev);
        const uint64_t *d_list = S == 1 ? d_src : nullptr;   // (one shard: first[0] == 0, the resident list is this part's)
        int rc = SZG_OK;
        if (!d_list) {
            rc = own_list.ensure((size_t)m);
            if (rc) return rc;
            HIPCHK(hipMemcpy(own_list.data(), list, m * sizeof(uint64_t), hipMemcpyHostToDevice));
            d_list = own_list.data();
        }
        if (S > 1) rc = old_all.ensure(index_words(old_rows));
        if (rc) return rc;
        Groups gr;
        if (S > 1) {
            if (!carry_group_rows(list, m, old_first.data(), old_n.data(), S, &gr.sub, &gr.at))
                return fail(SZG_E_RANGE, "row out of range");
            for (size_t s = 0; s < S; s++) {
                gr.d_sub.emplace_back(ix->shards[s]->device);
                gr.d_at.emplace_back(dev);
            }
            for (size_t s = 0; s < S; s++) {
                const size_t cnt = gr.sub[s].size();
                if (cnt == 0) continue;
                rc = gr.d_sub[s].ensure(cnt);
                if (rc) return rc;
                HIPCHK(hipMemcpy(gr.d_sub[s].data(), gr.sub[s].data(), cnt * sizeof(uint64_t), hipMemcpyHostToDevice));
                rc = gr.d_at[s].ensure(cnt);
                if (rc) return rc;
                HIPCHK(hipMemcpy(gr.d_at[s].data(), gr.at[s].data(), cnt * sizeof(uint64_t), hipMemcpyHostToDevice));
            }
        }
        for (size_t k = 0; k < cols.size(); k++) {
            const szg_column *c = cols[k];
            szg_column::Part &np = out->parts[k][d];
            // the present bits: new bit i = old bit list[i], as the masks' (the old words of all parts side by side)
            HIPCHK(hipSetDevice(dev));
            const uint64_t *old_words = c->parts[0].present;
            if (S > 1) {
                for (const szg_column::Part &p : c->parts)
                    if (p.n_rows)
                        HIPCHK(hipMemcpy(old_all.data() + p.first / 64, p.present, index_words(p.n_rows) * sizeof(uint64_t),
                                         hipMemcpyDefault));
                old_words = old_all.data();
            }
            HIPCHK(szg::launch_mask_gather_rows(old_words, d_list, m, np.present, np.cap_rows / 128, nullptr));
            HIPCHK(hipMemcpy(np.present_host.data(), np.present, index_words(m) * sizeof(uint64_t), hipMemcpyDeviceToHost));
            rc = S == 1 ? carry_part_single(c, c->parts[0], d_list, np) : carry_part_grouped(c, gr, stage_bytes, np);
            if (rc) return rc;
        }
        HIPCHK(hipSetDevice(dev));
        HIPCHK(hipStreamSynchronize(nullptr));   // (before the lists go)
    }
    return SZG_OK;
}

void column_carry_switch(CarriedColumns *cc, uint64_t rows, uint64_t epoch)
{
    for (size_t k = 0; k < cc->cols.size(); k++) {
        szg_column *c = cc->cols[k];
        c->parts = std::move(cc->parts[k]);   // (the old allocations go, each on its own device)
        c->rows = rows;
        c->epoch = epoch;
    }
    cc->cols.clear();
    cc->parts.clear();
}

}  // namespace szgi
