// scan_column.cpp -- resident metadata columns (include/syzgy_scan.h, szg_column) and the masks made from them.
//
// A column holds, per shard of its handle, that shard's part on the shard's device: the values (float64, uint32 codes
// whose dictionary the host owns, or -- a text column -- 8-byte references into a byte heap of the part's own), the
// present bits in the masks' layout of 16-byte pairs of words, and a host copy of the present words (what appends and
// single-row updates edit before they upload the words they touched).  Parts
// follow Shard::first; index appends only extend the last shard that holds rows or start the next one, so a part never
// moves -- it grows geometrically, in place of its old allocation.  szg_mask_where_* run one compare kernel per shard
// (kernels_column.hip) that writes the words and the count of an ordinary szg_mask.  A compaction / reorder that is
// asked to carry a column replaces its parts as a whole (scan_column_carry.cpp).
#include "scan_internal.h"
#include "column_bits.h"
#include "column_str.h"
#include "column_dfa.h"

using namespace szgi;

int szgi::stale_column() { return fail(SZG_E_INVALID, "stale column: the handle's rows were loaded or renumbered after the column was made"); }

// room for `need` rows in part p: a new allocation by column_grow_rows, the old contents carried over
int szgi::part_reserve(const szg_column *c, szg_column::Part &p, uint64_t need)
{
    if (need <= p.cap_rows) return SZG_OK;
    const uint64_t cap = column_grow_rows(p.cap_rows, need);
    DevMem<uint8_t> values(p.device);
    DevMem<uint64_t> present(p.device);
    if (int rc = values.alloc_exact(cap * c->elem(), "out of device memory (column)")) return rc;
    if (int rc = present.alloc_exact(cap / 64, "out of device memory (column)")) return rc;
    hipError_t e = hipMemset(present, 0, cap / 8);
    if (e == hipSuccess && p.n_rows) e = hipMemcpy(values, p.values, p.n_rows * c->elem(), hipMemcpyDeviceToDevice);
    if (e == hipSuccess && p.n_rows)
        e = hipMemcpy(present, p.present_host.data(), index_words(p.n_rows) * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "column growth", e);
    p.present_host.resize((size_t)(cap / 64), 0ull);
    p.values = std::move(values);
    p.present = std::move(present);
    p.cap_rows = cap;
    return SZG_OK;
}

// room for `used` bytes in part p's heap (str_heap_fits(used)): as part_reserve, the new bytes zero -- unless the
// caller writes every byte of the new heap itself (zeroed == false)
int szgi::heap_reserve(szg_column::Part &p, uint64_t used, bool zeroed)
{
    if (p.heap_cap && str_heap_capacity(used) <= p.heap_cap) return SZG_OK;
    const uint64_t cap = str_heap_grow(p.heap_cap, used);
    DevMem<uint8_t> heap(p.device);
    if (int rc = heap.alloc_exact(cap, "out of device memory (column heap)")) return rc;
    hipError_t e = zeroed ? hipMemset(heap, 0, cap) : hipSuccess;
    if (e == hipSuccess && p.heap_used) e = hipMemcpy(heap, p.heap, p.heap_used, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "column heap growth", e);
    p.heap = std::move(heap);
    p.heap_cap = cap;
    return SZG_OK;
}

// a complete column of this handle: made at the handle's column epoch, every part as long as its shard
int szgi::column_complete_check(const szg_index *ix, const szg_column *c)
{
    if (c->owner != ix) return fail(SZG_E_INVALID, "column belongs to another handle");
    if (c->epoch != ix->col_epoch.load() || c->parts.size() != ix->shards.size()) return stale_column();
    if (c->rows != szg_index_rows(ix))
        return fail(SZG_E_INVALID, "short column: rows were appended to the handle but not to the column");
    for (size_t s = 0; s < c->parts.size(); s++)
        if (c->parts[s].n_rows != ix->shards[s]->n_rows || (c->parts[s].n_rows && c->parts[s].first != ix->shards[s]->first))
            return stale_column();
    return SZG_OK;
}

// the checks every call but rows / read / destroy makes first
int szgi::column_check(const szg_column *c)
{
    if (c->epoch != c->owner->col_epoch.load()) return stale_column();
    if (c->parts.size() != c->owner->shards.size()) return stale_column();
    return SZG_OK;
}

int szgi::kind_mismatch() { return fail(SZG_E_INVALID, "the column's kind does not match the call"); }

namespace {

// an empty column of `kind` shaped after the handle's shards
szg_column *column_new(szg_index *ix, int kind)
{
    szg_column *c = new szg_column();
    c->owner = ix;
    c->kind = kind;
    c->epoch = ix->col_epoch.load();
    for (const Shard *sh : ix->shards) {
        c->parts.emplace_back(sh->device);
        c->parts.back().first = sh->first;
    }
    return c;
}

// how many more rows each part has room for: what its shard holds beyond it
std::vector<uint64_t> column_room(const szg_column *c)
{
    std::vector<uint64_t> room(c->parts.size(), 0);
    for (size_t s = 0; s < room.size(); s++) {
        const uint64_t have = c->owner->shards[s]->n_rows;
        if (have > c->parts[s].n_rows) room[s] = have - c->parts[s].n_rows;
    }
    return room;
}

// the parts that take rows of an append continue the column's rows: the shards' ranges are contiguous in row order
int column_take_check(const szg_column *c, const std::vector<uint64_t> &take)
{
    uint64_t at = c->rows;
    for (size_t s = 0; s < take.size(); s++) {
        if (!take[s]) continue;
        if (c->owner->shards[s]->first + c->parts[s].n_rows != at) return stale_column();
        at += take[s];
    }
    return SZG_OK;
}

// n more rows behind the column's last: values and present bits (bit i = the i-th of these rows; null = all present)
int column_extend(szg_column *c, const void *values, const uint64_t *present_bits, uint64_t n)
{
    szg_index *ix = c->owner;
    if (c->rows + n > szg_index_rows(ix)) return fail(SZG_E_RANGE, "column append past the handle's rows");
    // which part takes how many
    const std::vector<uint64_t> room = column_room(c);
    std::vector<uint64_t> take(c->parts.size(), 0);
    if (split_rows(room.data(), room.size(), n, take.data())) return stale_column();
    if (int rc = column_take_check(c, take)) return rc;
    for (size_t s = 0; s < c->parts.size(); s++)
        if (take[s])
            if (int rc = part_reserve(c, c->parts[s], c->parts[s].n_rows + take[s])) return rc;
    uint64_t done = 0;
    for (size_t s = 0; s < c->parts.size(); s++) {
        if (!take[s]) continue;
        szg_column::Part &p = c->parts[s];
        HIPCHK(hipSetDevice(p.device));
        if (p.n_rows == 0) p.first = ix->shards[s]->first;
        HIPCHK(hipMemcpy(p.values + p.n_rows * c->elem(), (const uint8_t *)values + done * c->elem(),
                         take[s] * c->elem(), hipMemcpyHostToDevice));
        copy_bits(p.present_host.data(), p.n_rows, present_bits, done, take[s]);
        const size_t w0 = (size_t)(p.n_rows / 64), w1 = index_words(p.n_rows + take[s]);
        HIPCHK(hipMemcpy(p.present + w0, p.present_host.data() + w0, (w1 - w0) * sizeof(uint64_t), hipMemcpyHostToDevice));
        p.n_rows += take[s];
        c->rows += take[s];
        done += take[s];
    }
    return SZG_OK;
}

// n more rows of a text column: row i of the call = bytes[offsets[i] .. offsets[i + 1]).  Each part that takes rows
// receives its slice of the bytes behind its heap's used bytes, and references rebased to there; an absent row gets
// length 0.  Every size is settled (str_plan_append) before anything is allocated.
int column_extend_str(szg_column *c, const uint8_t *bytes, const uint64_t *offsets, const uint64_t *present_bits, uint64_t n)
{
    szg_index *ix = c->owner;
    if (c->rows + n > szg_index_rows(ix)) return fail(SZG_E_RANGE, "column append past the handle's rows");
    if (n == 0) return SZG_OK;
    const std::vector<uint64_t> room = column_room(c);
    std::vector<uint64_t> used(c->parts.size()), take(c->parts.size(), 0), nbytes(c->parts.size(), 0);
    for (size_t s = 0; s < used.size(); s++) used[s] = c->parts[s].heap_used;
    switch (str_plan_append(offsets, n, room.data(), used.data(), room.size(), take.data(), nbytes.data())) {
    case kStrPlanOk: break;
    case kStrPlanOffsets: return fail(SZG_E_INVALID, "offsets start at 0 and never decrease");
    case kStrPlanRows: return stale_column();
    default: return fail(SZG_E_UNSUPPORTED, "a part's text heap stays below 4 GiB");
    }
    if (int rc = column_take_check(c, take)) return rc;
    for (size_t s = 0; s < c->parts.size(); s++) {
        if (!take[s]) continue;
        if (int rc = part_reserve(c, c->parts[s], c->parts[s].n_rows + take[s])) return rc;
        if (int rc = heap_reserve(c->parts[s], c->parts[s].heap_used + nbytes[s])) return rc;
    }
    uint64_t done = 0;
    std::vector<uint64_t> refs;
    for (size_t s = 0; s < c->parts.size(); s++) {
        if (!take[s]) continue;
        szg_column::Part &p = c->parts[s];
        HIPCHK(hipSetDevice(p.device));
        if (p.n_rows == 0) p.first = ix->shards[s]->first;
        refs.resize((size_t)take[s]);
        for (uint64_t i = 0; i < take[s]; i++) {
            const uint64_t r = done + i;
            const bool there = !present_bits || ((present_bits[r >> 6] >> (r & 63)) & 1ull);
            const uint64_t start = p.heap_used + (offsets[r] - offsets[done]);
            refs[(size_t)i] = start | ((there ? offsets[r + 1] - offsets[r] : 0ull) << 32);
        }
        if (nbytes[s])
            HIPCHK(hipMemcpy(p.heap + p.heap_used, bytes + offsets[done], nbytes[s], hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p.values_as<uint64_t>() + p.n_rows, refs.data(), take[s] * sizeof(uint64_t), hipMemcpyHostToDevice));
        copy_bits(p.present_host.data(), p.n_rows, present_bits, done, take[s]);
        const size_t w0 = (size_t)(p.n_rows / 64), w1 = index_words(p.n_rows + take[s]);
        HIPCHK(hipMemcpy(p.present + w0, p.present_host.data() + w0, (w1 - w0) * sizeof(uint64_t), hipMemcpyHostToDevice));
        p.heap_used += nbytes[s];
        p.n_rows += take[s];
        c->rows += take[s];
        done += take[s];
    }
    return SZG_OK;
}

// the part that holds the column's local row `row`, or null
szg_column::Part *part_of(szg_column *c, uint64_t row)
{
    for (szg_column::Part &p : c->parts)
        if (row >= p.first && row - p.first < p.n_rows) return &p;
    return nullptr;
}

// row l of part p present or absent: the host word and its copy on the device
int set_present(szg_column::Part &p, uint64_t l, bool there)
{
    uint64_t w = p.present_host[l / 64];
    w = there ? (w | (1ull << (l & 63))) : (w & ~(1ull << (l & 63)));
    HIPCHK(hipMemcpy(p.present + l / 64, &w, sizeof(w), hipMemcpyHostToDevice));
    p.present_host[l / 64] = w;
    return SZG_OK;
}

// What the szg_mask_where_* calls share: every check on the host, then one launch per shard through `launch(s, w)`,
// the count and the host copy of the words brought back once.
template <class Launch>
int mask_where(const szg_column *c, int kind, const szg_mask *base, szg_mask **out, Launch &&launch)
{
    if (!c || !out) return fail(SZG_E_INVALID, "null argument");
    szg_index *ix = c->owner;
    int rc = column_check(c);
    if (rc) return rc;
    if (kind >= 0 && c->kind != kind) return kind_mismatch();
    if ((rc = column_complete_check(ix, c))) return rc;
    if (base && (rc = mask_check(ix, base))) return rc;
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
            const szg::ColumnWhere w{c->parts[s].present, base ? mask_shard_words(base, s) : nullptr, p.words, p.pairs,
                                     p.n_rows, cnt};
            const int r2 = launch(s, w);
            if (r2) return r2;
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
}

// `n` elements of host memory on the current device for the length of one launch
template <typename T>
int upload_small(DevBuf<T> *buf, const T *src, size_t n)
{
    if (int rc = buf->ensure(std::max<size_t>(n, 1))) return rc;
    if (n) HIPCHK(hipMemcpy(buf->data(), src, n * sizeof(T), hipMemcpyHostToDevice));
    return SZG_OK;
}

}  // namespace

extern "C" {

int szg_column_create(szg_index *ix, int kind, const void *values, const uint64_t *present_bits, uint64_t n_rows,
                      szg_column **out)
{
    SZG_TRY
    if (!ix || !out || (!values && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (kind != SZG_COL_F64 && kind != SZG_COL_U32) return fail(SZG_E_INVALID, "unknown column kind");
    if (n_rows > szg_index_rows(ix)) return fail(SZG_E_RANGE, "column longer than the handle's rows");
    szg_column *c = column_new(ix, kind);
    const int rc = column_extend(c, values, present_bits, n_rows);
    if (rc) {
        delete c;
        return rc;
    }
    *out = c;
    return SZG_OK;
    SZG_CATCH
}

int szg_column_append(szg_column *c, const void *values, const uint64_t *present_bits, uint64_t n_rows)
{
    SZG_TRY
    if (!c || (!values && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (int rc = column_check(c)) return rc;
    if (c->kind == SZG_COL_STR) return kind_mismatch();
    if (n_rows == 0) return SZG_OK;
    return column_extend(c, values, present_bits, n_rows);
    SZG_CATCH
}

int szg_column_set(szg_column *c, uint64_t row, const void *value)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
    if (int rc = column_check(c)) return rc;
    if (c->kind == SZG_COL_STR) return kind_mismatch();
    if (row < c->owner->row_base || row - c->owner->row_base >= c->rows) return fail(SZG_E_RANGE, "row out of range");
    row -= c->owner->row_base;
    szg_column::Part *p = part_of(c, row);
    if (!p) return stale_column();
    const uint64_t l = row - p->first;
    HIPCHK(hipSetDevice(p->device));
    if (value) HIPCHK(hipMemcpy(p->values + l * c->elem(), value, c->elem(), hipMemcpyHostToDevice));
    return set_present(*p, l, value != nullptr);
    SZG_CATCH
}

uint64_t szg_column_rows(const szg_column *c) { return c ? c->rows : 0; }

int szg_column_get_info(const szg_column *c, szg_column_info *out)
{
    SZG_TRY
    if (!c || !out) return fail(SZG_E_INVALID, "null argument");
    szg_column_info info{};
    info.kind = c->kind;
    info.rows = c->rows;
    for (const szg_column::Part &p : c->parts) {
        info.device_bytes += p.cap_rows * c->elem() + p.cap_rows / 8 + p.heap_cap;
        info.heap_used += p.heap_used;
        info.heap_capacity += p.heap_cap;
    }
    *out = info;
    return SZG_OK;
    SZG_CATCH
}

int szg_column_read(const szg_column *c, uint64_t first_row, uint64_t n_rows, void *out_values, uint64_t *out_present_bits)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
    if (out_values && c->kind == SZG_COL_STR) return kind_mismatch();
    if (first_row < c->owner->row_base) return fail(SZG_E_RANGE, "row range out of bounds");
    first_row -= c->owner->row_base;
    if (first_row > c->rows || n_rows > c->rows - first_row) return fail(SZG_E_RANGE, "row range out of bounds");
    if (out_present_bits) std::fill(out_present_bits, out_present_bits + index_words(n_rows), 0ull);
    for (const szg_column::Part &p : c->parts) {
        const uint64_t lo = std::max(first_row, p.first), hi = std::min(first_row + n_rows, p.first + p.n_rows);
        if (lo >= hi) continue;
        if (out_values) {
            HIPCHK(hipSetDevice(p.device));
            HIPCHK(hipMemcpy((uint8_t *)out_values + (lo - first_row) * c->elem(),
                             p.values + (lo - p.first) * c->elem(), (hi - lo) * c->elem(),
                             hipMemcpyDeviceToHost));
        }
        if (out_present_bits) copy_bits(out_present_bits, lo - first_row, p.present_host.data(), lo - p.first, hi - lo);
    }
    return SZG_OK;
    SZG_CATCH
}

int szg_column_create_str(szg_index *ix, const uint8_t *bytes, const uint64_t *offsets, const uint64_t *present_bits,
                          uint64_t n_rows, szg_column **out)
{
    SZG_TRY
    if (!out || (!offsets && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (n_rows && !str_offsets_valid(offsets, n_rows)) return fail(SZG_E_INVALID, "offsets start at 0 and never decrease");
    if (!ix || (!bytes && n_rows && offsets[n_rows])) return fail(SZG_E_INVALID, "null argument");
    if (n_rows > szg_index_rows(ix)) return fail(SZG_E_RANGE, "column longer than the handle's rows");
    szg_column *c = column_new(ix, SZG_COL_STR);
    const int rc = column_extend_str(c, bytes, offsets, present_bits, n_rows);
    if (rc) {
        delete c;
        return rc;
    }
    *out = c;
    return SZG_OK;
    SZG_CATCH
}

int szg_column_append_str(szg_column *c, const uint8_t *bytes, const uint64_t *offsets, const uint64_t *present_bits,
                          uint64_t n_rows)
{
    SZG_TRY
    if (!offsets && n_rows) return fail(SZG_E_INVALID, "null argument");
    if (n_rows && !str_offsets_valid(offsets, n_rows)) return fail(SZG_E_INVALID, "offsets start at 0 and never decrease");
    if (!c || (!bytes && n_rows && offsets[n_rows])) return fail(SZG_E_INVALID, "null argument");
    if (int rc = column_check(c)) return rc;
    if (c->kind != SZG_COL_STR) return kind_mismatch();
    return column_extend_str(c, bytes, offsets, present_bits, n_rows);
    SZG_CATCH
}

int szg_column_set_str(szg_column *c, uint64_t row, const uint8_t *value, uint64_t len)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
    if (int rc = column_check(c)) return rc;
    if (c->kind != SZG_COL_STR) return kind_mismatch();
    if (row < c->owner->row_base || row - c->owner->row_base >= c->rows) return fail(SZG_E_RANGE, "row out of range");
    row -= c->owner->row_base;
    szg_column::Part *p = part_of(c, row);
    if (!p) return stale_column();
    const uint64_t l = row - p->first;
    HIPCHK(hipSetDevice(p->device));
    if (!value) return set_present(*p, l, false);
    uint64_t *slot = p->values_as<uint64_t>() + l, ref = 0;
    HIPCHK(hipMemcpy(&ref, slot, sizeof(ref), hipMemcpyDeviceToHost));
    if (len <= (ref >> 32)) {   // in place
        if (len) HIPCHK(hipMemcpy(p->heap + (uint32_t)ref, value, len, hipMemcpyHostToDevice));
        ref = (uint64_t)(uint32_t)ref | (len << 32);
        HIPCHK(hipMemcpy(slot, &ref, sizeof(ref), hipMemcpyHostToDevice));
    } else {                    // behind the heap's last byte; the old bytes are dead
        if (len > kStrHeapLimit || !str_heap_fits(p->heap_used + len))
            return fail(SZG_E_UNSUPPORTED, "a part's text heap stays below 4 GiB");
        if (int rc = heap_reserve(*p, p->heap_used + len)) return rc;
        HIPCHK(hipMemcpy(p->heap + p->heap_used, value, len, hipMemcpyHostToDevice));
        ref = p->heap_used | (len << 32);
        HIPCHK(hipMemcpy(slot, &ref, sizeof(ref), hipMemcpyHostToDevice));
        p->heap_used += len;
    }
    return set_present(*p, l, true);
    SZG_CATCH
}

int szg_column_read_str(const szg_column *c, uint64_t first_row, uint64_t n_rows, uint64_t *out_offsets, uint8_t *out_bytes,
                        uint64_t capacity, uint64_t *out_present_bits)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
    if (c->kind != SZG_COL_STR) return kind_mismatch();
    if (first_row < c->owner->row_base) return fail(SZG_E_RANGE, "row range out of bounds");
    first_row -= c->owner->row_base;
    if (first_row > c->rows || n_rows > c->rows - first_row) return fail(SZG_E_RANGE, "row range out of bounds");
    if (out_present_bits) std::fill(out_present_bits, out_present_bits + index_words(n_rows), 0ull);
    // the references of the rows, part by part, then the bytes from a copy of each part's heap
    std::vector<uint64_t> refs((size_t)n_rows);
    for (const szg_column::Part &p : c->parts) {
        const uint64_t lo = std::max(first_row, p.first), hi = std::min(first_row + n_rows, p.first + p.n_rows);
        if (lo >= hi) continue;
        HIPCHK(hipSetDevice(p.device));
        HIPCHK(hipMemcpy(refs.data() + (lo - first_row), p.values_as<const uint64_t>() + (lo - p.first),
                         (hi - lo) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out_present_bits) copy_bits(out_present_bits, lo - first_row, p.present_host.data(), lo - p.first, hi - lo);
    }
    uint64_t total = 0;
    for (uint64_t i = 0; i < n_rows; i++) {
        if (out_offsets) out_offsets[i] = total;
        total += refs[(size_t)i] >> 32;
    }
    if (out_offsets) out_offsets[n_rows] = total;
    if (!out_bytes) return SZG_OK;
    if (capacity < total) return fail(SZG_E_TRUNCATED, "the rows' bytes do not fit the buffer");
    std::vector<uint8_t> heap;
    uint64_t at = 0;
    for (const szg_column::Part &p : c->parts) {
        const uint64_t lo = std::max(first_row, p.first), hi = std::min(first_row + n_rows, p.first + p.n_rows);
        if (lo >= hi) continue;
        heap.resize((size_t)p.heap_used);
        HIPCHK(hipSetDevice(p.device));
        if (p.heap_used) HIPCHK(hipMemcpy(heap.data(), p.heap, p.heap_used, hipMemcpyDeviceToHost));
        for (uint64_t r = lo; r < hi; r++) {
            const uint64_t ref = refs[(size_t)(r - first_row)], len = ref >> 32;
            if (len) std::copy_n(heap.data() + (uint32_t)ref, len, out_bytes + at);
            at += len;
        }
    }
    return SZG_OK;
    SZG_CATCH
}

void szg_column_destroy(szg_column *c) { delete c; }  // (its parts free themselves, each on its own device)

int szg_mask_where_f64(const szg_column *c, int op, double value, const szg_mask *base, szg_mask **out)
{
    SZG_TRY
    if (op < SZG_CMP_EQ || op > SZG_CMP_GE) return fail(SZG_E_INVALID, "unknown comparison operator");
    return mask_where(c, SZG_COL_F64, base, out, [&](size_t s, const szg::ColumnWhere &w) -> int {
        HIPCHK(szg::launch_column_cmp_f64(c->parts[s].values_as<const double>(), op, value, w, nullptr));
        return SZG_OK;
    });
    SZG_CATCH
}

int szg_mask_where_in_f64(const szg_column *c, const double *values, uint32_t n_values, const szg_mask *base,
                          szg_mask **out)
{
    SZG_TRY
    if (!values && n_values) return fail(SZG_E_INVALID, "null argument");
    if (n_values > (uint32_t)szg::kColumnInMax) return fail(SZG_E_UNSUPPORTED, "an IN-list holds at most 1024 constants");
    std::vector<double> sorted;
    for (uint32_t i = 0; i < n_values; i++)
        if (values[i] == values[i]) sorted.push_back(values[i]);   // (a NaN equals no value: it never matches)
    std::sort(sorted.begin(), sorted.end());
    return mask_where(c, SZG_COL_F64, base, out, [&](size_t s, const szg::ColumnWhere &w) -> int {
        DevBuf<double> list;   // (freed after the launch: mask_where's copies wait for the kernel)
        if (int rc = upload_small(&list, sorted.data(), sorted.size())) return rc;
        HIPCHK(szg::launch_column_in_f64(c->parts[s].values_as<const double>(), list, (uint32_t)sorted.size(), w,
                                         nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return SZG_OK;
    });
    SZG_CATCH
}

int szg_mask_where_u32(const szg_column *c, const uint64_t *code_bits, uint32_t n_codes, const szg_mask *base,
                       szg_mask **out)
{
    SZG_TRY
    if (!code_bits && n_codes) return fail(SZG_E_INVALID, "null argument");
    return mask_where(c, SZG_COL_U32, base, out, [&](size_t s, const szg::ColumnWhere &w) -> int {
        DevBuf<uint64_t> bits;
        if (int rc = upload_small(&bits, code_bits, index_words(n_codes))) return rc;
        HIPCHK(szg::launch_column_codes_u32(c->parts[s].values_as<const uint32_t>(), bits, n_codes, w, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return SZG_OK;
    });
    SZG_CATCH
}

int szg_mask_where_str(const szg_column *c, int op, const uint8_t *constant, uint32_t len, const szg_mask *base,
                       szg_mask **out)
{
    SZG_TRY
    if (op < SZG_CMP_EQ || op > SZG_STR_CONTAINS) return fail(SZG_E_INVALID, "unknown comparison or string operator");
    if (len > SZG_STR_PATTERN_MAX) return fail(SZG_E_UNSUPPORTED, "a text constant holds at most 256 bytes");
    if (!constant && len) return fail(SZG_E_INVALID, "null argument");
    std::vector<uint32_t> dwords((len + 3) / 4, 0u);   // (the last one zero-padded)
    if (len) std::memcpy(dwords.data(), constant, len);
    return mask_where(c, SZG_COL_STR, base, out, [&](size_t s, const szg::ColumnWhere &w) -> int {
        DevBuf<uint32_t> k;   // (freed after the launch: mask_where's copies wait for the kernel)
        if (int rc = upload_small(&k, dwords.data(), dwords.size())) return rc;
        HIPCHK(szg::launch_column_str(c->parts[s].values_as<const uint64_t>(), c->parts[s].heap, op, k, len, w,
                                      nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return SZG_OK;
    });
    SZG_CATCH
}

int szg_mask_where_dfa(const szg_column *c, const szg_dfa *dfa, const szg_mask *base, szg_mask **out)
{
    SZG_TRY
    if (!dfa) return fail(SZG_E_INVALID, "null argument");
    switch (dfa_validate(dfa->n_states, dfa->n_classes, dfa->start, dfa->class_of, dfa->next, dfa->accept_bits)) {
    case kDfaOk: break;
    case kDfaNull: return fail(SZG_E_INVALID, "null argument");
    case kDfaCounts: return fail(SZG_E_INVALID, "dfa: 1 or more states and 1 to 256 classes");
    case kDfaTooLarge: return fail(SZG_E_UNSUPPORTED, "dfa: at most 32768 states and 2^20 table entries");
    case kDfaStart: return fail(SZG_E_INVALID, "dfa: the start state is out of range");
    case kDfaClass: return fail(SZG_E_INVALID, "dfa: a class_of entry is out of range");
    default: return fail(SZG_E_INVALID, "dfa: a next entry is out of range");
    }
    if (!c || !out) return fail(SZG_E_INVALID, "null argument");
    uint32_t start = 0;
    const std::vector<uint32_t> image = dfa_stage(dfa->n_states, dfa->n_classes, dfa->start, dfa->class_of, dfa->next, &start);
    return mask_where(c, SZG_COL_STR, base, out, [&](size_t s, const szg::ColumnWhere &w) -> int {
        DevBuf<uint32_t> table;   // (freed after the launch: mask_where's copies wait for the kernel)
        DevBuf<uint64_t> accept;
        if (int rc = upload_small(&table, image.data(), image.size())) return rc;
        if (int rc = upload_small(&accept, dfa->accept_bits, index_words(dfa->n_states))) return rc;
        HIPCHK(szg::launch_column_dfa(c->parts[s].values_as<const uint64_t>(), c->parts[s].heap, table, accept,
                                      dfa->n_states, dfa->n_classes, start, w, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
        return SZG_OK;
    });
    SZG_CATCH
}

int szg_mask_where_present(const szg_column *c, const szg_mask *base, szg_mask **out)
{
    SZG_TRY
    return mask_where(c, -1, base, out, [&](size_t, const szg::ColumnWhere &w) -> int {
        HIPCHK(szg::launch_column_present(w, nullptr));
        return SZG_OK;
    });
    SZG_CATCH
}

}  // extern "C"
