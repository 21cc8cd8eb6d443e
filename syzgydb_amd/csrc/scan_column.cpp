// scan_column.cpp -- resident metadata columns (include/syzgy_scan.h, szg_column) and the masks made from them.
//
// A column holds, per shard of its handle, that shard's part on the shard's device: the values (float64, or uint32
// codes whose dictionary the host owns), the present bits in the masks' layout of 16-byte pairs of words, and a host copy
// of the present words (what appends and single-row updates edit before they upload the words they touched).  Parts
// follow Shard::first; index appends only extend the last shard that holds rows or start the next one, so a part never
// moves -- it grows geometrically, in place of its old allocation.  szg_mask_where_* run one compare kernel per shard
// (kernels_column.hip) that writes the words and the count of an ordinary szg_mask.
#include "scan_internal.h"
#include "column_bits.h"

using namespace szgi;

namespace {

int stale_column() { return fail(SZG_E_INVALID, "stale column: the handle's rows were loaded or renumbered after the column was made"); }

void column_free(szg_column *c)
{
    if (!c) return;
    for (szg_column::Part &p : c->parts) {
        if (!p.values && !p.present) continue;
        (void)hipSetDevice(p.device);
        (void)hipFree(p.values);
        (void)hipFree(p.present);
    }
    delete c;
}

// room for `need` rows in part p: a new allocation of at least twice the old capacity, the old contents carried over
int part_reserve(szg_column *c, szg_column::Part &p, uint64_t need)
{
    if (need <= p.cap_rows) return SZG_OK;
    uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need, 2 * p.cap_rows), 1024);
    cap = (cap + 127) & ~127ull;
    HIPCHK(hipSetDevice(p.device));
    void *values = nullptr;
    uint64_t *present = nullptr;
    if (hipMalloc(&values, cap * c->elem()) != hipSuccess || hipMalloc((void **)&present, cap / 8) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(values);
        return fail(SZG_E_NOMEM, "out of device memory (column)");
    }
    hipError_t e = hipMemset(present, 0, cap / 8);
    if (e == hipSuccess && p.n_rows) e = hipMemcpy(values, p.values, p.n_rows * c->elem(), hipMemcpyDeviceToDevice);
    if (e == hipSuccess && p.n_rows)
        e = hipMemcpy(present, p.present_host.data(), index_words(p.n_rows) * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(values);
        (void)hipFree(present);
        return fail(SZG_E_DEVICE, "column growth", e);
    }
    p.present_host.resize((size_t)(cap / 64), 0ull);
    (void)hipFree(p.values);
    (void)hipFree(p.present);
    p.values = values;
    p.present = present;
    p.cap_rows = cap;
    return SZG_OK;
}

// the checks every call but rows / read / destroy makes first
int column_check(const szg_column *c)
{
    if (c->epoch != c->owner->col_epoch.load()) return stale_column();
    if (c->parts.size() != c->owner->shards.size()) return stale_column();
    return SZG_OK;
}

// n more rows behind the column's last: values and present bits (bit i = the i-th of these rows; null = all present)
int column_extend(szg_column *c, const void *values, const uint64_t *present_bits, uint64_t n)
{
    szg_index *ix = c->owner;
    if (c->rows + n > szg_index_rows(ix)) return fail(SZG_E_RANGE, "column append past the handle's rows");
    // which part takes how many: the shards' ranges are contiguous in row order
    std::vector<uint64_t> take(c->parts.size(), 0);
    uint64_t at = c->rows, left = n;
    for (size_t s = 0; s < c->parts.size() && left; s++) {
        const Shard *sh = ix->shards[s];
        const szg_column::Part &p = c->parts[s];
        if (sh->n_rows <= p.n_rows) continue;
        if (sh->first + p.n_rows != at) return stale_column();
        take[s] = std::min(left, sh->n_rows - p.n_rows);
        at += take[s], left -= take[s];
    }
    if (left) return stale_column();
    for (size_t s = 0; s < c->parts.size(); s++)
        if (take[s])
            if (int rc = part_reserve(c, c->parts[s], c->parts[s].n_rows + take[s])) return rc;
    uint64_t done = 0;
    for (size_t s = 0; s < c->parts.size(); s++) {
        if (!take[s]) continue;
        szg_column::Part &p = c->parts[s];
        HIPCHK(hipSetDevice(p.device));
        if (p.n_rows == 0) p.first = ix->shards[s]->first;
        HIPCHK(hipMemcpy((uint8_t *)p.values + p.n_rows * c->elem(), (const uint8_t *)values + done * c->elem(),
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

// What the szg_mask_where_* calls share: every check on the host, then one launch per shard through `launch(s, w)`,
// the count and the host copy of the words brought back once.
template <class Launch>
int mask_where(const szg_column *c, int kind, const szg_mask *base, szg_mask **out, Launch &&launch)
{
    if (!c || !out) return fail(SZG_E_INVALID, "null argument");
    szg_index *ix = c->owner;
    int rc = column_check(c);
    if (rc) return rc;
    if (kind >= 0 && c->kind != kind) return fail(SZG_E_INVALID, "the column's kind does not match the call");
    if (c->rows != szg_index_rows(ix)) return fail(SZG_E_INVALID, "short column: rows were appended to the handle but not to the column");
    for (size_t s = 0; s < c->parts.size(); s++)
        if (c->parts[s].n_rows != ix->shards[s]->n_rows || (c->parts[s].n_rows && c->parts[s].first != ix->shards[s]->first))
            return stale_column();
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
    szg_column *c = new szg_column();
    c->owner = ix;
    c->kind = kind;
    c->epoch = ix->col_epoch.load();
    c->parts.resize(ix->shards.size());
    for (size_t s = 0; s < ix->shards.size(); s++) {
        c->parts[s].device = ix->shards[s]->device;
        c->parts[s].first = ix->shards[s]->first;
    }
    const int rc = column_extend(c, values, present_bits, n_rows);
    if (rc) {
        column_free(c);
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
    if (n_rows == 0) return SZG_OK;
    return column_extend(c, values, present_bits, n_rows);
    SZG_CATCH
}

int szg_column_set(szg_column *c, uint64_t row, const void *value)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
    if (int rc = column_check(c)) return rc;
    if (row < c->owner->row_base || row - c->owner->row_base >= c->rows) return fail(SZG_E_RANGE, "row out of range");
    row -= c->owner->row_base;
    for (szg_column::Part &p : c->parts) {
        if (row < p.first || row - p.first >= p.n_rows) continue;
        const uint64_t l = row - p.first;
        HIPCHK(hipSetDevice(p.device));
        if (value) HIPCHK(hipMemcpy((uint8_t *)p.values + l * c->elem(), value, c->elem(), hipMemcpyHostToDevice));
        uint64_t w = p.present_host[l / 64];
        w = value ? (w | (1ull << (l & 63))) : (w & ~(1ull << (l & 63)));
        HIPCHK(hipMemcpy(p.present + l / 64, &w, sizeof(w), hipMemcpyHostToDevice));
        p.present_host[l / 64] = w;
        return SZG_OK;
    }
    return stale_column();
    SZG_CATCH
}

uint64_t szg_column_rows(const szg_column *c) { return c ? c->rows : 0; }

int szg_column_read(const szg_column *c, uint64_t first_row, uint64_t n_rows, void *out_values, uint64_t *out_present_bits)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
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
                             (const uint8_t *)p.values + (lo - p.first) * c->elem(), (hi - lo) * c->elem(),
                             hipMemcpyDeviceToHost));
        }
        if (out_present_bits) copy_bits(out_present_bits, lo - first_row, p.present_host.data(), lo - p.first, hi - lo);
    }
    return SZG_OK;
    SZG_CATCH
}

void szg_column_destroy(szg_column *c) { column_free(c); }

int szg_mask_where_f64(const szg_column *c, int op, double value, const szg_mask *base, szg_mask **out)
{
    SZG_TRY
    if (op < SZG_CMP_EQ || op > SZG_CMP_GE) return fail(SZG_E_INVALID, "unknown comparison operator");
    return mask_where(c, SZG_COL_F64, base, out, [&](size_t s, const szg::ColumnWhere &w) -> int {
        HIPCHK(szg::launch_column_cmp_f64(static_cast<const double *>(c->parts[s].values), op, value, w, nullptr));
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
        HIPCHK(szg::launch_column_in_f64(static_cast<const double *>(c->parts[s].values), list, (uint32_t)sorted.size(), w,
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
        HIPCHK(szg::launch_column_codes_u32(static_cast<const uint32_t *>(c->parts[s].values), bits, n_codes, w, nullptr));
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
