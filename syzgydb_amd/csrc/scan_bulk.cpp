// scan_bulk.cpp -- bulk mutations: a list of rows overwritten, tombstoned or given new column values in ONE call
// (szg_index_overwrite_rows, its _f64 form, szg_index_tombstone_rows / _mask, szg_column_set_rows), and the two
// mutations whose vectors lie in device memory (szg_index_append_dev, szg_index_overwrite_rows_dev: launch_ingest
// reads the caller's memory in place, after dev_source_check has cleared the pointer on the host).  The same
// descriptor and checks serve the two reverse directions: szg_index_fetch_rows_dev decodes stored rows into the
// caller's device memory (launch_fetch), and szg_search_topk_dev / szg_search_radius_dev widen queries that lie there
// into one float64 batch (launch_widen_rows) and hand it to the masked searches.
//
// Every list is checked and split per shard on the host (bulk_plan.h) and every staging block is reserved before
// anything on the card changes: a bad list or a refused allocation leaves the handle as it was.  An overwrite then
// goes, per shard and per chunk of at most 64 MiB of the caller's data, through the shard's stage: the data and the
// chunk's list are uploaded, the existing encoders (launch_repack / launch_synth) fill a LINEAR block of resident rows
// behind them, one scatter launch places those rows by the list into the shard's own layout, and -- where the shard
// keeps row norms -- launch_row_norms over the linear block and a scatter of the floats refresh the listed rows'
// norms.  Everything rides the null stream; a shard is synchronised once before and once after.  Tombstones need no
// kernel: the host's live words are the master, the touched word range follows them to the card in one copy per shard.
#include "scan_internal.h"
#include "bulk_plan.h"

using namespace szgi;

namespace {

constexpr uint64_t kBulkChunkBytes = 64ull << 20;

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the checked split of a caller's list over the handle's shards (rows numbered as szg_index_overwrite numbers them)
int plan_index_rows(szg_index *ix, const uint64_t *rows, uint64_t n, int allow_duplicates, BulkPlan *plan)
{
    std::vector<uint64_t> first, count;
    for (const Shard *sh : ix->shards) first.push_back(sh->first), count.push_back(sh->n_rows);
    const char *what = "";
    const int rc = bulk_plan(first.data(), count.data(), first.size(), 0, rows, n, allow_duplicates, plan, &what);
    return rc ? fail(rc, what) : SZG_OK;
}

// The stages of the shards a call goes through, shard s's at least need[s] bytes (0: not used), each locked for the
// length of the call.  A stage that has to grow gets its new block BEFORE any old one goes, so a refusal leaves every
// stage -- and the process's block count -- as it was.
int reserve_stages(szg_index *ix, const std::vector<size_t> &need, std::vector<std::unique_lock<std::mutex>> *locks)
{
    std::vector<DevMem<uint8_t>> bigger;
    for (size_t s = 0; s < need.size(); s++) {
        bigger.emplace_back(ix->shards[s]->device);
        if (need[s]) locks->emplace_back(ix->shards[s]->stage_mu);
    }
    for (size_t s = 0; s < need.size(); s++)
        if (need[s] > ix->shards[s]->stage_cap)
            if (int rc = bigger[s].alloc_exact(std::max<size_t>(need[s], 4096), "hipMalloc(staging)")) return rc;
    for (size_t s = 0; s < need.size(); s++) {
        if (!bigger[s]) continue;
        Shard *sh = ix->shards[s];
        sh->stage_cap = bigger[s].capacity();
        sh->stage = std::move(bigger[s]);  // (the old block goes here)
    }
    return SZG_OK;
}

// entries [off, off + m) of a shard's sub-list as one block of host memory: the caller's own where they lie side by
// side in its data, else gathered into *tmp
const uint8_t *chunk_data(const uint8_t *data, size_t entry_bytes, const std::vector<uint64_t> &source, uint64_t off, uint64_t m,
                          std::vector<uint8_t> *tmp)
{
    bool dense = true;
    for (uint64_t j = 1; j < m && dense; j++) dense = source[off + j] == source[off] + j;
    if (dense) return data + source[off] * entry_bytes;
    tmp->resize((size_t)(m * entry_bytes));
    for (uint64_t j = 0; j < m; j++)
        std::memcpy(tmp->data() + j * entry_bytes, data + source[off + j] * entry_bytes, entry_bytes);
    return tmp->data();
}

// note_overwritten for every listed row, the handle's generation moved once
void note_overwritten_rows(szg_index *ix, const uint64_t *rows, uint64_t n)
{
    ix->gen++;
    for (uint64_t i = 0; i < n; i++) {
        if (!ix->sketch || ix->sk_need_full) return;
        if (ix->sk_dirty_rows.size() >= 4096) {
            ix->sk_need_full = true;
            ix->sk_dirty_rows.clear();
            return;
        }
        ix->sk_dirty_rows.push_back(rows[i]);
    }
}

// ---- vectors in device memory (szg_dev_vectors) ---------------------------------------------------------------------
constexpr size_t kSrcElemBytes[4] = {8, 4, 2, 2};  // SZG_SRC_F64, _F32, _F16, _BF16

// Every check of a device source that needs no handle state beyond dim, all of them on the host: the descriptor, the
// list of source rows, what the runtime knows about the pointer (hipPointerGetAttributes) and the extent of its
// allocation (hipMemGetAddressRange).  Nothing is launched, nothing on the card is touched.  n == 0 checks the
// descriptor only (an empty tensor has no memory to ask about).
int dev_source_check(const szg_index *ix, const szg_dev_vectors *src, const uint64_t *src_rows, uint64_t n)
{
    if (src->dtype < SZG_SRC_F64 || src->dtype > SZG_SRC_BF16) return fail(SZG_E_INVALID, "unknown source dtype");
    const size_t es = kSrcElemBytes[src->dtype];
    if (src->row_stride < (uint64_t)ix->dim) return fail(SZG_E_INVALID, "row_stride < dim");
    if (n == 0) return SZG_OK;
    if (!src->data) return fail(SZG_E_INVALID, "null argument");
    if (reinterpret_cast<uintptr_t>(src->data) % es) return fail(SZG_E_INVALID, "data not aligned to its element size");
    uint64_t last = n - 1;  // the largest source row used
    if (!src_rows) {
        if (n > src->n_rows) return fail(SZG_E_INVALID, "n_rows > src->n_rows");
    } else {
        last = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (src_rows[i] >= src->n_rows) return fail(SZG_E_RANGE, "source row out of range");
            last = std::max(last, src_rows[i]);
        }
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) count = 0;
    if (src->device < 0 || src->device >= count) return fail(SZG_E_INVALID, "device ordinal out of range");
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof attr);
    if (hipPointerGetAttributes(&attr, src->data) != hipSuccess) {  // (a pointer the runtime does not know is host memory)
        (void)hipGetLastError();
        return fail(SZG_E_INVALID, "not device memory");
    }
    if (attr.type != hipMemoryTypeDevice) return fail(SZG_E_INVALID, "not device memory");
    if (attr.device != src->device) return fail(SZG_E_INVALID, "not device memory of src->device");
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(src->data)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(SZG_E_INVALID, "not device memory");
    }
    // the last element addressed ends at data + (last * row_stride + dim) * es: inside [base, base + size)
    const unsigned __int128 end = (unsigned __int128)(reinterpret_cast<uintptr_t>(src->data) - reinterpret_cast<uintptr_t>(base)) +
                                  ((unsigned __int128)last * src->row_stride + (uint64_t)ix->dim) * es;
    if (end > size) return fail(SZG_E_RANGE, "source rows reach past the allocation");
    return SZG_OK;
}

// rows one launch_ingest may take: at most the bulk chunk's 8-byte list entries, and a grid that fits
uint64_t ingest_chunk_rows(const szg_index *ix)
{
    return std::max<uint64_t>(1, std::min<uint64_t>(kBulkChunkBytes / sizeof(uint64_t), (0x7FFFFFFFull * 256) / (ix->pitch / 16)));
}

// what an overwrite's entries are: host memory -- rows in the reference encoding, or dim float64 each -- or vectors in
// device memory, entry i from source row src_rows[i] (null: row i)
struct RowSource {
    const uint8_t *host = nullptr;
    size_t entry_bytes = 0;
    bool f64 = false;
    const szg_dev_vectors *dev = nullptr;
    const uint64_t *src_rows = nullptr;
    const char *name = "overwrite_rows";
};

// All overwrite forms: entry i replaces row rows[i].  A device source is encoded where it lies: its part of the stage
// holds the chunk's list of source rows (8 bytes per row) instead of data.
int overwrite_rows(szg_index *ix, const uint64_t *rows, const RowSource &from, uint64_t n)
{
    BulkPlan plan;
    if (int rc = plan_index_rows(ix, rows, n, 0, &plan)) return rc;
    if (n == 0) return SZG_OK;
    const size_t S = ix->shards.size();
    const szg_dev_vectors *dev = from.dev;
    if (dev)
        for (size_t s = 0; s < S; s++)
            if (!plan.local[s].empty() && ix->shards[s]->device != dev->device) return fail(SZG_E_INVALID, "source on another device");
    const size_t entry_bytes = dev ? sizeof(uint64_t) : from.entry_bytes;
    const uint64_t chunk = dev ? std::min<uint64_t>(ingest_chunk_rows(ix), std::max<uint64_t>(1, kBulkChunkBytes / ix->pitch))
                               : std::max<uint64_t>(1, kBulkChunkBytes / entry_bytes);
    // a chunk of m entries in the stage: the data (the source rows' list) | m linear resident rows | the list | m norms
    auto at_rows = [&](uint64_t m) { return up256((size_t)(m * entry_bytes)); };
    auto at_list = [&](uint64_t m) { return at_rows(m) + up256((size_t)(m * ix->pitch)); };
    auto at_norm = [&](uint64_t m) { return at_list(m) + up256((size_t)(m * sizeof(uint64_t))); };
    std::vector<size_t> need(S, 0);
    for (size_t s = 0; s < S; s++)
        if (const uint64_t c = plan.local[s].size()) need[s] = at_norm(std::min(chunk, c)) + up256((size_t)(std::min(chunk, c) * sizeof(float)));
    std::vector<std::unique_lock<std::mutex>> locks;
    if (int rc = reserve_stages(ix, need, &locks)) return rc;

    note_overwritten_rows(ix, rows, n);
    const szg::RowLayout linear{ix->pitch, 0, 0};
    std::vector<uint8_t> tmp;
    std::vector<uint64_t> from_rows;
    for (size_t s = 0; s < S; s++) {
        const uint64_t c = plan.local[s].size();
        if (c == 0) continue;
        Shard *sh = ix->shards[s];
        HIPCHK(hipSetDevice(sh->device));
        HIPCHK(hipDeviceSynchronize());  // (searches in flight on this device finish first, as for one row; a device
                                         // source lies on this device: whatever was queued to write it has finished too)
        const bool norms = sh->row_norm && sh->norm_valid;  // (the array only exists where the row width keeps norms)
        uint8_t *stage = sh->stage;
        hipError_t e = hipSuccess;
        for (uint64_t off = 0; off < c && e == hipSuccess; off += chunk) {
            const uint64_t m = std::min(chunk, c - off);
            uint8_t *d_in = stage, *d_rows = stage + at_rows(m);
            uint64_t *d_list = reinterpret_cast<uint64_t *>(stage + at_list(m));
            float *d_norm = reinterpret_cast<float *>(stage + at_norm(m));
            if (dev) {
                from_rows.resize((size_t)m);
                for (uint64_t j = 0; j < m; j++) {
                    const uint64_t i = plan.source[s][off + j];
                    from_rows[(size_t)j] = from.src_rows ? from.src_rows[i] : i;
                }
                e = hipMemcpy(d_in, from_rows.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice);
            } else {
                e = hipMemcpy(d_in, chunk_data(from.host, entry_bytes, plan.source[s], off, m, &tmp), m * entry_bytes, hipMemcpyHostToDevice);
            }
            if (e == hipSuccess) e = hipMemcpy(d_list, plan.local[s].data() + off, m * sizeof(uint64_t), hipMemcpyHostToDevice);
            if (e == hipSuccess) {
                if (dev)
                    e = szg::launch_ingest(ix->bits, d_rows, linear, 0, ix->dim, m, dev->data, dev->dtype, dev->row_stride,
                                           reinterpret_cast<const uint64_t *>(d_in), nullptr);
                else
                    e = from.f64 ? szg::launch_synth(ix->bits, d_rows, linear, 0, ix->dim, m, 0, 0, reinterpret_cast<const double *>(d_in), nullptr)
                                 : szg::launch_repack(ix->bits, d_in, ix->row_bytes, d_rows, linear, 0, m, 0, nullptr);
            }
            if (e == hipSuccess)
                e = szg::launch_scatter_rows(d_rows, linear, sh->rows, ix->layout, ix->pitch / 16, d_list, m, sh->n_rows, nullptr);
            if (e == hipSuccess && norms)  // the norms of the staged rows, then to the listed rows below norm_valid
                e = szg::launch_row_norms(ix->bits, d_rows, linear, ix->dim, (float)ix->norm_bias, 0, m, d_norm, nullptr);
            if (e == hipSuccess && norms)
                e = szg::launch_column_scatter(d_norm, sizeof(float), d_list, m, sh->row_norm.data(), sh->norm_valid, nullptr);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, from.name, e);
    }
    return SZG_OK;
}

// words [lo, hi] of a shard's live words follow the host copy to the card; `dropped` rows of it have just died
int upload_live_words(Shard *sh, uint64_t lo, uint64_t hi, uint64_t dropped)
{
    if (dropped == 0) return SZG_OK;
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipDeviceSynchronize());  // (searches in flight on this device finish first)
    HIPCHK(hipMemcpy(sh->live_bits + lo, sh->live_host.data() + lo, (hi - lo + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    sh->n_live -= dropped;
    sh->has_dead = true;
    return SZG_OK;
}

}  // namespace

extern "C" {

int szg_index_overwrite_rows(szg_index *ix, const uint64_t *rows, const uint8_t *row_bytes, uint64_t n_rows)
{
    SZG_TRY
    if (!ix || (n_rows && (!rows || !row_bytes))) return fail(SZG_E_INVALID, "null argument");
    RowSource from;
    from.host = row_bytes, from.entry_bytes = ix->row_bytes;
    return overwrite_rows(ix, rows, from, n_rows);
    SZG_CATCH
}

int szg_index_overwrite_rows_f64(szg_index *ix, const uint64_t *rows, const double *vectors, uint64_t n_rows)
{
    SZG_TRY
    if (!ix || (n_rows && (!rows || !vectors))) return fail(SZG_E_INVALID, "null argument");
    RowSource from;
    from.host = reinterpret_cast<const uint8_t *>(vectors), from.entry_bytes = (size_t)ix->dim * sizeof(double);
    from.f64 = true, from.name = "overwrite_rows_f64";
    return overwrite_rows(ix, rows, from, n_rows);
    SZG_CATCH
}

int szg_index_overwrite_rows_dev(szg_index *ix, const uint64_t *rows, const szg_dev_vectors *src, const uint64_t *src_rows,
                                 uint64_t n_rows)
{
    SZG_TRY
    if (!ix || !src || (n_rows && !rows)) return fail(SZG_E_INVALID, "null argument");
    if (int rc = dev_source_check(ix, src, src_rows, n_rows)) return rc;
    RowSource from;
    from.dev = src, from.src_rows = src_rows, from.name = "overwrite_rows_dev";
    return overwrite_rows(ix, rows, from, n_rows);
    SZG_CATCH
}

// szg_index_append_f64 for vectors in device memory: the same target shard, growth, live bits and counts; the encoder
// reads the caller's memory where it lies, and only a list of source rows (if given) goes through the stage
int szg_index_append_dev(szg_index *ix, const szg_dev_vectors *src, const uint64_t *src_rows, uint64_t n_rows)
{
    SZG_TRY
    if (!ix || !src) return fail(SZG_E_INVALID, "null argument");
    if (int rc = dev_source_check(ix, src, src_rows, n_rows)) return rc;
    Shard *sh = append_target(ix);
    if (n_rows && sh->device != src->device) return fail(SZG_E_INVALID, "source on another device");
    ix->gen++;
    ix->mask_epoch++;  // (the row count moves: masks made before are stale)
    if (n_rows == 0) return SZG_OK;
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipDeviceSynchronize());  // (the source's device: whatever was queued to write the source has finished)
    int rc = shard_reserve(ix, sh, sh->n_rows + n_rows);
    if (rc) return rc;
    const uint64_t chunk = ingest_chunk_rows(ix);
    const uint8_t *data = static_cast<const uint8_t *>(src->data);
    const size_t row_step = (size_t)src->row_stride * kSrcElemBytes[src->dtype];
    std::unique_lock<std::mutex> stage_lock(sh->stage_mu);
    uint8_t *stage8 = nullptr;
    if (src_rows)
        if ((rc = shard_stage(sh, (size_t)(std::min(chunk, n_rows) * sizeof(uint64_t)), &stage8))) return rc;
    uint64_t *d_from = reinterpret_cast<uint64_t *>(stage8);
    hipError_t e = hipSuccess;
    for (uint64_t off = 0; off < n_rows && e == hipSuccess; off += chunk) {
        const uint64_t m = std::min(chunk, n_rows - off);
        if (src_rows) e = hipMemcpy(d_from, src_rows + off, m * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = szg::launch_ingest(ix->bits, sh->rows, ix->layout, sh->n_rows + off, ix->dim, m, src_rows ? data : data + off * row_step,
                                   src->dtype, src->row_stride, d_from, nullptr);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    stage_lock.unlock();
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "append_dev", e);
    rc = shard_set_live(sh, sh->n_rows, sh->n_rows + n_rows);
    if (rc) return rc;
    sh->n_rows += n_rows;
    sh->n_live += n_rows;
    return SZG_OK;
    SZG_CATCH
}

// Stored vectors decoded into the caller's device memory: launch_fetch writes it in place, after dev_source_check (with
// n_rows destination rows) and the row checks have cleared everything on the host.  A list goes to the card once per
// chunk, through the stage of the first shard it reaches; every shard it reaches (all on the destination's device)
// then serves its own entries of that chunk.
int szg_index_fetch_rows_dev(szg_index *ix, const uint64_t *rows, uint64_t first_row, uint64_t n_rows, const szg_dev_vectors *dst)
{
    SZG_TRY
    if (!ix || !dst) return fail(SZG_E_INVALID, "null argument");
    if (int rc = dev_source_check(ix, dst, nullptr, n_rows)) return rc;
    if (n_rows == 0) return SZG_OK;  // (the descriptor only)
    const uint64_t total = szg_index_rows(ix), base = ix->row_base;
    const size_t S = ix->shards.size();
    std::vector<char> reached(S, 0);
    if (rows) {  // bulk_plan's checks, numbered with the row base; of its split only which shards are reached is used
        std::vector<uint64_t> first, count;
        for (const Shard *sh : ix->shards) first.push_back(sh->first), count.push_back(sh->n_rows);
        BulkPlan plan;
        const char *what = "";
        if (int rc = bulk_plan(first.data(), count.data(), S, base, rows, n_rows, 1, &plan, &what)) return fail(rc, what);
        for (size_t s = 0; s < S; s++) reached[s] = !plan.local[s].empty();
    } else {
        if (first_row < base || first_row - base > total || n_rows > total - (first_row - base))
            return fail(SZG_E_RANGE, "row range out of bounds");
        first_row -= base;
        for (size_t s = 0; s < S; s++) {
            const Shard *sh = ix->shards[s];
            reached[s] = std::max(first_row, sh->first) < std::min(first_row + n_rows, sh->first + sh->n_rows);
        }
    }
    Shard *lead = nullptr;  // the first shard reached: its stage carries the list
    for (size_t s = 0; s < S; s++) {
        if (!reached[s]) continue;
        if (ix->shards[s]->device != dst->device) return fail(SZG_E_INVALID, "destination on another device");
        if (!lead) lead = ix->shards[s];
    }
    HIPCHK(hipSetDevice(dst->device));
    HIPCHK(hipDeviceSynchronize());  // (whatever was queued to read or write the destination has finished)
    const uint64_t chunk = ingest_chunk_rows(ix);
    uint8_t *data = static_cast<uint8_t *>(const_cast<void *>(dst->data));
    const size_t row_step = (size_t)dst->row_stride * kSrcElemBytes[dst->dtype];
    hipError_t e = hipSuccess;
    if (!rows) {
        for (size_t s = 0; s < S && e == hipSuccess; s++) {
            const Shard *sh = ix->shards[s];
            if (!reached[s]) continue;
            const uint64_t lo = std::max(first_row, sh->first), hi = std::min(first_row + n_rows, sh->first + sh->n_rows);
            for (uint64_t off = lo; off < hi && e == hipSuccess; off += chunk)
                e = szg::launch_fetch(ix->bits, sh->rows, ix->layout, ix->dim, std::min(chunk, hi - off), nullptr, 0, sh->n_rows,
                                      off - sh->first, data + (off - first_row) * row_step, dst->dtype, dst->row_stride, nullptr);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    } else {
        std::unique_lock<std::mutex> stage_lock(lead->stage_mu);
        uint8_t *stage8 = nullptr;
        if (int rc = shard_stage(lead, (size_t)(std::min(chunk, n_rows) * sizeof(uint64_t)), &stage8)) return rc;
        HIPCHK(hipSetDevice(dst->device));
        uint64_t *d_list = reinterpret_cast<uint64_t *>(stage8);
        for (uint64_t off = 0; off < n_rows && e == hipSuccess; off += chunk) {
            const uint64_t m = std::min(chunk, n_rows - off);
            e = hipMemcpy(d_list, rows + off, m * sizeof(uint64_t), hipMemcpyHostToDevice);
            for (size_t s = 0; s < S && e == hipSuccess; s++) {
                const Shard *sh = ix->shards[s];
                if (reached[s])
                    e = szg::launch_fetch(ix->bits, sh->rows, ix->layout, ix->dim, m, d_list, base + sh->first, sh->n_rows, 0,
                                          data + off * row_step, dst->dtype, dst->row_stride, nullptr);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);  // (before the stage is anyone else's)
    }
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "fetch_rows_dev", e);
    return SZG_OK;
    SZG_CATCH
}

namespace {

// The queries of a _dev search as the dense float64 batch on the host that the masked calls take: the descriptor's
// checks, launch_widen_rows on the source's device into the handle's buffer there, one copy into the handle's pinned
// buffer.  *lock holds ix->dq_mu from here on: the buffers are the caller's until it lets go.
int dev_queries(szg_index *ix, const szg_dev_vectors *src, const uint64_t *src_rows, int n_queries, const double **out,
                std::unique_lock<std::mutex> *lock)
{
    static const double none = 0.0;
    *out = &none;  // (n_queries <= 0: nothing to convert, and the masked call says what it thinks of the count)
    if (n_queries <= 0) return dev_source_check(ix, src, src_rows, 0);
    const uint64_t n = (uint64_t)n_queries;
    if (int rc = dev_source_check(ix, src, src_rows, n)) return rc;
    *lock = std::unique_lock<std::mutex>(ix->dq_mu);
    const size_t elems = (size_t)n * (size_t)ix->dim;  // the batch, then the list of source rows
    if (ix->dq_dev.device() != src->device) ix->dq_dev = DevMem<double>(src->device);
    if (int rc = ix->dq_dev.ensure(elems + (src_rows ? (size_t)n : 0), "hipMalloc(device queries)")) return rc;
    if (int rc = ix->dq_host.ensure(elems, "hipHostMalloc(device queries)")) return rc;
    HIPCHK(hipDeviceSynchronize());  // (the source's device, current since ensure: what was queued to write the queries has finished)
    uint64_t *d_list = nullptr;
    if (src_rows) {
        d_list = reinterpret_cast<uint64_t *>(ix->dq_dev.data() + elems);
        HIPCHK(hipMemcpy(d_list, src_rows, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    HIPCHK(szg::launch_widen_rows(ix->dq_dev, ix->dim, n, src->data, src->dtype, src->row_stride, d_list, nullptr));
    HIPCHK(hipMemcpy(ix->dq_host.data(), ix->dq_dev.data(), elems * sizeof(double), hipMemcpyDeviceToHost));
    *out = ix->dq_host.data();
    return SZG_OK;
}

}  // namespace

int szg_search_topk_dev(szg_index *ix, const szg_dev_vectors *queries, const uint64_t *src_rows, int n_queries, int k,
                        const szg_mask *const *masks, int n_masks, uint64_t *out_rows, double *out_dist, int32_t *out_count)
{
    SZG_TRY
    if (!ix || !queries) return fail(SZG_E_INVALID, "null argument");
    const double *q = nullptr;
    std::unique_lock<std::mutex> lock;
    if (int rc = dev_queries(ix, queries, src_rows, n_queries, &q, &lock)) return rc;
    return szg_search_topk_masked(ix, q, n_queries, k, masks, n_masks, out_rows, out_dist, out_count);
    SZG_CATCH
}

int szg_search_radius_dev(szg_index *ix, const szg_dev_vectors *queries, const uint64_t *src_rows, int n_queries,
                          const double *radii, const szg_mask *const *masks, int n_masks, uint64_t *out_rows, double *out_dist,
                          uint64_t capacity, uint64_t *out_offsets)
{
    SZG_TRY
    if (!ix || !queries) return fail(SZG_E_INVALID, "null argument");
    const double *q = nullptr;
    std::unique_lock<std::mutex> lock;
    if (int rc = dev_queries(ix, queries, src_rows, n_queries, &q, &lock)) return rc;
    return szg_search_radius_masked(ix, q, n_queries, radii, masks, n_masks, out_rows, out_dist, capacity, out_offsets);
    SZG_CATCH
}

int szg_index_tombstone_rows(szg_index *ix, const uint64_t *rows, uint64_t n_rows, uint64_t *out_dropped)
{
    SZG_TRY
    if (!ix || (n_rows && !rows)) return fail(SZG_E_INVALID, "null argument");
    BulkPlan plan;
    if (int rc = plan_index_rows(ix, rows, n_rows, 1, &plan)) return rc;
    if (out_dropped) *out_dropped = 0;
    if (n_rows == 0) return SZG_OK;
    ix->gen++;
    ix->sk_live_dirty = true;
    uint64_t total = 0;
    int rc = SZG_OK;
    for (size_t s = 0; s < ix->shards.size() && rc == SZG_OK; s++) {
        Shard *sh = ix->shards[s];
        uint64_t dropped = 0;
        for (uint64_t l : plan.local[s]) {
            uint64_t &w = sh->live_host[l / 64];
            const uint64_t bit = 1ull << (l % 64);
            if (w & bit) w &= ~bit, dropped++;
        }
        rc = upload_live_words(sh, plan.word_lo[s], plan.word_hi[s], dropped);
        total += dropped;
    }
    if (out_dropped) *out_dropped = total;
    return rc;
    SZG_CATCH
}

int szg_index_tombstone_mask(szg_index *ix, const szg_mask *mask, uint64_t *out_dropped)
{
    SZG_TRY
    if (!ix || !mask) return fail(SZG_E_INVALID, "null argument");
    if (int rc = mask_check(ix, mask)) return rc;
    if (out_dropped) *out_dropped = 0;
    ix->gen++;  // (as the list form and the single-row form: whether or not a row dies)
    ix->sk_live_dirty = true;
    const uint64_t *words = mask_host_words(mask);  // index-level; shard starts are multiples of 64
    uint64_t total = 0;
    int rc = SZG_OK;
    for (size_t s = 0; s < ix->shards.size() && rc == SZG_OK; s++) {
        Shard *sh = ix->shards[s];
        uint64_t dropped = 0, lo = UINT64_MAX, hi = 0;
        for (size_t w = 0; w < index_words(sh->n_rows); w++) {
            const uint64_t kill = sh->live_host[w] & words[(size_t)(sh->first / 64) + w];
            if (!kill) continue;
            sh->live_host[w] &= ~kill;
            dropped += (uint64_t)__builtin_popcountll(kill);
            lo = std::min<uint64_t>(lo, w);
            hi = w;
        }
        rc = upload_live_words(sh, lo, hi, dropped);
        total += dropped;
    }
    if (out_dropped) *out_dropped = total;
    return rc;
    SZG_CATCH
}

int szg_column_set_rows(szg_column *c, const uint64_t *rows, const void *values, const uint64_t *present_bits, uint64_t n_rows)
{
    SZG_TRY
    if (!c) return fail(SZG_E_INVALID, "null argument");
    if (int rc = column_check(c)) return rc;
    if (c->kind == SZG_COL_STR) return kind_mismatch();
    if (n_rows && (!rows || !values)) return fail(SZG_E_INVALID, "null argument");
    szg_index *ix = c->owner;
    const size_t S = c->parts.size(), elem = c->elem();
    std::vector<uint64_t> first, count;
    for (const szg_column::Part &p : c->parts) first.push_back(p.first), count.push_back(p.n_rows);
    BulkPlan plan;
    const char *what = "";
    if (int rc = bulk_plan(first.data(), count.data(), S, ix->row_base, rows, n_rows, 0, &plan, &what)) return fail(rc, what);
    if (n_rows == 0) return SZG_OK;
    // per part: the present entries' rows and values side by side (an absent entry only clears its bit)
    std::vector<std::vector<uint64_t>> list(S);
    std::vector<std::vector<uint8_t>> vals(S);
    const uint64_t chunk = kBulkChunkBytes / 8;
    std::vector<size_t> need(S, 0);
    for (size_t s = 0; s < S; s++) {
        for (size_t j = 0; j < plan.local[s].size(); j++) {
            const uint64_t i = plan.source[s][j];
            if (present_bits && !((present_bits[i >> 6] >> (i & 63)) & 1ull)) continue;
            list[s].push_back(plan.local[s][j]);
            const uint8_t *v = static_cast<const uint8_t *>(values) + i * elem;
            vals[s].insert(vals[s].end(), v, v + elem);
        }
        if (const uint64_t m = std::min<uint64_t>(chunk, list[s].size())) need[s] = up256((size_t)(m * elem)) + (size_t)(m * sizeof(uint64_t));
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    if (int rc = reserve_stages(ix, need, &locks)) return rc;

    for (size_t s = 0; s < S; s++) {
        if (plan.local[s].empty()) continue;
        szg_column::Part &p = c->parts[s];
        for (size_t j = 0; j < plan.local[s].size(); j++) {
            const uint64_t i = plan.source[s][j], l = plan.local[s][j];
            const bool there = !present_bits || ((present_bits[i >> 6] >> (i & 63)) & 1ull);
            uint64_t &w = p.present_host[(size_t)(l / 64)];
            w = there ? (w | (1ull << (l & 63))) : (w & ~(1ull << (l & 63)));
        }
        HIPCHK(hipSetDevice(p.device));
        uint8_t *stage = ix->shards[s]->stage;
        const uint64_t cnt = list[s].size();
        hipError_t e = hipSuccess;
        for (uint64_t off = 0; off < cnt && e == hipSuccess; off += chunk) {
            const uint64_t m = std::min(chunk, cnt - off);
            uint64_t *d_list = reinterpret_cast<uint64_t *>(stage + up256((size_t)(m * elem)));
            e = hipMemcpy(stage, vals[s].data() + off * elem, m * elem, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = hipMemcpy(d_list, list[s].data() + off, m * sizeof(uint64_t), hipMemcpyHostToDevice);
            if (e == hipSuccess) e = szg::launch_column_scatter(stage, (uint32_t)elem, d_list, m, p.values.data(), p.n_rows, nullptr);
        }
        const uint64_t lo = plan.word_lo[s], hi = plan.word_hi[s];
        if (e == hipSuccess)
            e = hipMemcpy(p.present + lo, p.present_host.data() + lo, (hi - lo + 1) * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "column_set_rows", e);
    }
    return SZG_OK;
    SZG_CATCH
}

int szg_debug_bulk_plan(uint64_t n_rows, uint64_t row_base, const uint64_t *rows, uint64_t n, int n_shards, int allow_duplicates,
                        uint64_t *out_counts, uint64_t *out_local, uint64_t *out_source, uint64_t *out_word_lo,
                        uint64_t *out_word_hi)
{
    SZG_TRY
    if (n_shards <= 0) return fail(SZG_E_INVALID, "n_shards must be > 0");
    std::vector<uint64_t> count, first((size_t)n_shards, 0);
    split_counts((size_t)n_shards, n_rows, &count);
    for (int s = 1; s < n_shards; s++) first[s] = first[s - 1] + count[s - 1];
    BulkPlan plan;
    const char *what = "";
    const int rc = bulk_plan(first.data(), count.data(), (size_t)n_shards, row_base, rows, n, allow_duplicates, &plan, &what);
    if (rc) return fail(rc, what);
    uint64_t at = 0;
    for (int s = 0; s < n_shards; s++) {
        if (out_counts) out_counts[s] = plan.local[s].size();
        if (out_word_lo) out_word_lo[s] = plan.word_lo[s];
        if (out_word_hi) out_word_hi[s] = plan.word_hi[s];
        for (size_t j = 0; j < plan.local[s].size(); j++, at++) {
            if (out_local) out_local[at] = plan.local[s][j];
            if (out_source) out_source[at] = plan.source[s][j];
        }
    }
    return SZG_OK;
    SZG_CATCH
}

}  // extern "C"
