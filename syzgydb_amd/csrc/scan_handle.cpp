// scan_handle.cpp -- the handle: lifetime, per-shard contexts, mutations, tunables, statistics.
#include "scan_internal.h"
#include "column_carry.h"

namespace szgi {

int ctx_alloc(szg_index *ix, Shard *sh, Ctx **out)
{
    Ctx *c = new Ctx();
    *out = c;
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev_scan0));
    HIPCHK(hipEventCreate(&c->ev_scan1));
    HIPCHK(hipEventCreate(&c->ev_all0));
    HIPCHK(hipEventCreate(&c->ev_all1));
    HIPCHK(hipEventCreate(&c->ev_p0));
    HIPCHK(hipEventCreate(&c->ev_p1));
    HIPCHK(hipEventCreateWithFlags(&c->ev_scan_done, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
    const size_t B = kMaxBatch;
    // hit counters of the collect sweeps, one 128-byte line per sweep of a launch
    const size_t n_count = (size_t)kMaxBatch * szg::kCandCountStride;  // (a batch may hold kMaxBatch sweeps)
    int rc = c->h_qsw.ensure(B * ix->qsw_bytes);
    if (rc == SZG_OK) rc = c->h_q64.ensure(B * ix->dim);
    if (rc == SZG_OK) rc = c->h_count.ensure(n_count);
    if (rc == SZG_OK) rc = c->d_qsw.ensure(B * ix->qsw_bytes);
    if (rc == SZG_OK) rc = c->d_q64.ensure(B * ix->dim);
    if (rc == SZG_OK) rc = c->d_count.ensure(n_count);
    return rc;
}

void ctx_free(Ctx *c)  // (the buffers free themselves)
{
    if (!c) return;
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (hipEvent_t e : {c->ev_scan0, c->ev_scan1, c->ev_all0, c->ev_all1, c->ev_scan_done, c->ev_up, c->ev_p0, c->ev_p1})
        if (e) (void)hipEventDestroy(e);
    delete c;
}

// the one place a context is handed out (sh->mu held): the record of the batch that had it before ends here
// (limit > 0: the most recently freed context among the shard's first `limit`; null when none of them is free -- the
// caller waits for one.  Should none of them be in rotation at all -- the "contexts" option parks from the highest
// number down, so this takes an option set while a search held contexts -- the limit is void: any free context)
static Ctx *ctx_take(Shard *sh, int limit)
{
    if (limit > 0) {
        size_t eligible = 0;
        for (const Ctx *c : sh->all_ctx) eligible += c->no < limit ? 1 : 0;
        for (const Ctx *c : sh->parked_ctx) eligible -= c->no < limit ? 1 : 0;
        if (eligible == 0) limit = 0;
    }
    size_t at = sh->free_ctx.size();
    while (at > 0 && limit > 0 && sh->free_ctx[at - 1]->no >= limit) at--;
    if (at == 0) return nullptr;
    Ctx *c = sh->free_ctx[at - 1];
    sh->free_ctx.erase(sh->free_ctx.begin() + (ptrdiff_t)(at - 1));
    c->pass = Pass{};
    c->pass.work = c->stream;
    return c;
}
Ctx *ctx_acquire(Shard *sh, int limit)
{
    std::unique_lock<std::mutex> lk(sh->mu);
    Ctx *c = nullptr;
    sh->cv.wait(lk, [&] { return (c = ctx_take(sh, limit)) != nullptr; });
    return c;
}
Ctx *ctx_try_acquire(Shard *sh, int limit)
{
    std::lock_guard<std::mutex> lk(sh->mu);
    return ctx_take(sh, limit);
}
int one_sweep_contexts(const szg_index *ix)
{
    static const int queues = [] {
        const char *e = getenv("GPU_MAX_HW_QUEUES");
        const int q = e ? atoi(e) : 0;
        return q > 0 ? q : 4;
    }();
    return std::max(1, std::min(ix->n_ctx, queues - 1));
}
void ctx_release(Shard *sh, Ctx *c)
{
    {
        std::lock_guard<std::mutex> lk(sh->mu);
        sh->free_ctx.push_back(c);
    }
    sh->cv.notify_all();  // (waiters may be waiting for different contexts)
}

// the shard's staging buffer, at least `bytes` large (kept up to 64 MiB between calls); nothing in it is kept, so the
// old block goes before the new one comes
int shard_stage(Shard *sh, size_t bytes, uint8_t **out)
{
    if (sh->stage_cap < bytes) {
        sh->stage_cap = 0;
        const size_t want = std::max<size_t>(bytes, 4096);
        if (int rc = sh->stage.alloc_exact(want, "hipMalloc(staging)")) return rc;
        sh->stage_cap = want;
    }
    *out = sh->stage;
    return SZG_OK;
}

int upload_rows(szg_index *ix, Shard *sh, uint64_t dst_row, const uint8_t *rows, uint64_t n)
{
    if (n == 0) return SZG_OK;
    HIPCHK(hipSetDevice(sh->device));
    const uint64_t chunk_rows = std::max<uint64_t>(1, (64ull << 20) / ix->row_bytes);
    const uint64_t cr = std::min(chunk_rows, n);
    uint8_t *stage = nullptr;
    std::lock_guard<std::mutex> stage_lock(sh->stage_mu);
    int rc = shard_stage(sh, cr * ix->row_bytes, &stage);
    if (rc) return rc;
    // copies and the page-in kernel share the null stream: a chunk's copy waits for the previous
    // chunk's kernel, one synchronisation at the end
    hipError_t e = hipSuccess;
    for (uint64_t off = 0; off < n && e == hipSuccess; off += cr) {
        const uint64_t m = std::min(cr, n - off);
        e = hipMemcpy(stage, rows + off * ix->row_bytes, m * ix->row_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = szg::launch_repack(ix->bits, stage, ix->row_bytes, sh->rows, ix->layout, dst_row + off, m, 0,
                                   nullptr);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "upload_rows", e);
    return SZG_OK;
}

// room for `rows_needed` rows in the holder (device current): the rows' block of at least one and a half times the old
// capacity and the live words that go with it (new words zero), what the old blocks held carried over
int rows_reserve(const szg::RowLayout &layout, ShardRows *h, uint64_t rows_needed)
{
    if (rows_needed > 0xFFFFFFF0ull) return fail(SZG_E_UNSUPPORTED, "more than 2^32 rows per shard");
    if (rows_needed > h->cap_rows) {
        uint64_t cap = std::max<uint64_t>(rows_needed, h->cap_rows + h->cap_rows / 2);
        cap = (cap + 63) & ~63ull;
        DevMem<uint8_t> nr(h->rows.device());
        if (int rc = nr.alloc_exact(szg::layout_bytes(layout, cap) + 64, "hipMalloc(corpus)")) return rc;
        if (h->rows && h->n_rows) {
            const hipError_t e = hipMemcpy(nr, h->rows, szg::layout_bytes(layout, h->n_rows), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipMemcpy(corpus)", e);
        }
        h->rows = std::move(nr);
        h->cap_rows = cap;
    }
    const uint64_t words = (h->cap_rows + 63) / 64;
    if (words > h->bits_cap) {
        DevMem<uint64_t> nb(h->live_bits.device());
        if (int rc = nb.alloc_exact(words, "hipMalloc(live bits)")) return rc;
        hipError_t e = hipMemset(nb, 0, words * sizeof(uint64_t));
        if (e == hipSuccess && h->live_bits && h->bits_cap)
            e = hipMemcpy(nb, h->live_bits, h->bits_cap * sizeof(uint64_t), hipMemcpyDeviceToDevice);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipMemcpy(live bits)", e);
        h->live_bits = std::move(nb);
        h->bits_cap = words;
    }
    return SZG_OK;
}

int shard_reserve(szg_index *ix, Shard *sh, uint64_t rows_needed)
{
    HIPCHK(hipSetDevice(sh->device));
    if (int rc = rows_reserve(ix->layout, sh, rows_needed)) return rc;
    if (sh->live_host.size() < sh->bits_cap) sh->live_host.resize(sh->bits_cap, 0);
    return SZG_OK;
}

// the host's live words of a shard that holds `n_rows` rows, none of them dead: ones up to there, zero behind
void live_host_fill(Shard *sh, uint64_t n_rows)
{
    std::fill(sh->live_host.begin(), sh->live_host.end(), 0ull);
    for (uint64_t w = 0; w * 64 < n_rows; w++)
        sh->live_host[w] = n_rows - w * 64 >= 64 ? ~0ull : ((1ull << (n_rows - w * 64)) - 1ull);
}

// set live bits for rows [lo, hi) of a shard: the host copy is the master, the touched words
// follow it to the device (no read-back)
int shard_set_live(Shard *sh, uint64_t lo, uint64_t hi)
{
    if (hi <= lo) return SZG_OK;
    HIPCHK(hipSetDevice(sh->device));
    const uint64_t w0 = lo / 64, w1 = (hi - 1) / 64;
    if (sh->live_host.size() <= w1) return fail(SZG_E_RANGE, "live bitmap smaller than the shard");
    for (uint64_t r = lo; r < hi;) {
        const uint64_t w = r / 64;
        const uint64_t end = std::min(hi, (w + 1) * 64);
        const uint64_t nb = end - r;
        const uint64_t mask = (nb == 64 ? ~0ull : ((1ull << nb) - 1ull)) << (r % 64);
        sh->live_host[w] |= mask;
        r = end;
    }
    HIPCHK(hipMemcpy(sh->live_bits + w0, sh->live_host.data() + w0, (w1 - w0 + 1) * sizeof(uint64_t),
                     hipMemcpyHostToDevice));
    return SZG_OK;
}

// rows of the index are split over shards in contiguous ranges whose boundaries
// are multiples of 64 (so filter words slice cleanly): split_counts, reorder_plan.h
void split_rows(const szg_index *ix, uint64_t n_rows, std::vector<uint64_t> *counts)
{
    split_counts(ix->shards.size(), n_rows, counts);
}

Shard *shard_of(szg_index *ix, uint64_t row, uint64_t *local)
{
    for (Shard *s : ix->shards) {
        if (row >= s->first && row < s->first + s->n_rows) {
            *local = row - s->first;
            return s;
        }
    }
    return nullptr;
}

int reset_shards(szg_index *ix, const std::vector<uint64_t> &counts)
{
    uint64_t first = 0;
    for (size_t s = 0; s < ix->shards.size(); s++) {
        Shard *sh = ix->shards[s];
        HIPCHK(hipSetDevice(sh->device));
        HIPCHK(hipDeviceSynchronize());
        sh->first = first;
        sh->n_rows = 0;
        sh->norm_valid = 0;
        sh->n_live = 0;
        sh->has_dead = false;
        int rc = shard_reserve(ix, sh, counts[s]);
        if (rc) return rc;
        HIPCHK(szg::launch_fill_bits(sh->live_bits, counts[s], sh->bits_cap, nullptr));
        HIPCHK(hipDeviceSynchronize());
        live_host_fill(sh, counts[s]);
        first += counts[s];
    }
    return SZG_OK;
}

// The shard new rows go to.  Ranges stay contiguous in row order, so only the last shard
// that holds rows can grow -- or the next, still empty one can start, which it does only at
// a 64-row boundary (every shard's first row must be a multiple of 64: filter and tombstone
// bitmaps are split between shards by whole words) and once its predecessor holds 4M rows.
// a row was rewritten in place: the sketch pre-pass (if this index keeps one) re-sketches it at its next sync
void note_overwritten(szg_index *ix, uint64_t row)
{
    ix->gen++;
    if (!ix->sketch || ix->sk_need_full) return;  // no sketch yet (or a full rebuild pending): nothing to track
    if (ix->sk_dirty_rows.size() >= 4096) {       // more than a rebuild is worth
        ix->sk_need_full = true;
        ix->sk_dirty_rows.clear();
        return;
    }
    ix->sk_dirty_rows.push_back(row);
}

Shard *append_target(szg_index *ix)
{
    size_t idx = 0;
    for (size_t s = 0; s < ix->shards.size(); s++)
        if (ix->shards[s]->n_rows) idx = s;
    Shard *t = ix->shards[idx];
    if (idx + 1 < ix->shards.size() && t->n_rows >= (4ull << 20) && (t->first + t->n_rows) % 64 == 0) {
        Shard *nx = ix->shards[idx + 1];
        nx->first = t->first + t->n_rows;
        return nx;
    }
    if (t->n_rows == 0) t->first = 0;
    return t;
}

}  // namespace szgi

using namespace szgi;

extern "C" {

int szg_index_create(szg_index **out, int dim, int quant_bits, int metric, const int *devices,
                     int n_devices)
{
    SZG_TRY
    if (!out) return fail(SZG_E_INVALID, "out is null");
    *out = nullptr;
    RowFormat fmt;
    const int fmt_rc = row_format(dim, quant_bits, &fmt);
    if (fmt_rc == SZG_E_INVALID) return fmt_rc;
    if (metric != SZG_EUCLIDEAN && metric != SZG_COSINE)
        return fail(SZG_E_INVALID, "unsupported distance method (collection.go:282)");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(SZG_E_NODEVICE, "hipGetDeviceCount", e);
    if (fmt_rc) return fail(SZG_E_UNSUPPORTED, "dimension too large for the LDS-resident query");

    szg_index *ix = new szg_index();
    ix->dim = dim;
    ix->bits = quant_bits;
    ix->metric = metric;
    ix->row_bytes = fmt.row_bytes;
    ix->pitch = fmt.pitch;
    ix->layout = fmt.layout;
    ix->map = fmt.map;
    ix->qsw_bytes = fmt.qsw_bytes;
    if (quant_bits == 8 || quant_bits == 4) {
        const double M = (double)((1u << quant_bits) - 1u);
        const double slots = (double)ix->map.r16 * (128 / quant_bits);  // elements incl. padding
        ix->norm_bias = slots - (slots - dim) * M * M;  // each padding slot decodes to n = -maxInt
    }
    std::vector<int> devs;
    if (devices && n_devices > 0) {
        devs.assign(devices, devices + n_devices);
    } else {
        int cur = 0;
        (void)hipGetDevice(&cur);
        devs.push_back(cur);
    }
    for (int d : devs) {
        if (d < 0 || d >= count) {
            szg_index_destroy(ix);
            return fail(SZG_E_INVALID, "device ordinal out of range");
        }
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, d);
        if (e != hipSuccess) {
            szg_index_destroy(ix);
            return fail(SZG_E_NODEVICE, "hipGetDeviceProperties", e);
        }
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            szg_index_destroy(ix);
            return fail(SZG_E_NODEVICE, "device is not gfx950 (kernels are built for MI355X only)");
        }
        Shard *sh = new Shard(d);
        sh->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        ix->shards.push_back(sh);
    }
    for (Shard *sh : ix->shards) {
        if (hipSetDevice(sh->device) != hipSuccess ||
            hipStreamCreateWithFlags(&sh->scan_stream, hipStreamNonBlocking) != hipSuccess) {
            szg_index_destroy(ix);
            return fail(SZG_E_DEVICE, "hipStreamCreate(scan stream)");
        }
        int rc = sh->zero16.alloc_exact(64, "hipMalloc(zero16)");
        if (rc == SZG_OK && hipMemset(sh->zero16, 0, 64) != hipSuccess) rc = fail(SZG_E_NOMEM, "hipMemset(zero16)");
        if (rc) {
            szg_index_destroy(ix);
            return rc;
        }
        for (int i = 0; i < ix->n_ctx; i++) {
            Ctx *c = nullptr;
            rc = ctx_alloc(ix, sh, &c);
            if (rc) {
                ctx_free(c);
                szg_index_destroy(ix);
                return rc;
            }
            c->no = i;
            sh->all_ctx.push_back(c);
            (i < ix->n_ctx_active ? sh->free_ctx : sh->parked_ctx).push_back(c);
        }
    }
    *out = ix;
    return SZG_OK;
    SZG_CATCH
}

void szg_index_destroy(szg_index *ix)
{
    if (!ix) return;
    if (ix->sketch) {
        szg_index_destroy(ix->sketch);
        ix->sketch = nullptr;
    }
    if (g_sites.on) {
        for (int i = 0; i < SiteTimers::N; i++)
            if (g_sites.n[i])
                fprintf(stderr, "[szg sites] %-14s %10.1f us / %8llu calls = %7.2f us\n", g_sites.name[i], g_sites.us[i],
                        (unsigned long long)g_sites.n[i], g_sites.us[i] / (double)g_sites.n[i]);
        g_sites = SiteTimers{};
    }
    for (Shard *sh : ix->shards) {
        (void)hipSetDevice(sh->device);
        (void)hipDeviceSynchronize();
        for (Ctx *c : sh->all_ctx) ctx_free(c);
        if (sh->scan_stream) (void)hipStreamDestroy(sh->scan_stream);
        delete sh;  // (its device memory goes with it)
    }
    delete ix;
}

uint64_t szg_index_rows(const szg_index *ix)
{
    uint64_t n = 0;
    if (ix) for (const Shard *s : ix->shards) n += s->n_rows;
    return n;
}

uint64_t szg_index_live_rows(const szg_index *ix)
{
    uint64_t n = 0;
    if (ix) for (const Shard *s : ix->shards) n += s->n_live;
    return n;
}

int szg_index_load(szg_index *ix, const uint8_t *rows, uint64_t n_rows)
{
    SZG_TRY
    if (ix) { ix->gen++; ix->mask_epoch++; ix->col_epoch++; sketch_rearm(ix); }  // (masks and columns made before are stale from here on)
    if (!ix || (!rows && n_rows)) return fail(SZG_E_INVALID, "null argument");
    std::vector<uint64_t> counts;
    split_rows(ix, n_rows, &counts);
    int rc = reset_shards(ix, counts);
    if (rc) return rc;
    for (size_t s = 0; s < ix->shards.size(); s++) {
        Shard *sh = ix->shards[s];
        rc = upload_rows(ix, sh, 0, rows + sh->first * ix->row_bytes, counts[s]);
        if (rc) return rc;
        sh->n_rows = counts[s];
        sh->n_live = counts[s];
    }
    return SZG_OK;
    SZG_CATCH
}

int szg_index_synth(szg_index *ix, uint64_t n_rows, uint64_t seed, uint64_t first_row)
{
    SZG_TRY
    if (ix) { ix->gen++; ix->mask_epoch++; ix->col_epoch++; sketch_rearm(ix); }  // (masks and columns made before are stale from here on)
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    std::vector<uint64_t> counts;
    split_rows(ix, n_rows, &counts);
    int rc = reset_shards(ix, counts);
    if (rc) return rc;
    for (size_t s = 0; s < ix->shards.size(); s++) {
        Shard *sh = ix->shards[s];
        HIPCHK(hipSetDevice(sh->device));
        HIPCHK(szg::launch_synth(ix->bits, sh->rows, ix->layout, 0, ix->dim, counts[s], seed,
                                 first_row + sh->first, nullptr, nullptr));
        HIPCHK(hipDeviceSynchronize());
        sh->n_rows = counts[s];
        sh->n_live = counts[s];
    }
    return SZG_OK;
    SZG_CATCH
}

int szg_index_append(szg_index *ix, const uint8_t *rows, uint64_t n_rows)
{
    SZG_TRY
    if (ix) { ix->gen++; ix->mask_epoch++; }  // (the row count moves: masks made before are stale)
    if (!ix || (!rows && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (n_rows == 0) return SZG_OK;
    Shard *sh = append_target(ix);
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipDeviceSynchronize());
    int rc = shard_reserve(ix, sh, sh->n_rows + n_rows);
    if (rc) return rc;
    rc = upload_rows(ix, sh, sh->n_rows, rows, n_rows);
    if (rc) return rc;
    rc = shard_set_live(sh, sh->n_rows, sh->n_rows + n_rows);
    if (rc) return rc;
    sh->n_rows += n_rows;
    sh->n_live += n_rows;
    return SZG_OK;
    SZG_CATCH
}

// AddDocument for a block of float64 vectors: quantize + pack on the device
int szg_index_append_f64(szg_index *ix, const double *vectors, uint64_t n_rows)
{
    SZG_TRY
    if (ix) { ix->gen++; ix->mask_epoch++; }  // (the row count moves: masks made before are stale)
    if (!ix || (!vectors && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (n_rows == 0) return SZG_OK;
    Shard *sh = append_target(ix);
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipDeviceSynchronize());
    int rc = shard_reserve(ix, sh, sh->n_rows + n_rows);
    if (rc) return rc;
    const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)ix->dim * 8));
    uint8_t *stage8 = nullptr;
    std::unique_lock<std::mutex> stage_lock(sh->stage_mu);
    rc = shard_stage(sh, std::min(chunk, n_rows) * (uint64_t)ix->dim * 8, &stage8);
    if (rc) return rc;
    double *stage = reinterpret_cast<double *>(stage8);
    hipError_t e = hipSuccess;
    for (uint64_t off = 0; off < n_rows && e == hipSuccess; off += chunk) {
        const uint64_t m = std::min(chunk, n_rows - off);
        e = hipMemcpy(stage, vectors + off * (uint64_t)ix->dim, m * (uint64_t)ix->dim * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = szg::launch_synth(ix->bits, sh->rows, ix->layout, sh->n_rows + off, ix->dim, m, 0, 0, stage,
                                  nullptr);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    stage_lock.unlock();
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "append_f64", e);
    rc = shard_set_live(sh, sh->n_rows, sh->n_rows + n_rows);
    if (rc) return rc;
    sh->n_rows += n_rows;
    sh->n_live += n_rows;
    return SZG_OK;
    SZG_CATCH
}

// AddDocument on an existing id from a float64 vector: re-encode one row in place
int szg_index_overwrite_f64(szg_index *ix, uint64_t row, const double *vector)
{
    SZG_TRY
    if (!ix || !vector) return fail(SZG_E_INVALID, "null argument");
    uint64_t local;
    Shard *sh = shard_of(ix, row, &local);
    if (!sh) return fail(SZG_E_RANGE, "row out of range");
    note_overwritten(ix, row);
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipDeviceSynchronize());
    uint8_t *stage8 = nullptr;
    std::lock_guard<std::mutex> stage_lock(sh->stage_mu);
    int rc = shard_stage(sh, (size_t)ix->dim * 8, &stage8);
    if (rc) return rc;
    double *stage = reinterpret_cast<double *>(stage8);
    hipError_t e = hipMemcpy(stage, vector, (size_t)ix->dim * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = szg::launch_synth(ix->bits, sh->rows, ix->layout, local, ix->dim, 1, 0, 0, stage, nullptr);
    if (e == hipSuccess && sh->row_norm && local < sh->norm_valid)
        e = szg::launch_row_norms(ix->bits, sh->rows, ix->layout, ix->dim, (float)ix->norm_bias, local, 1, sh->row_norm, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(SZG_E_DEVICE, "overwrite_f64", e);
    return SZG_OK;
    SZG_CATCH
}

int szg_index_overwrite(szg_index *ix, uint64_t row, const uint8_t *row_bytes)
{
    SZG_TRY
    if (!ix || !row_bytes) return fail(SZG_E_INVALID, "null argument");
    uint64_t local;
    Shard *sh = shard_of(ix, row, &local);
    if (!sh) return fail(SZG_E_RANGE, "row out of range");
    note_overwritten(ix, row);
    HIPCHK(hipSetDevice(sh->device));
    HIPCHK(hipDeviceSynchronize());
    const int rc = upload_rows(ix, sh, local, row_bytes, 1);
    if (rc == SZG_OK && sh->row_norm && local < sh->norm_valid) {
        HIPCHK(szg::launch_row_norms(ix->bits, sh->rows, ix->layout, ix->dim, (float)ix->norm_bias, local, 1, sh->row_norm, nullptr));
        HIPCHK(hipStreamSynchronize(nullptr));
    }
    return rc;
    SZG_CATCH
}

int szg_index_tombstone(szg_index *ix, uint64_t row)
{
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    ix->gen++;
    ix->sk_live_dirty = true;
    uint64_t local;
    Shard *sh = shard_of(ix, row, &local);
    if (!sh) return fail(SZG_E_RANGE, "row out of range");
    HIPCHK(hipSetDevice(sh->device));
    const uint64_t bit = 1ull << (local % 64);
    uint64_t &w = sh->live_host[local / 64];
    if (w & bit) {
        // searches in flight on this device finish first (callers hold the write lock; this
        // also covers a search that failed half-way)
        HIPCHK(hipDeviceSynchronize());
        w &= ~bit;
        HIPCHK(hipMemcpy(sh->live_bits + local / 64, &w, sizeof(w), hipMemcpyHostToDevice));
        sh->n_live--;
        sh->has_dead = true;
    }
    return SZG_OK;
}

int szg_index_read_rows(szg_index *ix, uint64_t first_row, uint64_t n_rows, uint8_t *out)
{
    SZG_TRY
    if (!ix || (!out && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (first_row + n_rows > szg_index_rows(ix)) return fail(SZG_E_RANGE, "row range out of bounds");
    for (Shard *sh : ix->shards) {
        const uint64_t lo = std::max(first_row, sh->first);
        const uint64_t hi = std::min(first_row + n_rows, sh->first + sh->n_rows);
        if (hi <= lo) continue;
        HIPCHK(hipSetDevice(sh->device));
        const uint64_t m = hi - lo;
        const uint64_t cr = std::min<uint64_t>(m, std::max<uint64_t>(1, (64ull << 20) / ix->row_bytes));
        uint8_t *stage = nullptr;
        std::lock_guard<std::mutex> stage_lock(sh->stage_mu);
        int rc = shard_stage(sh, cr * ix->row_bytes, &stage);
        if (rc) return rc;
        hipError_t e = hipSuccess;
        for (uint64_t off = 0; off < m && e == hipSuccess; off += cr) {
            const uint64_t mm = std::min(cr, m - off);
            e = szg::launch_repack(ix->bits, stage, ix->row_bytes, sh->rows, ix->layout, lo - sh->first + off, mm, 1,
                                   nullptr);
            if (e == hipSuccess)
                e = hipMemcpy(out + (lo - first_row + off) * ix->row_bytes, stage, mm * ix->row_bytes,
                              hipMemcpyDeviceToHost);
        }
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "read_rows", e);
    }
    return SZG_OK;
    SZG_CATCH
}

int szg_index_set_row_base(szg_index *ix, uint64_t base)
{
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    ix->row_base = base;
    return SZG_OK;
}

int szg_set_timing(szg_index *ix, int enabled)
{
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    for (Shard *sh : ix->shards) {
        (void)hipSetDevice(sh->device);
        (void)hipDeviceSynchronize();
    }
    ix->timing = enabled < 0 ? 0 : (enabled > 2 ? 2 : enabled);
    if (ix->sketch) ix->sketch->timing = ix->timing;
    return SZG_OK;
}

int szg_get_stats(szg_index *ix, szg_stats *out)
{
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    *out = ix->stats;
    if (ix->sketch) {  // the sweeps of the sketch pre-pass count as this index's
        std::lock_guard<std::mutex> lk2(ix->sketch->stats_mu);
        const szg_stats &k = ix->sketch->stats;
        out->scan_launches += k.scan_launches;
        out->escalations += k.escalations;
        out->scan_bytes += k.scan_bytes;
        out->scan_ms += k.scan_ms;
        out->total_ms += k.total_ms;
        out->timed_launches += k.timed_launches;
        out->full_replays += k.full_replays;
        out->mq_launches += k.mq_launches;
        out->mq_queries += k.mq_queries;
        out->mq_fallbacks += k.mq_fallbacks;
        out->host_prep_us += k.host_prep_us;
        out->host_finish_us += k.host_finish_us;
        out->host_enqueue_us += k.host_enqueue_us;
    }
    return SZG_OK;
}

int szg_reset_stats(szg_index *ix)
{
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->stats = szg_stats{};
    ix->mask_h2d = ix->mask_d2d = ix->mask_shared = 0;  // (szg_mask_stats' counters; live masks stay counted)
    ix->mx_masked_launches = ix->mx_masked_skip = ix->mx_masked_queries = 0;  // (szg_debug_sketch_masked's)
    ix->sk_topk = szg_sketch_topk_stats{};  // (szg_index_sketch_topk_stats')
    ix->qp = szg_query_prep_stats{};        // (szg_index_query_prep_stats')
    if (ix->sketch) {
        std::lock_guard<std::mutex> lk2(ix->sketch->stats_mu);
        ix->sketch->stats = szg_stats{};
        ix->sketch->mask_h2d = ix->sketch->mask_d2d = ix->sketch->mask_shared = 0;
        ix->sketch->mx_masked_launches = ix->sketch->mx_masked_skip = ix->sketch->mx_masked_queries = 0;
    }
    return SZG_OK;
}

}  // extern "C"

// ---- the options (options.h has the table: names, ranges, texts, stores and the two flags of each row)
static_assert(kCarryStageMax == kCarryStageBytes, "carry_stage_bytes: up to the default window");

// "contexts": value of the shard's contexts stay in rotation, the others are parked (call while no search is in flight)
static void contexts_apply(szg_index *ix, int64_t value)
{
    ix->n_ctx_active = (int)value;
    for (Shard *sh : ix->shards) {
        std::lock_guard<std::mutex> lk(sh->mu);
        while (!sh->parked_ctx.empty()) {
            sh->free_ctx.push_back(sh->parked_ctx.back());
            sh->parked_ctx.pop_back();
        }
        // the contexts with the highest numbers leave the rotation, whatever order earlier calls returned them in:
        // a one-sweep call keeps to the lowest numbers (one_sweep_contexts)
        std::sort(sh->free_ctx.begin(), sh->free_ctx.end(), [](const Ctx *a, const Ctx *b) { return a->no < b->no; });
        while ((int64_t)sh->free_ctx.size() > value) {
            sh->parked_ctx.push_back(sh->free_ctx.back());
            sh->free_ctx.pop_back();
        }
    }
}

// the one path by which an accepted value reaches a handle: szg_set_option, its forward and the replay
static void option_apply(szg_index *ix, const OptionRow *row, int64_t value)
{
    if (row->store == OptionStore::kContexts) contexts_apply(ix, value);
    else option_store(row, ix, value);
}

// The sketch index follows the forwarded options: those set on `ix` so far, with the values it holds now (the last
// accepted "contexts" is n_ctx_active: a search may hold contexts while this runs), applied to its new sketch index.
// In table order: no row's acceptance depends on another row's value ("contexts" is held
// against n_ctx, which is the same constant on both), so the order the caller set them in does not matter.
void szgi::options_replay(szg_index *ix, szg_index *sketch)
{
    int n = 0;
    const OptionRow *rows = option_rows(&n);
    for (int i = 0; i < n; i++)
        if (ix->opt_set >> i & 1)
            option_apply(sketch, &rows[i], rows[i].store == OptionStore::kContexts ? ix->n_ctx_active : option_load(&rows[i], *ix));
}

extern "C" {

int szg_debug_option_check(const char *name, int64_t value)
{
    if (!name) return fail(SZG_E_INVALID, "null argument");
    const OptionRow *row = option_find(name);
    if (!row || !row->scan_check) return fail(SZG_E_INVALID, "not an option of the one-sweep kernel");
    const char *why = option_refusal(row, value);
    return why ? fail(SZG_E_INVALID, why) : SZG_OK;
}

int szg_set_option(szg_index *ix, const char *name, int64_t value)
{
    SZG_TRY
    if (!ix || !name) return fail(SZG_E_INVALID, "null argument");
    const OptionRow *row = option_find(name);
    if (!row) return fail(SZG_E_INVALID, "unknown option");
    if (const char *why = option_refusal(row, value)) return fail(SZG_E_INVALID, why);
    if (row->store == OptionStore::kContexts && value > ix->n_ctx) return fail(SZG_E_INVALID, row->refusal);
    option_apply(ix, row, value);
    if (row->forwarded) {  // the sketch index follows (options_replay: when it is created)
        int n = 0;
        ix->opt_set |= 1ull << (row - option_rows(&n));
        if (ix->sketch) option_apply(ix->sketch, row, value);
    }
    return SZG_OK;
    SZG_CATCH
}

// test hook: what an option holds, on the handle or (on_sketch) on its sketch index; never syncs.  "contexts": the
// contexts in rotation on the first shard that has any -- the free ones, no search being in flight
int szg_debug_option_get(szg_index *ix, const char *name, int on_sketch, int64_t *out)
{
    if (!ix || !name || !out) return fail(SZG_E_INVALID, "null argument");
    const OptionRow *row = option_find(name);
    if (!row) return fail(SZG_E_INVALID, "unknown option");
    std::unique_lock<std::mutex> lk(ix->sk_mu, std::defer_lock);
    if (on_sketch) {
        lk.lock();
        if (!ix->sketch) return fail(SZG_E_UNSUPPORTED, "no sketch index yet");
        ix = ix->sketch;
    }
    *out = option_load(row, *ix);
    if (row->store == OptionStore::kContexts)
        for (Shard *sh : ix->shards) {
            std::lock_guard<std::mutex> lks(sh->mu);
            if (sh->all_ctx.empty()) continue;
            *out = (int64_t)sh->free_ctx.size();
            break;
        }
    return SZG_OK;
}

}  // extern "C"
