// scan_api.cpp -- the search entry points of include/syzgy_scan.h.
//
// Host side of the drop-in: owns the HBM mirror of a Collection's packed
// vectors and runs, per batch of queries, the pipeline
//     H2D queries -> fused scan (query-major, one launch per batch)
//                 -> list merges -> float64 rerank -> D2H
// on pooled HIP streams, then does the reference's result assembly on the few
// survivors: certification of the candidate set, the container/heap replay of
// consider() (collection.go:598-619) and the ascending pop loop (:694-697).
//
// There is no CPU scan in here: without a usable gfx950 device every entry
// point that computes fails with SZG_E_NODEVICE.
#include "scan_internal.h"

using namespace szgi;

namespace szgi {

szg_cert_record cert_record(int query, int pass)
{
    szg_cert_record r;
    memset(&r, 0, sizeof(r));
    r.query = query;
    r.pass = pass;
    r.keys = r.certified = r.k = -1;
    r.thr_min = r.kmax = r.thr = r.eps = r.D = r.slack = NAN;
    return r;
}

szg_cert_record cert_record(const szg_index *ix, int query, int pass)
{
    szg_cert_record r = cert_record(query, pass);
    for (const Shard *sh : ix->shards) r.row_hi = std::max<uint64_t>(r.row_hi, sh->first + sh->n_rows);
    return r;
}

bool cert_room(szg_index *ix, size_t n)
{
    CertTrace &t = ix->cert;
    std::lock_guard<std::mutex> lk(t.mu);
    if (!t.on.load()) return false;
    if (t.recs.size() < kCertMaxRecords && n <= kCertMaxEntries && t.entries.size() + n <= kCertMaxEntries) return true;
    t.dropped++;
    return false;
}

void cert_emit(szg_index *ix, szg_cert_record r, const std::vector<szg_cert_entry> &entries)
{
    CertTrace &t = ix->cert;
    std::lock_guard<std::mutex> lk(t.mu);
    if (!t.on.load()) return;  // (switched off since the caller looked)
    if (t.recs.size() >= kCertMaxRecords || t.entries.size() + entries.size() > kCertMaxEntries) {
        t.dropped++;
        return;
    }
    try {
        r.first_entry = t.entries.size();
        r.n_entries = entries.size();
        t.entries.insert(t.entries.end(), entries.begin(), entries.end());
        t.recs.push_back(r);
    } catch (const std::bad_alloc &) {
        t.entries.resize(std::min<size_t>(t.entries.size(), (size_t)r.first_entry));
        t.dropped++;
    }
}

}  // namespace szgi

extern "C" {

// The reference's float64 distance from one query to each listed row
int szg_distances(szg_index *ix, const double *query, const uint64_t *rows, uint64_t n, double *out_dist)
{
    SZG_TRY
    if (!ix || !query || (!rows && n) || (!out_dist && n)) return fail(SZG_E_INVALID, "null argument");
    if (n == 0) return SZG_OK;
    const uint64_t total = szg_index_rows(ix);
    for (uint64_t i = 0; i < n; i++)
        if (rows[i] < ix->row_base || rows[i] - ix->row_base >= total) return fail(SZG_E_RANGE, "row out of range");
    for (Shard *sh : ix->shards) {
        if (sh->n_rows == 0) continue;
        std::vector<uint64_t> cands;
        std::vector<uint64_t> where;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t r = rows[i] - ix->row_base;
            if (r >= sh->first && r < sh->first + sh->n_rows) {
                cands.push_back(r - sh->first);  // key bits 0, row in the low word
                where.push_back(i);
            }
        }
        if (cands.empty()) continue;
        Ctx *c = ctx_acquire(sh);
        CtxGuard guard{sh, c};
        int rc = SZG_OK;
        auto body = [&]() -> int {
            HIPCHK(hipSetDevice(sh->device));
            memcpy(c->h_q64, query, sizeof(double) * ix->dim);
            HIPCHK(hipMemcpyAsync(c->d_q64, c->h_q64, sizeof(double) * ix->dim, hipMemcpyHostToDevice,
                                  c->stream));
            int r2 = c->d_collect.ensure(cands.size());
            if (r2) return r2;
            r2 = c->d_out.ensure(cands.size());
            if (r2) return r2;
            r2 = c->h_out.ensure(cands.size());
            if (r2) return r2;
            HIPCHK(hipMemcpyAsync(c->d_collect, cands.data(), cands.size() * sizeof(uint64_t),
                                  hipMemcpyHostToDevice, c->stream));
            HIPCHK(szg::launch_rerank(ix->bits, ix->metric, sh->rows, ix->layout, ix->dim, c->d_q64,
                                      c->d_collect, nullptr, (uint32_t)cands.size(), 1, c->d_out, c->stream));
            HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, sizeof(szg::RerankOut) * cands.size(),
                                  hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            for (size_t i = 0; i < cands.size(); i++) out_dist[where[i]] = c->h_out[i].dist;
            return SZG_OK;
        };
        rc = body();
        if (rc) return rc;
    }
    return SZG_OK;
    SZG_CATCH
}

// decodeVector + dequantize on the host (collection.go:768-794, quantization.go:25-36);
// integer -> float64 conversions, one correctly rounded division, exact *2 and -1
static void decode_row_host(const uint8_t *data, int dim, int q, double *out)
{
    for (int i = 0; i < dim; i++) {
        uint64_t v = 0;
        switch (q) {
        case 4: v = (i % 2 == 0) ? (uint64_t)(data[i / 2] >> 4) : (uint64_t)(data[i / 2] & 0x0F); break;
        case 8: v = data[i]; break;
        case 16: v = ((uint64_t)data[i * 2] << 8) | data[i * 2 + 1]; break;
        case 32: for (int b = 0; b < 4; b++) v = (v << 8) | data[i * 4 + b]; break;
        default: for (int b = 0; b < 8; b++) v = (v << 8) | data[i * 8 + b]; break;
        }
        if (q == 32) {
            const uint32_t u = (uint32_t)v;
            float f;
            memcpy(&f, &u, 4);
            out[i] = (double)f;
        } else if (q == 64) {
            memcpy(&out[i], &v, 8);
        } else {
            const double maxInt = (double)((1ull << q) - 1);
            const double t = (double)v / maxInt;
            out[i] = t * 2 - 1;
        }
    }
}

int szg_pair_distances(szg_index *ix, const uint64_t *rows_a, const uint64_t *rows_b, uint64_t n_pairs,
                       double *out_dist)
{
    SZG_TRY
    if (!ix || ((!rows_a || !rows_b || !out_dist) && n_pairs)) return fail(SZG_E_INVALID, "null argument");
    if (n_pairs == 0) return SZG_OK;
    const uint64_t total = szg_index_rows(ix);
    for (uint64_t i = 0; i < n_pairs; i++)
        if (rows_a[i] < ix->row_base || rows_a[i] - ix->row_base >= total || rows_b[i] < ix->row_base ||
            rows_b[i] - ix->row_base >= total)
            return fail(SZG_E_RANGE, "row out of range");
    std::vector<uint8_t> done(n_pairs, 0);
    // pairs whose two rows live in one shard: both decoded and compared on the device, one launch per shard
    for (Shard *sh : ix->shards) {
        if (sh->n_rows == 0) continue;
        std::vector<uint32_t> left;
        std::vector<uint64_t> right, where;
        for (uint64_t i = 0; i < n_pairs; i++) {
            const uint64_t a = rows_a[i] - ix->row_base, b = rows_b[i] - ix->row_base;
            if (a >= sh->first && a < sh->first + sh->n_rows && b >= sh->first && b < sh->first + sh->n_rows) {
                left.push_back((uint32_t)(a - sh->first));
                right.push_back(b - sh->first);
                where.push_back(i);
            }
        }
        if (where.empty()) continue;
        Ctx *c = ctx_acquire(sh);
        CtxGuard guard{sh, c};
        HIPCHK(hipSetDevice(sh->device));
        const size_t n = where.size();
        int rc = c->d_collect.ensure(n + (n + 1) / 2);  // right rows (u64) + left rows (u32)
        if (rc) return rc;
        rc = c->d_out.ensure(n);
        if (rc) return rc;
        rc = c->h_out.ensure(n);
        if (rc) return rc;
        uint32_t *d_left = reinterpret_cast<uint32_t *>(c->d_collect + n);
        HIPCHK(hipMemcpyAsync(c->d_collect, right.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_left, left.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(szg::launch_rerank_pairs(ix->bits, ix->metric, sh->rows, ix->layout, ix->dim, d_left, c->d_collect,
                                        (uint32_t)n, c->d_out, c->stream));
        HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, sizeof(szg::RerankOut) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // also keeps `left` / `right` alive until the copies are done
        for (size_t i = 0; i < n; i++) {
            out_dist[where[i]] = c->h_out[i].dist;
            done[where[i]] = 1;
        }
    }
    // pairs that straddle two shards (devices): the left row is read back, decoded as the reference
    // does and sent as the query of a szg_distances call on the right row's shard
    std::vector<uint8_t> bytes((size_t)szg_row_bytes(ix->bits, ix->dim));
    std::vector<double> vec(ix->dim);
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (done[i]) continue;
        int rc = szg_index_read_rows(ix, rows_a[i] - ix->row_base, 1, bytes.data());
        if (rc) return rc;
        decode_row_host(bytes.data(), ix->dim, ix->bits, vec.data());
        rc = szg_distances(ix, vec.data(), &rows_b[i], 1, &out_dist[i]);
        if (rc) return rc;
    }
    return SZG_OK;
    SZG_CATCH
}

}  // extern "C"

namespace {

// min(total, capacity) closest hits of a radius search into the caller's buffers (global rows)
int radius_output(const szg_index *ix, const std::vector<HeapItem> &hits, uint64_t *out_rows, double *out_dist,
                  uint64_t capacity, uint64_t *out_total)
{
    const uint64_t total = hits.size();
    *out_total = total;
    for (uint64_t i = 0; i < total && i < capacity; i++) {
        out_rows[i] = hits[i].row + ix->row_base;
        out_dist[i] = hits[i].priority;
    }
    if (total > capacity) return fail(SZG_E_TRUNCATED, "radius search: capacity too small");
    return SZG_OK;
}

// One batch of coalesced single-query callers of the same kind (top-k with the same k, or radius searches -- each
// with its own radius): answered through one call of the batch path, results handed to every caller's own buffers.
struct BatchScratch {
    std::vector<double> q, dist, radii;
    std::vector<uint64_t> rows;
    std::vector<int32_t> count;
    std::vector<const uint64_t *> masks;
    std::vector<const szg_mask *> handles;
    std::vector<std::vector<HeapItem>> hits;
};

void serve_batch(szg_index *ix, const std::vector<PendingSearch *> &batch, BatchScratch &w)
{
    const int nq = (int)batch.size();
    const bool radius = batch[0]->radius > 0;
    int rc = SZG_OK;
    try {
        w.q.resize((size_t)nq * ix->dim);
        w.masks.resize(nq);
        w.handles.resize(nq);
        bool any = false, raw = false, resident = false;
        for (int i = 0; i < nq; i++) {
            memcpy(&w.q[(size_t)i * ix->dim], batch[i]->query, sizeof(double) * ix->dim);
            w.masks[i] = batch[i]->allow;  // each caller's own filter, if it has one
            w.handles[i] = batch[i]->handle;  // ... or its resident mask
            raw |= w.masks[i] != nullptr;
            resident |= w.handles[i] != nullptr;
        }
        // callers with raw words beside callers with resident masks: everything through the host path, with the
        // handles' host words
        if (raw && resident) {
            for (int i = 0; i < nq; i++)
                if (w.handles[i]) w.masks[i] = mask_host_words(w.handles[i]);
            resident = false;
        }
        any = raw || resident;
        const szg_mask *const *hptr = resident ? w.handles.data() : nullptr;
        if (radius) {
            w.radii.resize(nq);
            for (int i = 0; i < nq; i++) w.radii[i] = batch[i]->radius;
            rc = search_radius_any(ix, w.q.data(), nq, w.radii.data(), any ? w.masks.data() : nullptr, &w.hits);
            for (int i = 0; i < nq; i++) {
                PendingSearch *p = batch[i];
                p->rc = rc ? rc : radius_output(ix, w.hits[i], p->out_rows, p->out_dist, p->capacity, p->out_total);
            }
            return;
        }
        const int kk = batch[0]->k;
        if (nq == 1) {
            PendingSearch *p = batch[0];
            rc = search_topk_any(ix, p->query, 1, kk, p->allow, p->out_rows, p->out_dist, p->out_count, nullptr,
                                 p->handle ? &p->handle : nullptr);
        } else {
            w.rows.resize((size_t)nq * kk);
            w.dist.resize((size_t)nq * kk);
            w.count.resize(nq);
            rc = search_topk_any(ix, w.q.data(), nq, kk, nullptr, w.rows.data(), w.dist.data(), w.count.data(),
                                 any && !hptr ? w.masks.data() : nullptr, hptr);
            for (int i = 0; i < nq && rc == SZG_OK; i++) {
                memcpy(batch[i]->out_rows, &w.rows[(size_t)i * kk], sizeof(uint64_t) * kk);
                memcpy(batch[i]->out_dist, &w.dist[(size_t)i * kk], sizeof(double) * kk);
                if (batch[i]->out_count) *batch[i]->out_count = w.count[i];
            }
        }
    } catch (const std::bad_alloc &) {
        rc = fail(SZG_E_NOMEM, "out of memory (host)");
    } catch (...) {
        rc = fail(SZG_E_DEVICE, "unexpected exception");
    }
    for (PendingSearch *p : batch) p->rc = rc;
}

// Search holds only RLock in the reference (collection.go:570), so many goroutines call in at once, each with ONE
// query.  Whoever finds no batch in flight becomes the leader: it answers everything that is waiting and is of one
// kind as one batch (one shared sweep, or one query-major collect launch, instead of one launch per caller), then
// hands the lead to a waiter once its own answer has arrived.  A lone caller is its own batch of one and pays
// nothing for this.
int combine(szg_index *ix, PendingSearch &me)
{
    std::vector<PendingSearch *> batch;
    std::unique_lock<std::mutex> lk(ix->comb_mu);
    try {
        batch.reserve(kMaxBatch);  // nothing below that touches the combiner's state may throw
        ix->comb_waiting.push_back(&me);
    } catch (...) {
        return fail(SZG_E_NOMEM, "out of memory (host)");
    }
    if (ix->comb_leader) {
        me.cv.wait(lk, [&] { return me.done || me.lead; });
        if (me.done) {
            if (me.rc) (void)fail(me.rc, szg_strerror(me.rc));  // (the error text lives on the leader's thread)
            return me.rc;
        }
    }
    ix->comb_leader = true;
    BatchScratch scratch;
    while (!me.done) {
        batch.clear();
        const PendingSearch *head = ix->comb_waiting.front();  // never empty here: `me` is in it until done
        const bool radius = head->radius > 0;
        for (auto it = ix->comb_waiting.begin(); it != ix->comb_waiting.end() && batch.size() < (size_t)kMaxBatch;) {
            const bool same = radius ? (*it)->radius > 0 : ((*it)->radius == 0 && (*it)->k == head->k);
            if (same) {
                batch.push_back(*it);  // within the reserved capacity
                it = ix->comb_waiting.erase(it);
            } else {
                ++it;
            }
        }
        lk.unlock();
        serve_batch(ix, batch, scratch);
        lk.lock();
        for (PendingSearch *p : batch) {
            p->done = true;
            if (p != &me) p->cv.notify_one();
        }
    }
    if (!ix->comb_waiting.empty()) {
        ix->comb_waiting.front()->lead = true;  // it stays queued and forms the next batch itself
        ix->comb_waiting.front()->cv.notify_one();
    } else {
        ix->comb_leader = false;
    }
    return me.rc;
}

}  // namespace

extern "C" {

int szg_search_topk(szg_index *ix, const double *queries, int n_queries, int k,
                    const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist,
                    int32_t *out_count)
{
    if (!ix || !queries || !out_rows || !out_dist) return fail(SZG_E_INVALID, "null argument");
    if (n_queries < 0 || k <= 0) return fail(SZG_E_INVALID, "k must be > 0 (K==0 is listing mode, collection.go:633)");
    if (n_queries == 0) return SZG_OK;
    if (szg_index_rows(ix) == 0) {  // empty collection -> no results (collection_test.go:294-309)
        for (size_t i = 0; i < (size_t)n_queries * k; i++) {
            out_rows[i] = UINT64_MAX;
            out_dist[i] = 0.0;
        }
        if (out_count) for (int i = 0; i < n_queries; i++) out_count[i] = 0;
        return SZG_OK;
    }
    if (!(ix->coalesce && n_queries == 1 && ix->multi_query)) {
        SZG_TRY
        return search_topk_any(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count);
        SZG_CATCH
    }
    PendingSearch me;
    me.query = queries;
    me.allow = allow_bits;
    me.k = k;
    me.out_rows = out_rows;
    me.out_dist = out_dist;
    me.out_count = out_count;
    return combine(ix, me);
}

int szg_search_topk_masked(szg_index *ix, const double *queries, int n_queries, int k, const szg_mask *const *masks,
                           int n_masks, uint64_t *out_rows, double *out_dist, int32_t *out_count)
{
    const szg_mask *lone = nullptr;
    {
        SZG_TRY
        const int rc = search_topk_masked_prepare(ix, queries, n_queries, k, masks, n_masks, out_rows, out_dist, out_count, &lone);
        if (rc || !lone) return rc;
        SZG_CATCH
    }
    PendingSearch me;  // a lone query: answered together with whoever else is waiting (combine)
    me.query = queries;
    me.allow = nullptr;
    me.handle = lone;
    me.k = k;
    me.out_rows = out_rows;
    me.out_dist = out_dist;
    me.out_count = out_count;
    return combine(ix, me);
}

int szg_search_radius(szg_index *ix, const double *query, double radius,
                      const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist,
                      uint64_t capacity, uint64_t *out_total)
{
    if (!ix || !query || !out_total) return fail(SZG_E_INVALID, "null argument");
    if (!(radius > 0)) return fail(SZG_E_INVALID, "radius must be > 0 (collection.go:598)");
    if (capacity && (!out_rows || !out_dist)) return fail(SZG_E_INVALID, "null output buffer");
    *out_total = 0;
    if (szg_index_rows(ix) == 0) return SZG_OK;
    if (!ix->coalesce) {
        SZG_TRY
        std::vector<std::vector<HeapItem>> hits;
        const int rc = search_radius_any(ix, query, 1, &radius, allow_bits ? &allow_bits : nullptr, &hits);
        if (rc) return rc;
        return radius_output(ix, hits[0], out_rows, out_dist, capacity, out_total);
        SZG_CATCH
    }
    // concurrent callers (the reference's Searches under RLock) share query-major collect launches
    PendingSearch me;
    me.query = query;
    me.allow = allow_bits;
    me.k = 0;
    me.radius = radius;
    me.out_rows = out_rows;
    me.out_dist = out_dist;
    me.capacity = capacity;
    me.out_total = out_total;
    return combine(ix, me);
}

int szg_search_radius_batch(szg_index *ix, const double *queries, int n_queries, const double *radii,
                            const uint64_t *allow_bits, uint64_t *out_rows, double *out_dist, uint64_t capacity,
                            uint64_t *out_offsets)
{
    SZG_TRY
    if (!ix || !queries || !radii || !out_offsets) return fail(SZG_E_INVALID, "null argument");
    if (n_queries < 0) return fail(SZG_E_INVALID, "n_queries < 0");
    if (capacity && (!out_rows || !out_dist)) return fail(SZG_E_INVALID, "null output buffer");
    for (int i = 0; i < n_queries; i++)
        if (!(radii[i] > 0)) return fail(SZG_E_INVALID, "radius must be > 0 (collection.go:598)");
    for (int i = 0; i <= n_queries; i++) out_offsets[i] = 0;
    const uint64_t total_rows = szg_index_rows(ix);
    if (n_queries == 0 || total_rows == 0) return SZG_OK;
    const size_t words = (size_t)((total_rows + 63) / 64);
    std::vector<const uint64_t *> masks;
    if (allow_bits) {
        masks.resize(n_queries);
        for (int i = 0; i < n_queries; i++) masks[i] = allow_bits + (size_t)i * words;
    }
    std::vector<std::vector<HeapItem>> hits;
    const int rc = search_radius_any(ix, queries, n_queries, radii, allow_bits ? masks.data() : nullptr, &hits);
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

// test hook: device float64 primitives (0 div, 1 sqrt, 2 go acos, 3 round, 4 f32 narrowing)
int szg_debug_f64_probe(int op, const double *a, const double *b, double *out, uint64_t n)
{
    if (!a || !out) return fail(SZG_E_INVALID, "null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(SZG_E_NODEVICE, "hipGetDeviceCount");
    DevBuf<double> da, db, dout;
    int rc = da.ensure((size_t)n);
    if (rc == SZG_OK) rc = db.ensure((size_t)n);
    if (rc == SZG_OK) rc = dout.ensure((size_t)n);
    if (rc) return rc;
    HIPCHK(hipMemcpy(da, a, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b ? b : a, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(szg::launch_f64_probe(op, da, db, dout, n, nullptr));
    HIPCHK(hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost));
    return SZG_OK;
}

// test hooks, host only (dev_mem.h): the device blocks the library's owning buffers hold in this process and their bytes;
// and the countdown that refuses the nth device allocation from now on (0 disarms)
int szg_debug_device_memory(uint64_t *out_blocks, uint64_t *out_bytes)
{
    if (out_blocks) *out_blocks = dev_alloc_state().blocks.load();
    if (out_bytes) *out_bytes = dev_alloc_state().bytes.load();
    return SZG_OK;
}

int szg_debug_refuse_device_alloc(int64_t nth)
{
    if (nth < 0) return fail(SZG_E_INVALID, "nth is 0 (disarm) or the allocation to refuse, counted from 1");
    dev_alloc_state().refuse_in.store(nth);
    return SZG_OK;
}

// test hook: the certificate trace (include/syzgy_scan.h).  Switching clears; reading copies out and empties.
int szg_debug_trace_certificates(szg_index *ix, int on)
{
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->cert.mu);
    ix->cert.recs.clear();
    ix->cert.entries.clear();
    ix->cert.recs.shrink_to_fit();
    ix->cert.entries.shrink_to_fit();
    ix->cert.dropped = 0;
    ix->cert.on.store(on != 0);
    return SZG_OK;
}

int szg_debug_certificates(szg_index *ix, szg_cert_record *records, uint64_t record_capacity, szg_cert_entry *entries,
                           uint64_t entry_capacity, uint64_t *out_records, uint64_t *out_entries, uint64_t *out_dropped)
{
    if (!ix) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->cert.mu);
    CertTrace &t = ix->cert;
    if (out_records) *out_records = t.recs.size();
    if (out_entries) *out_entries = t.entries.size();
    if (out_dropped) *out_dropped = t.dropped;
    if (!records || !entries) return SZG_OK;
    if (record_capacity < t.recs.size() || entry_capacity < t.entries.size())
        return fail(SZG_E_TRUNCATED, "certificate trace: buffers too small");
    if (!t.recs.empty()) memcpy(records, t.recs.data(), t.recs.size() * sizeof(szg_cert_record));
    if (!t.entries.empty()) memcpy(entries, t.entries.data(), t.entries.size() * sizeof(szg_cert_entry));
    t.recs.clear();
    t.entries.clear();
    return SZG_OK;
}

// test hooks: the sketch index's state, read only (scan_sketch.cpp; include/syzgy_scan.h)
int szg_debug_sketch_info(szg_index *ix, szg_sketch_info *out, uint64_t *out_exc_rows, uint64_t exc_capacity)
{
    SZG_TRY
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    if (ix->bits != 32 && ix->bits != 64) return fail(SZG_E_INVALID, "sketch info: only float32 and float64 handles keep a sketch");
    return sketch_debug_info(ix, out, out_exc_rows, exc_capacity);
    SZG_CATCH
}

int szg_debug_sketch_rows(szg_index *ix, uint64_t first_row, uint64_t n_rows, uint8_t *out, uint64_t *out_live_words,
                          uint64_t live_capacity)
{
    SZG_TRY
    if (!ix || (!out && n_rows)) return fail(SZG_E_INVALID, "null argument");
    if (ix->bits != 32 && ix->bits != 64) return fail(SZG_E_INVALID, "sketch rows: only float32 and float64 handles keep a sketch");
    return sketch_debug_rows(ix, first_row, n_rows, out, out_live_words, live_capacity);
    SZG_CATCH
}

}  // extern "C"

// ---- the plan hooks (test hooks, host only; include/syzgy_scan.h says what each answers): what a one-sweep call would
// do, from the functions the launch path calls (row_format, scan_geometry, scan_variant, scan_lds_bytes, and sketch_plan.h
// for a call through the sketch), so tests derive their shapes from the code's own rules.
namespace {

// a hook's argument that stands for the option stored in `member`: held to that option's range, refused with its text
int hook_option(int Options::*member, int value)
{
    const char *why = option_refusal(option_of(member), value);
    return why ? fail(SZG_E_INVALID, why) : SZG_OK;
}

// the option arguments the hooks share, checked in this order; null = the hook has no such argument
int hook_options(const int *planes, const int *scan_group, const int *sketch_matrix, const int *sketch_select, const int *sketch_wide)
{
    if (planes && *planes != 2 && *planes != 3) return fail(SZG_E_INVALID, "planes is 2 or 3");
    int rc = scan_group ? hook_option(&Options::scan_group, *scan_group) : SZG_OK;
    if (!rc && sketch_matrix) rc = hook_option(&Options::sketch_matrix, *sketch_matrix);
    if (!rc && sketch_select) rc = hook_option(&Options::sketch_select, *sketch_select);
    if (!rc && sketch_wide) rc = hook_option(&Options::sketch_wide, *sketch_wide);
    return rc;
}

// One hook's call: the rows of (dim, quant_bits), the geometry of a sweep over them, the record of one launch -- the hook
// names what it sets behind `block` -- and what walking the call's launches over that record finds.
struct PlanHook {
    RowFormat f;
    LaunchGeom g;
    szg::ScanPlanIn in;
    SketchShape s;           // (sketch_rows) the sketch index of the hook's arguments, under the default batch and launch sizes
    szg::ScanVariant first;  // the first launch's variant and LDS bytes
    uint64_t lds_bytes;
    int32_t passes;          // over the rows, of all launches (what launch_scans_chained adds to szg_stats.scan_bytes)
    // (tiled: the caller may only take the tiled layout away from a format that has it)
    int rows(int dim, int quant_bits, int tiled, int kp, bool collect, int masked, uint64_t n_rows = 1u << 22, int cu_count = 256)
    {
        const int rc = row_format(dim, quant_bits, &f);
        if (rc == SZG_E_UNSUPPORTED) return fail(rc, "dimension too large for the LDS-resident query");
        if (rc) return rc;
        g = scan_geometry(quant_bits, f.map, f.row_bytes, f.layout.tiled != 0, n_rows, cu_count, kp);
        in = szg::ScanPlanIn{quant_bits, f.map, f.layout.tiled != 0 && tiled != 0, kp, collect, masked != 0, szg_index::ring,
                             !szg_index::shape_kernels};
        in.block = g.block;
        return SZG_OK;
    }
    // ... for the hooks of the sketch's launches: the options they take, checked and filled in (an option a hook does not
    // know: the value that leaves the form out).  kp is the launches' list length, whatever the grid: sketch_list = kp.
    int sketch_rows(int dim, int quant_bits, int kp, bool collect, int planes, int norms, int tiled, int masked, int scan_group,
                    int sketch_matrix, const int *sketch_select, const int *sketch_wide, int sketch_share = 1, int sketch_masked = 0)
    {
        if (const int rc = hook_options(&planes, &scan_group, &sketch_matrix, sketch_select, sketch_wide)) return rc;
        if (const int rc = rows(dim, quant_bits, tiled, kp, collect, masked)) return rc;
        s = SketchShape{quant_bits, f.map, in.tiled, in.ring, in.no_shape_kernels, scan_group, planes, 0, sketch_matrix,
                        sketch_select ? *sketch_select : 0, sketch_wide ? *sketch_wide : 1, sketch_share, sketch_masked, kp,
                        16, szg::kMaxSweepsPerLaunch, norms != 0};
        in = sketch_plan_in(s, kp, collect, masked != 0, 1, g.block);
        return SZG_OK;
    }
    // ... and for the two that answer a whole top-k call through the sketch: its batches, launches and passes
    SketchCallWalk call(int kp, int n_queries) const { return sketch_call_walk(s, g.grid, g.block, kp, n_queries, in.masked, true); }
    // the call's n_queries queries as launches of up to per_launch
    void walk(int n_queries, int per_launch)
    {
        passes = 0;
        for (int j = 0; j < n_queries; j += per_launch) {
            in.n_queries = std::min(per_launch, n_queries - j);
            const szg::ScanVariant v = szg::scan_variant(in);
            if (j == 0) {
                first = v;
                lds_bytes = szg::scan_lds_bytes(in.qbits, in.map, in.kp, in.block, v.group, in.planes, v.matrix_blocks());
            }
            passes += launch_passes(in);
        }
    }
    // launches of 32 where one qualifies for the two-block form, else of 16
    int wide_launches()
    {
        walk(szg::kMatrixWideQueries, szg::kMatrixWideQueries);
        return first.wide ? szg::kMatrixWideQueries : szg::kMaxSweepsPerLaunch;
    }
};

}  // namespace

extern "C" {

// the lane map, launch geometry and kernel variant a sweep over n_rows rows would take
int szg_debug_scan_plan(int dim, int quant_bits, uint64_t n_rows, int kp, int collect, int masked, int cu_count, szg_scan_plan *out)
{
    if (!out) return fail(SZG_E_INVALID, "out is null");
    if (kp < 0 || cu_count < 0) return fail(SZG_E_INVALID, "kp or cu_count negative");
    PlanHook h;  // (collect sweeps keep no lists)
    if (const int rc = h.rows(dim, quant_bits, 1, collect ? 0 : kp, collect != 0, masked, n_rows, cu_count ? cu_count : 256)) return rc;
    const szg::ScanVariant v = szg::scan_variant(h.in);
    const szg::RowMap &m = h.f.map;
    *out = szg_scan_plan{m.r16,    m.L,       m.P,          m.gpw,    m.pow2,        m.dense,           (int32_t)h.f.layout.tiled,
                         h.g.grid, h.g.block, v.ring_depth, v.shaped, v.nontemporal, h.g.rows_per_block};
    return SZG_OK;
}

// the groups a one-sweep call forms
int szg_debug_scan_group(int dim, int quant_bits, int kp, int collect, int masked, int scan_group, int n_queries,
                         int queries_per_launch, int32_t *group, uint64_t *lds_bytes, int32_t *passes)
{
    if (!group || !lds_bytes || !passes) return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1 || queries_per_launch < 1 || queries_per_launch > szg::kMaxSweepsPerLaunch)
        return fail(SZG_E_INVALID, "kp, n_queries or queries_per_launch out of range");
    if (const int rc = hook_options(nullptr, &scan_group, nullptr, nullptr, nullptr)) return rc;
    PlanHook h;
    if (const int rc = h.rows(dim, quant_bits, 1, collect ? 0 : kp, collect != 0, masked)) return rc;
    h.in.group = scan_group;
    h.walk(n_queries, queries_per_launch);
    *group = h.first.group;
    *lds_bytes = h.lds_bytes;
    *passes = h.passes;
    return SZG_OK;
}

// does the matrix sweep serve a one-sweep call, in launches of up to 16 (the default queries_per_launch)?
int szg_debug_scan_matrix(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                          int scan_group, int sketch_matrix, int32_t *serves, int32_t *passes, uint64_t *lds_bytes, int32_t *steps_form)
{
    if (!serves || !passes || !lds_bytes || !steps_form) return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1) return fail(SZG_E_INVALID, "kp or n_queries out of range");
    PlanHook h;
    if (const int rc = h.sketch_rows(dim, quant_bits, kp, false, planes, norms, tiled, masked, scan_group, sketch_matrix, nullptr, nullptr))
        return rc;
    h.walk(n_queries, szg::kMaxSweepsPerLaunch);
    *serves = h.first.matrix;
    *steps_form = h.first.matrix_steps;
    *lds_bytes = h.lds_bytes;
    *passes = h.passes;
    return SZG_OK;
}

// which selection the first launch (of up to 16 queries) of a one-sweep call takes under option sketch_select
int szg_debug_scan_select(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                          int scan_group, int sketch_matrix, int sketch_select, int32_t *serves, int32_t *row_lists)
{
    if (!serves || !row_lists) return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1) return fail(SZG_E_INVALID, "kp or n_queries out of range");
    PlanHook h;
    if (const int rc = h.sketch_rows(dim, quant_bits, kp, false, planes, norms, tiled, masked, scan_group, sketch_matrix, &sketch_select, nullptr))
        return rc;
    h.walk(std::min(szg::kMaxSweepsPerLaunch, n_queries), szg::kMaxSweepsPerLaunch);
    *serves = h.first.matrix;
    *row_lists = h.first.matrix && h.first.row_lists ? 1 : 0;
    return SZG_OK;
}

// the matrix sweep's two-block form (option sketch_wide) for a one-sweep top-k call, split as a call with wide batches
// splits it
int szg_debug_scan_wide(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                        int scan_group, int sketch_matrix, int sketch_select, int sketch_wide, int32_t *serves, int32_t *passes,
                        uint64_t *lds_bytes)
{
    if (!serves || !passes || !lds_bytes) return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1) return fail(SZG_E_INVALID, "kp or n_queries out of range");
    PlanHook h;
    if (const int rc = h.sketch_rows(dim, quant_bits, kp, false, planes, norms, tiled, masked, scan_group, sketch_matrix, &sketch_select, &sketch_wide))
        return rc;
    h.walk(n_queries, h.wide_launches());
    *serves = h.first.wide;
    *lds_bytes = h.lds_bytes;
    *passes = h.passes;
    return SZG_OK;
}

// the matrix sweep's shared form (option sketch_share) for a one-sweep top-k call of n_queries through the sketch under the
// default query_batch and queries_per_launch: whether a launch of min(n_queries, 64) takes it, and the call's batches,
// launches and passes as sketch_plan.h splits it for sketch_call_plan, plan_batch and enqueue_topk (the two parts of a
// short call included)
int szg_debug_scan_share(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                         int scan_group, int sketch_matrix, int sketch_select, int sketch_wide, int sketch_share, int32_t *serves,
                         int32_t *launches, int32_t *passes, int32_t *slices, uint64_t *lds_bytes, int32_t *batches,
                         int32_t batch_capacity, int32_t *n_batches)
{
    if (!serves || !launches || !passes || !slices || !lds_bytes || !n_batches || (!batches && batch_capacity > 0))
        return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1 || batch_capacity < 0) return fail(SZG_E_INVALID, "kp, n_queries or batch_capacity out of range");
    if (const int rc = hook_option(&Options::sketch_share, sketch_share)) return rc;
    PlanHook h;
    if (const int rc = h.sketch_rows(dim, quant_bits, kp, false, planes, norms, tiled, masked, scan_group, sketch_matrix, &sketch_select,
                                     &sketch_wide, sketch_share))
        return rc;
    h.in.n_queries = std::min(n_queries, szg::kMatrixShareQueries);
    const szg::ScanVariant v = szg::scan_variant(h.in);
    *serves = v.share;
    *slices = v.share ? szg::share_slices(szg::share_grid(h.g.grid)) : 0;
    *lds_bytes = szg::scan_lds_bytes(h.in.qbits, h.in.map, h.in.kp, h.in.block, v.group, h.in.planes, v.matrix_blocks());
    const SketchCallWalk w = h.call(kp, n_queries);
    *n_batches = (int32_t)w.batches.size();
    std::copy_n(w.batches.begin(), std::min<size_t>(w.batches.size(), (size_t)batch_capacity), batches);
    *launches = w.launches;
    *passes = w.passes;
    return SZG_OK;
}

// the matrix sweep's masked forms (option sketch_masked) for a one-sweep top-k call of n_queries through the sketch whose
// launches carry masks: the form a launch of min(n_queries, 64) takes, and the call's launches and passes as
// szg_debug_scan_share counts the unmasked call's
int szg_debug_scan_masked(int dim, int quant_bits, int n_queries, int kp, int planes, int norms, int tiled, int masked,
                          int scan_group, int sketch_matrix, int sketch_select, int sketch_wide, int sketch_share, int sketch_masked,
                          int shared_mask, szg_scan_masked_plan *out)
{
    if (!out) return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1) return fail(SZG_E_INVALID, "kp or n_queries out of range");
    if (const int rc = hook_option(&Options::sketch_share, sketch_share)) return rc;
    if (const int rc = hook_option(&Options::sketch_masked, sketch_masked)) return rc;
    PlanHook h;
    if (const int rc = h.sketch_rows(dim, quant_bits, kp, false, planes, norms, tiled, masked, scan_group, sketch_matrix, &sketch_select,
                                     &sketch_wide, sketch_share, sketch_masked))
        return rc;
    h.in.n_queries = std::min(n_queries, szg::kMatrixShareQueries);
    const szg::ScanVariant v = szg::scan_variant(h.in);
    memset(out, 0, sizeof(*out));
    out->serves = v.matrix && v.masked ? 1 : 0;
    out->wide = out->serves && v.wide ? 1 : 0;
    out->share = out->serves && v.share ? 1 : 0;
    out->tile_skip = out->serves && shared_mask ? 1 : 0;
    out->steps_form = out->serves ? v.matrix_steps : 0;
    const SketchCallWalk w = h.call(kp, n_queries);
    out->launches = w.launches;
    out->passes = w.passes;
    return SZG_OK;
}

// what the masked forms served on the handle's sketch index since szg_reset_stats
int szg_debug_sketch_masked(szg_index *ix, szg_sketch_masked_info *out)
{
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    std::lock_guard<std::mutex> lk(ix->sk_mu);
    const szg_index *sk = ix->is_sketch ? ix : ix->sketch;
    if (!sk) return SZG_OK;
    out->launches = sk->mx_masked_launches;
    out->skip_launches = sk->mx_masked_skip;
    out->queries = sk->mx_masked_queries;
    return SZG_OK;
}

// the matrix sweep's collect form for a collect call of n_queries queries with one sweep each (launches of 32: sketch_wide = 2)
int szg_debug_scan_collect(int dim, int quant_bits, int n_queries, int planes, int norms, int tiled, int masked, int scan_group,
                           int sketch_matrix, int sketch_wide, int32_t *serves, int32_t *wide, int32_t *passes, uint64_t *lds_bytes, int32_t *steps_form)
{
    if (!serves || !wide || !passes || !lds_bytes || !steps_form) return fail(SZG_E_INVALID, "null argument");
    if (n_queries < 1) return fail(SZG_E_INVALID, "n_queries out of range");
    PlanHook h;
    if (const int rc = h.sketch_rows(dim, quant_bits, 0, true, planes, norms, tiled, masked, scan_group, sketch_matrix, nullptr, &sketch_wide))
        return rc;
    h.walk(n_queries, sketch_wide == 2 ? h.wide_launches() : szg::kMaxSweepsPerLaunch);
    *serves = h.first.matrix;
    *wide = h.first.wide;
    *steps_form = h.first.matrix_steps;
    *lds_bytes = h.lds_bytes;
    *passes = h.passes;
    return SZG_OK;
}

// test hook, host only: does the one-launch short-list merge serve (n_lists, m, kp), and how many entries under its
// threshold its selection sorts at most (more: the tournament; fewer than kp: the tournament always)
int szg_debug_merge_short_plan(int n_lists, int m, int kp, int32_t *fits, int32_t *sorts)
{
    if (!fits || !sorts) return fail(SZG_E_INVALID, "null argument");
    *fits = szg::merge_short_fits(n_lists, m, kp) ? 1 : 0;
    *sorts = *fits ? szg::merge_short_sorts(n_lists, kp) : 0;
    return SZG_OK;
}

// the ring depth a one-sweep launch takes under options scan_group and scan_group_ring, and the depths the library carries
int szg_debug_scan_group_ring(int dim, int quant_bits, int kp, int scan_group, int n_queries, int scan_group_ring,
                              int32_t *ring_depth, int32_t *depths, int32_t *n_depths)
{
    if (!ring_depth || !depths || !n_depths) return fail(SZG_E_INVALID, "null argument");
    if (kp < 0 || n_queries < 1 || n_queries > szg::kMaxSweepsPerLaunch) return fail(SZG_E_INVALID, "kp or n_queries out of range");
    if (const int rc = hook_options(nullptr, &scan_group, nullptr, nullptr, nullptr)) return rc;
    if (const int rc = hook_option(&Options::scan_group_ring, scan_group_ring)) return rc;
    PlanHook h;
    if (const int rc = h.rows(dim, quant_bits, 1, kp, false, 0)) return rc;
    h.in.group = scan_group;
    h.in.group_ring = scan_group_ring;
    h.walk(n_queries, szg::kMaxSweepsPerLaunch);
    *ring_depth = h.first.ring_depth;
    depths[0] = szg::kGroupRingBase;
    depths[1] = szg::kGroupRingAlt;
    *n_depths = szg::kGroupRingAlt != szg::kGroupRingBase ? 2 : 1;
    return SZG_OK;
}

}  // extern "C"
