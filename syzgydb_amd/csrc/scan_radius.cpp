// scan_radius.cpp -- radius search, Search{Precision:"exact", Radius > 0} (K is ignored: collection.go:598-605).
//
// A radius search is a COLLECT sweep: every row whose scan key is at or below a threshold derived from the radius
// (plus the key's error bound) is appended to the query's buffer, the hits are re-ranked in float64 and the
// reference's exact predicate `distance <= Radius` (:598) decides.  The sweeps of a batch are walked query-major by
// ONE launch (per-sweep threshold, buffer and counter in ScanArgs), the re-rank reads the hit counters on the
// device, and up to three batches are in flight per shard -- no launch gap and no host round trip between the sweeps
// of a batch, which is what a single query per launch per caller used to cost (5.7 of 6.9 TB/s on cfg5's shard).
#include "scan_internal.h"

namespace szgi {

// key threshold that surely contains every row with distance <= radius
float radius_key_threshold(const szg_index *ix, double radius, const QMeta &meta)
{
    if (ix->metric == SZG_COSINE) {
        if (radius >= 1.0 || meta.m1 == 0) return 3.0e38f;  // acos(c)/pi <= 1 always; zero query -> all 1.0
        const double t = -std::cos(M_PI * radius) + 2.0 * key_eps(ix, 1.0, meta) + 1e-12;
        return std::nextafter((float)t, INFINITY);
    }
    const double scale = ix->bits <= 16 ? (double)((1u << ix->bits) - 1u) : 1.0;
    const double kk = (radius * scale) * (radius * scale);
    const double t = kk * (1.0 + 1e-12) + 2.0 * key_eps(ix, kk, meta);
    // (an infinite radius with a zero query makes t = inf + 0 * inf = NaN: everything, as for any t beyond the floats)
    return !(t < 3.0e38) ? 3.0e38f : std::nextafter((float)t, INFINITY);
}

namespace {

constexpr size_t kRadiusCapMin = 1024;      // entries per sweep a batch's buffers start with
constexpr size_t kRadiusCapMax = 1u << 20;  // beyond this a query goes through run_collect on its own
constexpr size_t kRadiusBlockCopyBytes = 2u << 20;  // a batch's re-ranked hits travel as one block up to this size

// consider()'s radius branch (collection.go:598-605) over the candidates in visit order -- every record with
// distance <= Radius is pushed onto the max-heap -- then the pop loop (:694-697).  Popping a heap of pairwise
// distinct priorities yields them in descending order whatever the push order was, so the result is simply the hits
// sorted by distance; only when two hits share a distance (or one is NaN, which `<=` never admits anyway) does the
// order inside the tie depend on the heap's history, and only then is the heap replayed (three times the work).
void radius_assemble(std::vector<HeapItem> &cs, bool presorted, std::vector<HeapItem> *out)
{   // cs: the hits (distance <= radius already applied); presorted: already ascending by distance (the device's sort)
    const size_t n = cs.size();
    if (!presorted)
        std::sort(cs.begin(), cs.end(), [](const HeapItem &x, const HeapItem &y) { return x.priority < y.priority; });
    bool tie = false;
    for (size_t i = 1; i < n && !tie; i++) tie = cs[i].priority == cs[i - 1].priority;
    if (!tie) {
        out->swap(cs);
        return;
    }
    std::sort(cs.begin(), cs.end(), [](const HeapItem &x, const HeapItem &y) { return x.row < y.row; });
    GoHeap h;
    h.a.reserve(n);
    for (const HeapItem &c : cs) h.push(c);
    h.drain(out);
}

struct RadiusBatch : Batch {
    std::vector<float> thr;        // key threshold per query (of the sweep that runs: shared or one per query)
    std::vector<float> thr_single; // ... of the single-query collect sweep (a query that overflows is swept again on its own)
    std::vector<size_t> cap;       // per shard: entries per sweep of this batch's buffers
    std::vector<uint8_t> copied;   // per shard: the block of re-ranked hits was copied back at enqueue time
    std::vector<QMeta> meta;       // certificate trace only: each query's constants with the flags of the sweep that runs
};

struct RadiusCall {
    szg_index *ix;
    const double *queries;
    int n_queries;
    const double *radii;
    QueryMasks mask_of;
    std::vector<std::vector<HeapItem>> *results;
    size_t n_sh = 0;
    bool tracing = false;  // the handle's certificate trace is on

    RadiusBatch plan(int q0);
    int stage(RadiusBatch &t);
    int enqueue_shard(RadiusBatch &t, size_t s);
    int finish(RadiusBatch &t);
};

RadiusBatch RadiusCall::plan(int q0)
{
    RadiusBatch t;
    const int left = n_queries - q0;
    const int qpl = std::max(1, std::min(ix->queries_per_launch, szg::kMaxSweepsPerLaunch));
    // two or more queries left: they share one sweep of the corpus (up to 96 per pass), as top-k batches do
    const int nb = ix->radius_mq && left >= 2 ? mq_blocks(ix, left, true) : 0;
    // a small first batch and a small last one, as top-k's; only the smallest calls are ONE batch here: a radius
    // query's result assembly -- hundreds of hits to sort -- takes the host ~15 us, which a longer call hides behind
    // the next batch's sweeps
    const int edge = std::min(qpl, kFirstBatch);
    plan_batch(ix, n_queries, q0, nb, BatchRules{qpl, edge, edge, false, true}, &t);
    t.cap.assign(n_sh, 0);
    t.copied.assign(n_sh, 0);
    t.thr.assign(t.nq, 0.0f);
    t.thr_single.assign(t.nq, 0.0f);
    return t;
}

int RadiusCall::enqueue_shard(RadiusBatch &t, size_t s)
{
    Shard *sh = ix->shards[s];
    Ctx *c = t.ctx[s];
    HIPCHK(hipSetDevice(sh->device));
    // buffers: t.nq sweeps x cap entries; cap follows the largest hit count this context has seen
    size_t cap = std::max(kRadiusCapMin, c->radius_cap);
    // (a shared sweep's batch is up to 96 queries: keep its buffers within 8M entries; a query with more hits than
    // its share is swept again on its own)
    if (t.nb > 0) cap = std::min(cap, std::max(kRadiusCapMin, ((size_t)8 << 20) / (size_t)t.nq));
    t.cap[s] = cap;
    int rc = c->d_collect.ensure(cap * (size_t)t.nq);
    if (rc) return rc;
    rc = c->d_out.ensure(cap * (size_t)t.nq);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_count, 0, sizeof(uint32_t) * (size_t)t.nq * szg::kCandCountStride, c->pass.work));
    HIPCHK(hipEventRecord(c->ev_up, c->pass.work));  // the sweeps must see the queries, the masks and the zeroed counters
    if (t.nb > 0) {  // one shared sweep for the whole batch
        rc = enqueue_collect_mq(ix, sh, c, t.nq, t.nb, t.any_mask, t.thr.data(), cap);
        if (rc) return rc;
    }
    const int qpl = std::max(1, std::min(ix->queries_per_launch, szg::kMaxSweepsPerLaunch));
    std::vector<szg::ScanArgs> a(t.nb > 0 ? 0 : (t.nq + qpl - 1) / qpl);
    for (int j0 = 0; j0 < t.nq && t.nb == 0; j0 += qpl) {  // launches of <= 16 sweeps, back to back
        szg::ScanArgs &x = a[j0 / qpl];
        const int m = std::min(qpl, t.nq - j0);
        fill_scan_args(ix, sh, c, t.any_mask, j0, m, &x);
        x.collect = 1;
        for (int j = 0; j < m; j++) x.thr_ukeys[j] = szg::ordered_key(t.thr[j0 + j]);
        x.collect_buf = c->d_collect + (size_t)j0 * cap;
        x.collect_cap = (uint32_t)cap;
        x.collect_count = c->d_count + (size_t)j0 * szg::kCandCountStride;
        if ((t.any_mask || sh->has_dead) && ix->mask_dense) {  // most rows pass: read every row, masks at the row finish
            double lowest = 1.0;
            for (int j = 0; j < m; j++) lowest = std::min(lowest, mask_pass_rate(sh, c, t.any_mask, j0 + j));
            x.mask_dense = lowest >= 0.5 ? 1 : 0;
        }
    }
    if (t.nb == 0) {
        rc = launch_scans_chained(ix, sh, c, a, scan_geometry(ix, sh, 0));
        if (rc) return rc;
    }
    // float64 distances of the hits: the counts stay on the device
    HIPCHK(szg::launch_rerank(ix->bits, ix->metric, sh->rows, ix->layout, ix->dim, c->d_q64, c->d_collect, c->d_count,
                              (uint32_t)cap, t.nq, c->d_out, c->pass.work, szg::kCandCountStride));
    // ... and each query's hits sorted by distance there too (lists of up to kSortHitsMax: the host only filters)
    HIPCHK(szg::launch_sort_hits(c->d_out, c->d_count, szg::kCandCountStride, (uint32_t)cap, t.nq, c->pass.work));
    HIPCHK(hipMemcpyAsync(c->h_count, c->d_count, sizeof(uint32_t) * (size_t)t.nq * szg::kCandCountStride, hipMemcpyDeviceToHost,
                          c->pass.work));
    // the re-ranked hits: while the batch's buffers are small (the usual hundreds of hits per query) the whole block
    // follows in ONE copy right here -- finish() then needs a single wait; larger ones are copied hit list by hit
    // list once the counts are known
    // (a shared sweep's batch of up to 96 queries: a copy call per hit list costs more than 64 KiB of transfer each)
    t.copied[s] = cap * (size_t)t.nq * sizeof(szg::RerankOut) <= std::max(kRadiusBlockCopyBytes, (size_t)t.nq * (64u << 10));
    if (t.copied[s]) {
        rc = c->h_out.ensure(cap * (size_t)t.nq);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, cap * (size_t)t.nq * sizeof(szg::RerankOut), hipMemcpyDeviceToHost,
                              c->pass.work));
    }
    return SZG_OK;
}

int RadiusCall::stage(RadiusBatch &t)
{
    const double *q = queries + (size_t)t.first * ix->dim;
    const std::vector<const uint64_t *> m = t.masks(mask_of);
    const std::vector<const szg_mask *> handles = t.handles(mask_of);
    const double t0 = now_us();
    const bool int_planes = t.nb > 0 && mq_uses_i8(ix, true);
    if (tracing) t.meta.assign(t.nq, QMeta{});
    int rc = stage_query_forms(ix, t, q, int_planes, [&](int j, QMeta &meta) {
        const double radius = radii[t.first + j];
        QMeta m2 = meta;  // the shared sweep's arithmetic has its own error bound
        if (t.nb == 0) {
            t.thr_single[j] = t.thr[j] = radius_key_threshold(ix, radius, meta);
        } else {
            m2.mq = !int_planes;
            m2.mq_bf16 = mq_uses_bf16(ix, true);
            t.thr[j] = radius_key_threshold(ix, radius, m2);
        }
        if (tracing) t.meta[j] = m2;
    });
    if (rc) return rc;
    const double t1 = now_us();
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        if (!t.ctx[s]) continue;
        rc = enqueue_queries(ix, ix->shards[s], t.ctx[s], q, t.nq, t.any_mask ? m.data() : nullptr, t.nb == 0,
                             handles.empty() ? nullptr : handles.data(), s);
        if (rc == SZG_OK) rc = enqueue_shard(t, s);
    }
    note_stage_times(ix, t0, t1);
    return rc;
}

int RadiusCall::finish(RadiusBatch &t)
{
    if (t.failed) {
        t.drain();
        return SZG_OK;
    }
    int rc = SZG_OK;
    std::vector<std::vector<HeapItem>> cands(t.nq);  // the hits proper: `distance <= Radius` (collection.go:598) applied here
    std::vector<uint8_t> redo(t.nq, 0);  // more hits than the batch's buffers hold: the query is swept again on its own
    std::vector<uint8_t> presorted(t.nq, 1);  // the query's hits come from ONE shard's device-sorted list
    std::vector<uint8_t> lists(t.nq, 0);
    std::vector<std::vector<szg_cert_entry>> traced(tracing ? t.nq : 0);  // every collected hit, before the predicate
    std::vector<uint8_t> untraced(tracing ? t.nq : 0, 0);  // the query's record will not fit the trace: nothing is gathered
    double t_wait = 0;
    const double t0 = now_us();
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        Ctx *c = t.ctx[s];
        if (!c) continue;
        Shard *sh = ix->shards[s];
        const double tw = now_us();
        hipError_t e = hipSetDevice(sh->device);
        if (e == hipSuccess) e = hipStreamSynchronize(c->pass.work);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
        rc = finish_timing(ix, c);
        if (rc) break;
        const size_t cap = t.cap[s];
        size_t most = 0;
        std::vector<size_t> cnt(t.nq, 0), off(t.nq + 1, 0);
        for (int j = 0; j < t.nq; j++) {
            const size_t n = c->h_count[(size_t)j * szg::kCandCountStride];
            most = std::max(most, n);
            if (n > cap) redo[j] = 1;
            cnt[j] = n > cap ? 0 : n;
            off[j + 1] = off[j] + cnt[j];
        }
        // the next batch on this context starts with room for what this one saw (and shrinks again slowly)
        size_t want = kRadiusCapMin;
        while (want < most + most / 4 && want < kRadiusCapMax) want <<= 1;
        c->radius_cap = std::max(want, c->radius_cap - c->radius_cap / 8);
        if (t.copied[s]) {  // hits of sweep j at h_out + j * cap
            for (int j = 0; j < t.nq; j++) off[j] = (size_t)j * cap;
        } else if (off[t.nq]) {
            // exact-size copies of each sweep's re-ranked hits, back to back in the pinned buffer
            rc = c->h_out.ensure(off[t.nq]);
            if (rc) break;
            for (int j = 0; j < t.nq; j++) {
                if (!cnt[j]) continue;
                e = hipMemcpyAsync(c->h_out + off[j], c->d_out + (size_t)j * cap, cnt[j] * sizeof(szg::RerankOut),
                                   hipMemcpyDeviceToHost, c->pass.work);
                if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipMemcpyAsync(radius hits)", e);
            }
            e = hipStreamSynchronize(c->pass.work);
            if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
        }
        t_wait += now_us() - tw;
        for (int j = 0; j < t.nq; j++) {
            if (redo[j]) continue;
            cands[j].reserve(cands[j].size() + cnt[j]);
            if (cnt[j]) {
                if (cnt[j] > (size_t)szg::kSortHitsMax || ++lists[j] > 1) presorted[j] = 0;
            }
            const double rad = radii[t.first + j];
            if (tracing && !untraced[j] && !cert_room(ix, traced[j].size() + cnt[j])) {
                untraced[j] = 1;
                std::vector<szg_cert_entry>().swap(traced[j]);
            }
            const bool keep = tracing && !untraced[j];
            for (size_t i = off[j]; i < off[j] + cnt[j]; i++) {
                const szg::RerankOut &r = c->h_out[i];
                if (r.dist <= rad) cands[j].push_back(HeapItem{sh->first + r.row, r.dist});
                if (keep) {
                    const float key = szg::key_from_ordered(r.ukey);
                    traced[j].push_back(szg_cert_entry{sh->first + r.row, r.dist, (double)key + key_eps(ix, key, t.meta[j]), key, 0u});
                }
            }
        }
    }
    for (int j = 0; j < t.nq && rc == SZG_OK; j++) {
        if (redo[j]) {
            cands[j].clear();
            std::vector<Cand> all;
            const double tw = now_us();
            if (t.nb > 0) {  // the single-query form of this query, now that it is needed
                QMeta m;
                rc = stage_single_form(ix, t, queries + (size_t)(t.first + j) * ix->dim, j, &m);
                t.thr_single[j] = radius_key_threshold(ix, radii[t.first + j], m);
            }
            for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
                if (!t.ctx[s]) continue;
                const CertTag tag{t.first + j, SZG_CERT_RADIUS_SINGLE};
                rc = run_collect(ix, ix->shards[s], t.ctx[s], j, t.thr_single[j], t.any_mask, &all, tracing ? &tag : nullptr);
            }
            t_wait += now_us() - tw;
            if (rc) break;
            const double rad = radii[t.first + j];
            for (const Cand &c : all)
                if (c.dist <= rad) cands[j].push_back(HeapItem{c.row, c.dist});
            presorted[j] = 0;
        } else if (tracing && !untraced[j]) {
            szg_cert_record rec = cert_record(t.first + j, t.nb > 0 ? SZG_CERT_RADIUS_SHARED : SZG_CERT_RADIUS_SINGLE);
            rec.sweep = t.nb == 0 ? 0 : (t.meta[j].mq_bf16 ? 2 : 1);
            for (const Shard *sh : ix->shards) rec.row_hi = std::max<uint64_t>(rec.row_hi, sh->first + sh->n_rows);
            rec.thr = (double)t.thr[j];
            rec.eps = key_eps(ix, t.thr[j], t.meta[j]);
            cert_emit(ix, rec, traced[j]);
        }
        radius_assemble(cands[j], presorted[j] != 0, &(*results)[t.first + j]);
    }
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->stats.host_finish_us += now_us() - t0 - t_wait;
        if (rc == SZG_OK) ix->stats.queries += t.nq;
    }
    t.release();
    return rc;
}

}  // namespace

int search_radius_impl(szg_index *ix, const double *queries, int n_queries, const double *radii,
                       const uint64_t *const *masks, std::vector<std::vector<HeapItem>> *results,
                       const szg_mask *const *handles)
{
    RadiusCall call{ix, queries, n_queries, radii, QueryMasks(ix, nullptr, masks, handles), results, ix->shards.size(),
                    cert_tracing(ix)};
    results->assign(n_queries, {});
    return run_batches<RadiusBatch>(call);
}

}  // namespace szgi
