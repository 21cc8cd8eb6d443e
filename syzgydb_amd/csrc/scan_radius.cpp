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
    const int *trace_index = nullptr;  // the queries' indexes in the call this one was made for (null: their own)

    int traced_as(int qi) const { return trace_index ? trace_index[qi] : qi; }
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
                const CertTag tag{traced_as(t.first + j), SZG_CERT_RADIUS_SINGLE};
                rc = run_collect(ix, ix->shards[s], t.ctx[s], j, t.thr_single[j], t.any_mask, &all, tracing ? &tag : nullptr);
            }
            t_wait += now_us() - tw;
            if (rc) break;
            const double rad = radii[t.first + j];
            for (const Cand &c : all)
                if (c.dist <= rad) cands[j].push_back(HeapItem{c.row, c.dist});
            presorted[j] = 0;
        } else if (tracing && !untraced[j]) {
            szg_cert_record rec = cert_record(traced_as(t.first + j), t.nb > 0 ? SZG_CERT_RADIUS_SHARED : SZG_CERT_RADIUS_SINGLE);
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

// ---- radius searches through the 8-bit sketch (option sketch_radius) --------------------------
//
// A radius search needs completeness only, and the triangle inequality of the reference's distance gives it by
// construction.  With A = max over the rows of d(row, its sketch) (sk_max_ang) and s the sketch of row x:
//
//     d(q, x) <= R   =>   d(q, s) <= d(q, x) + d(x, s) <= R + A <= D = R (1 + 1e-9) + slack
//                    =>   the real-number sketch key of the row is at or below the key D implies (the key is monotone
//                         in the distance), which is at or below thr - eps by radius_key_threshold's construction on
//                         the SKETCH handle (key_eps there is the two-plane integer bound)
//                    =>   the sweep's float32 key is at or below thr: the row is collected.
//
// So a collect sweep of the sketch at the widened radius finds every hit; the float64 re-rank on the float32 rows and
// the host's `dist <= radius` apply the reference's own predicate.  No answer-dependent certificate, no escalation, no
// drop bound.  The batch is RadiusBatch-shaped, on the sketch index's contexts and in the sketch pre-pass's batch plan
// (SketchCall::plan); launches of three queries or more without masks or tombstones share each row read on the matrix
// cores (kernels_scan_mx.hip, the collect form), the others keep scan_kernel's collect form: a quarter of the bytes
// either way.  Rows without a usable sketch (sk_exc) are staged as the head of each query's collect buffer, the
// counter starting at their count.  A zero query under cosine, a non-finite query or radius, D >= 1 under cosine and a
// query whose candidates overflow the batch's buffers are handed to search_radius_impl, all of a call as ONE call.

constexpr uint32_t kNoKeyUkey = 0xFFFFFFFFu;  // "ordered key" of the entries staged ahead of the sweep: a sweep's keys
                                              // are clamped to 3e38, so none of them orders that high

struct SketchRadiusBatch : Batch {
    std::vector<float> thr;       // the sketch sweep's key threshold per query
    std::vector<double> D;        // the sketch-distance radius per query (real units)
    std::vector<uint8_t> handed;  // handed over before any sweep (its slot collects nothing)
    std::vector<QMeta> meta;      // the queries' constants on the sketch index
    std::vector<size_t> cap;      // per shard: entries per query of this batch's buffers
    std::vector<uint8_t> copied;  // per shard: the block of re-ranked hits was copied back at enqueue time
};

// does the matrix sweep's two-block collect form serve an unmasked launch of 32 queries of sketch index sk on shard sh?
bool collect_wide_serves(const szg_index *sk, const Shard *sh)
{
    if (sk->sketch_wide == 1 || sh->has_dead) return false;
    const LaunchGeom g = scan_geometry(sk, sh, 0);
    return szg::scan_variant(sk->bits, sk->map, sk->layout.tiled != 0, 0, true, false, sk->ring, !sk->shape_kernels,
                             sk->scan_group, szg::kMatrixWideQueries, g.block, scan_planes(sk), sk->scan_group_ring,
                             sk->sketch_matrix, true, sk->sketch_select, sk->sketch_wide)
               .wide != 0;
}

struct SketchRadiusCall {
    szg_index *ix;  // the float32 handle (rows, masks, results, trace)
    szg_index *sk;  // its sketch index (contexts, sweeps)
    const double *queries;
    int n_queries;
    const double *radii;
    QueryMasks mask_of;
    std::vector<std::vector<HeapItem>> *results;
    std::vector<int> redo;  // queries handed over to search_radius_impl, ascending
    size_t n_sh = 0;
    bool tracing = false;
    double gs = 0.0, slack = 0.0;
    int wide = 0;  // as SketchCall::wide
    std::vector<double> q_sk;

    int run();
    SketchRadiusBatch plan(int q0);
    int stage(SketchRadiusBatch &t);
    int enqueue_shard(SketchRadiusBatch &t, size_t s, const std::vector<const uint64_t *> &masks);
    int finish(SketchRadiusBatch &t);
};

int SketchRadiusCall::run()
{
    n_sh = ix->shards.size();
    tracing = cert_tracing(ix);
    gs = ix->sk_gscale;
    // slack exactly as SketchCall::run forms it: max_ang (1 + 1e-9), plus the build kernel's angle rounding under cosine
    const double ang_round = std::max(1e-7, 2.0 * std::sqrt((ix->dim + 8) * 0x1p-52) / M_PI);
    slack = ix->sk_max_ang * (1.0 + 1e-9) + (gs > 0.0 ? 0.0 : ang_round);
    sk->timing = ix->timing;
    wide = 0;
    if (sk->sketch_wide != 1 && n_queries > szg::kMatrixQueries) {
        bool serves = true, any = false;
        for (size_t s = 0; s < n_sh && serves; s++) {
            if (sk->shards[s]->n_rows == 0) continue;
            any = true;
            serves = collect_wide_serves(sk, sk->shards[s]);
        }
        if (serves && any) {
            if (sk->sketch_wide == 2) wide = 2;
            else if (n_queries >= kWideCallMin && ix->query_batch == 16 && sk->queries_per_launch == 16) wide = 1;
        }
    }
    return run_batches<SketchRadiusBatch>(*this);
}

SketchRadiusBatch SketchRadiusCall::plan(int q0)
{
    SketchRadiusBatch t;
    const int batch = std::max(1, std::min(ix->query_batch, kMaxBatch));
    if (wide == 2)
        plan_batch(sk, n_queries, q0, 0, BatchRules{szg::kMatrixWideQueries, n_queries, szg::kMatrixWideQueries, false, false}, &t);
    else if (wide)
        plan_batch(sk, n_queries, q0, 0, BatchRules{szg::kMatrixWideQueries, kFirstBatch, std::min(kShortCall, kMaxBatch), true, false}, &t);
    else
        plan_batch(sk, n_queries, q0, 0, BatchRules{batch, kFirstBatch, std::min(kShortCall, kMaxBatch), true, false}, &t);
    t.thr.assign(t.nq, 0.0f);
    t.D.assign(t.nq, 0.0);
    t.handed.assign(t.nq, 0);
    t.meta.assign(t.nq, QMeta{});
    t.cap.assign(n_sh, 0);
    t.copied.assign(n_sh, 0);
    return t;
}

int SketchRadiusCall::stage(SketchRadiusBatch &t)
{
    const double t0 = now_us();
    const int dim = ix->dim;
    const double *q = queries + (size_t)t.first * dim;
    const std::vector<const uint64_t *> masks = t.masks(mask_of);
    const std::vector<const szg_mask *> handles = t.handles(mask_of);
    // the query forms of the sketch: q / gscale under Euclid; a query that is handed over sweeps as zeros and collects nothing
    q_sk.assign((size_t)t.nq * dim, 0.0);
    for (int j = 0; j < t.nq; j++) {
        const double *qj = q + (size_t)j * dim;
        const double R = radii[t.first + j];
        double m1 = 0.0;
        bool finite = std::isfinite(R);
        for (int i = 0; i < dim; i++) {
            finite = finite && std::isfinite(qj[i]);
            m1 += qj[i] * qj[i];
        }
        const double D = R * (1.0 + 1e-9) + slack;
        t.D[j] = D;
        t.handed[j] = !finite || !std::isfinite(m1) || !std::isfinite(D) || (gs <= 0.0 && (m1 == 0.0 || D >= 1.0));
        if (t.handed[j]) continue;
        for (int i = 0; i < dim; i++) q_sk[(size_t)j * dim + i] = gs > 0.0 ? qj[i] / gs : qj[i];
    }
    int rc = stage_query_forms(sk, t, q_sk.data(), false, [&](int j, QMeta &meta) {
        t.meta[j] = meta;
        // (radius_key_threshold on the sketch handle, with the sketch's constants: key_eps is the two-plane integer bound;
        // a slot that is handed over: below every key)
        t.thr[j] = t.handed[j] ? -FLT_MAX : radius_key_threshold(sk, gs > 0.0 ? t.D[j] / gs : t.D[j], meta);
    });
    if (rc) return rc;
    const double t1 = now_us();
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        if (!t.ctx[s]) continue;
        // (the float64 queries unscaled: the re-rank is on the float32 rows; a resident mask's shard words serve the sketch
        // shard too)
        rc = enqueue_queries(sk, sk->shards[s], t.ctx[s], q, t.nq, t.any_mask ? masks.data() : nullptr, true,
                             handles.empty() ? nullptr : handles.data(), s);
        if (rc == SZG_OK) rc = enqueue_shard(t, s, masks);
    }
    note_stage_times(ix, t0, t1);
    return rc;
}

int SketchRadiusCall::enqueue_shard(SketchRadiusBatch &t, size_t s, const std::vector<const uint64_t *> &masks)
{
    Shard *h = sk->shards[s];
    const Shard *a = ix->shards[s];
    Ctx *c = t.ctx[s];
    HIPCHK(hipSetDevice(h->device));
    const uint32_t stride = szg::kCandCountStride;
    // the shard's eligible rows without a usable sketch, per query: the head of its collect buffer
    std::vector<std::vector<uint64_t>> head(t.nq);
    size_t head_max = 0;
    for (int j = 0; j < t.nq; j++) {
        if (t.handed[j]) continue;
        const uint64_t *m = masks[j];
        for (uint64_t r : ix->sk_exc) {
            if (r < a->first || r >= a->first + a->n_rows) continue;
            const uint64_t l = r - a->first;
            if (((a->live_host[l >> 6] >> (l & 63)) & 1) && (!m || ((m[r >> 6] >> (r & 63)) & 1)))
                head[j].push_back(((uint64_t)kNoKeyUkey << 32) | l);
        }
        head_max = std::max(head_max, head[j].size());
    }
    size_t cap = std::max(kRadiusCapMin, c->radius_cap);
    cap = std::min(cap, std::max(kRadiusCapMin, ((size_t)8 << 20) / (size_t)t.nq));  // (a batch's buffers: 8M entries at most)
    while (cap < head_max + kRadiusCapMin) cap <<= 1;
    t.cap[s] = cap;
    int rc = c->d_collect.ensure(cap * (size_t)t.nq);
    if (rc == SZG_OK) rc = c->d_out.ensure(cap * (size_t)t.nq);
    if (rc == SZG_OK && head_max) rc = c->h_sent.ensure(head_max * (size_t)t.nq);
    if (rc) return rc;
    // the counters start at the staged rows' counts
    memset(c->h_count, 0, sizeof(uint32_t) * (size_t)t.nq * stride);
    for (int j = 0; j < t.nq; j++) {
        c->h_count[(size_t)j * stride] = (uint32_t)head[j].size();
        if (head[j].empty()) continue;
        uint64_t *src = c->h_sent + (size_t)j * head_max;
        memcpy(src, head[j].data(), head[j].size() * sizeof(uint64_t));
        HIPCHK(hipMemcpyAsync(c->d_collect + (size_t)j * cap, src, head[j].size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                              c->pass.work));
    }
    HIPCHK(hipMemcpyAsync(c->d_count, c->h_count, sizeof(uint32_t) * (size_t)t.nq * stride, hipMemcpyHostToDevice, c->pass.work));
    HIPCHK(hipEventRecord(c->ev_up, c->pass.work));  // the sweeps must see the queries, the masks, the heads and the counters

    const bool masked = t.any_mask || h->has_dead;
    const LaunchGeom g = scan_geometry(sk, h, 0);
    // launches that may share their row reads on the matrix cores take the rows' norms from the resident array
    const float *norms = nullptr;
    if (!masked && sk->scan_group == 0 && sk->sketch_matrix != 1 &&
        (wide || t.nq >= szg::kMatrixMinQueries || sk->sketch_matrix == 2)) {
        int nrc = SZG_OK;
        norms = scan_row_norms(sk, h, &nrc);
        if (nrc) return nrc;
    }
    const int qpl16 = std::max(1, std::min(sk->queries_per_launch, szg::kMaxSweepsPerLaunch));
    const int qpl = wide && norms && t.nq > szg::kMatrixQueries && collect_wide_serves(sk, h) ? szg::kMatrixWideQueries : qpl16;
    t.copied[s] = cap * (size_t)t.nq * sizeof(szg::RerankOut) <= std::max(kRadiusBlockCopyBytes, (size_t)t.nq * (64u << 10));
    if (t.copied[s]) {
        rc = c->h_out.ensure(cap * (size_t)t.nq);
        if (rc) return rc;
    }
    // one part -- or, for a short call (Pass::early_n), two, as enqueue_topk: the first queries' re-rank, sort and
    // copy-back leave the scan stream for the context's own and run beside the call's last sweeps
    const int early = c->pass.early_n > 0 && c->pass.early_n < t.nq ? c->pass.early_n : 0;
    for (int part = early ? 1 : 0; part >= 0; part--) {
        const int q0 = part ? 0 : early, q1 = part ? early : t.nq, nqp = q1 - q0;
        hipStream_t tl = part ? c->stream : c->pass.work;
        std::vector<szg::ScanArgs> args((nqp + qpl - 1) / qpl);
        for (int j0 = q0; j0 < q1; j0 += qpl) {
            szg::ScanArgs &x = args[(j0 - q0) / qpl];
            const int m = std::min(qpl, q1 - j0);
            fill_scan_args(sk, h, c, t.any_mask, j0, m, &x);
            x.collect = 1;
            for (int j = 0; j < m; j++) szg::scan_thr_ukey(x, j) = szg::ordered_key(t.thr[j0 + j]);
            x.collect_buf = c->d_collect + (size_t)j0 * cap;
            x.collect_cap = (uint32_t)cap;
            x.collect_count = c->d_count + (size_t)j0 * stride;
            if (masked && sk->mask_dense) {
                double lowest = 1.0;
                for (int j = 0; j < m; j++) lowest = std::min(lowest, mask_pass_rate(h, c, t.any_mask, j0 + j));
                x.mask_dense = lowest >= 0.5 ? 1 : 0;
            }
            // (a call with wide batches: its launches take the matrix sweep whatever their count, as top-k's)
            if (wide && x.matrix == 0) x.matrix = 2;
            if (norms && szg::scan_wants_norms(sk->bits, x, g.block)) x.row_norm = norms;
        }
        rc = launch_scans_chained(sk, h, c, args, g, tl, part);
        if (rc) return rc;
        // float64 distances on the FLOAT32 shard's rows, the counts staying on the device; then each query's hits sorted
        HIPCHK(szg::launch_rerank(ix->bits, ix->metric, a->rows, ix->layout, ix->dim, c->d_q64 + (size_t)q0 * ix->dim,
                                  c->d_collect + (size_t)q0 * cap, c->d_count + (size_t)q0 * stride, (uint32_t)cap, nqp,
                                  c->d_out + (size_t)q0 * cap, tl, stride));
        HIPCHK(szg::launch_sort_hits(c->d_out + (size_t)q0 * cap, c->d_count + (size_t)q0 * stride, stride, (uint32_t)cap, nqp, tl));
        HIPCHK(hipMemcpyAsync(c->h_count + (size_t)q0 * stride, c->d_count + (size_t)q0 * stride,
                              sizeof(uint32_t) * (size_t)nqp * stride, hipMemcpyDeviceToHost, tl));
        if (t.copied[s])
            HIPCHK(hipMemcpyAsync(c->h_out + (size_t)q0 * cap, c->d_out + (size_t)q0 * cap,
                                  cap * (size_t)nqp * sizeof(szg::RerankOut), hipMemcpyDeviceToHost, tl));
    }
    return SZG_OK;
}

int SketchRadiusCall::finish(SketchRadiusBatch &t)
{
    if (t.failed) {
        t.drain();
        return SZG_OK;
    }
    int rc = SZG_OK;
    std::vector<std::vector<HeapItem>> cands(t.nq);
    std::vector<uint8_t> over(t.nq, 0);       // more candidates than the batch's buffers hold: handed over
    std::vector<uint8_t> presorted(t.nq, 1);  // the query's hits come from ONE shard's device-sorted list
    std::vector<uint8_t> lists(t.nq, 0);
    std::vector<std::vector<szg_cert_entry>> traced(tracing ? t.nq : 0);
    std::vector<uint8_t> untraced(tracing ? t.nq : 0, 0);
    double t_wait = 0;
    const double t0 = now_us();
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        Ctx *c = t.ctx[s];
        if (!c) continue;
        const Shard *a = ix->shards[s];
        const double tw = now_us();
        hipError_t e = hipSetDevice(a->device);
        if (e == hipSuccess) e = hipStreamSynchronize(c->pass.work);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (a short call's early part)
        if (e != hipSuccess) {
            rc = fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
            break;
        }
        rc = finish_timing(sk, c);
        if (rc) break;
        const size_t cap = t.cap[s];
        size_t most = 0;
        std::vector<size_t> cnt(t.nq, 0), off(t.nq + 1, 0);
        for (int j = 0; j < t.nq; j++) {
            const size_t n = c->h_count[(size_t)j * szg::kCandCountStride];
            most = std::max(most, n);
            if (n > cap) over[j] = 1;
            cnt[j] = n > cap ? 0 : n;
            off[j + 1] = off[j] + cnt[j];
        }
        // the next batch on this context starts with room for what this one saw (and shrinks again slowly)
        size_t want = kRadiusCapMin;
        while (want < most + most / 4 && want < kRadiusCapMax) want <<= 1;
        c->radius_cap = std::max(want, c->radius_cap - c->radius_cap / 8);
        if (t.copied[s]) {
            for (int j = 0; j < t.nq; j++) off[j] = (size_t)j * cap;
        } else if (off[t.nq]) {
            rc = c->h_out.ensure(off[t.nq]);
            if (rc) break;
            for (int j = 0; j < t.nq && e == hipSuccess; j++)
                if (cnt[j])
                    e = hipMemcpyAsync(c->h_out + off[j], c->d_out + (size_t)j * cap, cnt[j] * sizeof(szg::RerankOut),
                                       hipMemcpyDeviceToHost, c->pass.work);
            if (e == hipSuccess) e = hipStreamSynchronize(c->pass.work);
            if (e != hipSuccess) {
                rc = fail(SZG_E_DEVICE, "hipMemcpyAsync(sketch radius hits)", e);
                break;
            }
        }
        t_wait += now_us() - tw;
        for (int j = 0; j < t.nq; j++) {
            if (over[j] || t.handed[j]) continue;
            cands[j].reserve(cands[j].size() + cnt[j]);
            if (cnt[j] && (cnt[j] > (size_t)szg::kSortHitsMax || ++lists[j] > 1)) presorted[j] = 0;
            const double rad = radii[t.first + j];
            if (tracing && !untraced[j] && !cert_room(ix, traced[j].size() + cnt[j])) {
                untraced[j] = 1;
                std::vector<szg_cert_entry>().swap(traced[j]);
            }
            const bool keep = tracing && !untraced[j];
            for (size_t i = off[j]; i < off[j] + cnt[j]; i++) {
                const szg::RerankOut &r = c->h_out[i];
                const uint64_t row = a->first + r.row;
                const bool no_key = r.ukey == kNoKeyUkey;
                // (the bytes that stand in a sketch shard for a row without a usable sketch mean nothing: should the
                // sweep collect such a row, the staged entry is the one that counts)
                if (!no_key && !ix->sk_exc.empty() && std::binary_search(ix->sk_exc.begin(), ix->sk_exc.end(), row)) continue;
                if (r.dist <= rad) cands[j].push_back(HeapItem{row, r.dist});  // (a NaN distance is never a hit)
                if (!keep) continue;
                if (no_key) {
                    traced[j].push_back(szg_cert_entry{row, r.dist, 0.0, 0.0f, SZG_CERT_ENTRY_NO_KEY});
                } else {
                    const float key = szg::key_from_ordered(r.ukey);
                    traced[j].push_back(szg_cert_entry{row, r.dist, (double)key + key_eps(sk, key, t.meta[j]), key, 0u});
                }
            }
        }
    }
    uint64_t settled = 0, fb = 0;
    for (int j = 0; j < t.nq && rc == SZG_OK; j++) {
        if (over[j] || t.handed[j]) {
            redo.push_back(t.first + j);
            fb++;
            continue;
        }
        settled++;
        if (tracing && !untraced[j]) {
            szg_cert_record rec = cert_record(t.first + j, SZG_CERT_SKETCH_RADIUS);
            rec.keys = SZG_CERT_KEYS_SINGLE;
            rec.sweep = 0;
            for (const Shard *sh : ix->shards) rec.row_hi = std::max<uint64_t>(rec.row_hi, sh->first + sh->n_rows);
            rec.thr = (double)t.thr[j];
            rec.eps = key_eps(sk, t.thr[j], t.meta[j]);
            rec.D = t.D[j];
            rec.slack = slack;
            cert_emit(ix, rec, traced[j]);
        }
        radius_assemble(cands[j], presorted[j] != 0, &(*results)[t.first + j]);
    }
    if (rc) t.drain();
    else t.release();
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->stats.host_finish_us += now_us() - t0 - t_wait;
    if (rc == SZG_OK) {
        ix->stats.queries += settled;
        ix->stats.sketch_radius_queries += settled;
        ix->stats.sketch_radius_fallbacks += fb;
    }
    return rc;
}

}  // namespace

int search_radius_any(szg_index *ix, const double *queries, int n_queries, const double *radii,
                      const uint64_t *const *masks, std::vector<std::vector<HeapItem>> *results,
                      const szg_mask *const *handles)
{
    // queries that would each take a sweep of their own (RadiusCall::plan gives them nb == 0); batches that share a
    // sweep keep it
    const bool own_sweeps = n_queries == 1 || !ix->radius_mq || mq_blocks(ix, n_queries, true) == 0;
    if (!ix->sketch_radius || !own_sweeps || n_queries < 1 || !sketch_applies_rows(ix))
        return search_radius_impl(ix, queries, n_queries, radii, masks, results, handles);
    int rc = sketch_sync_for_search(ix);
    if (rc) return rc;
    if (ix->sk_disabled || ix->sk_nomem) return search_radius_impl(ix, queries, n_queries, radii, masks, results, handles);
    results->assign(n_queries, {});
    SketchRadiusCall call{ix, ix->sketch, queries, n_queries, radii, QueryMasks(ix, nullptr, masks, handles), results};
    rc = call.run();
    if (rc && ix->sketch_on == 2) {
        // (a failure inside the pipeline, an allocation of a sketch context: the sketch index stays until the next load,
        // the whole call goes the full-precision way -- as search_topk_sketch)
        ix->sk_nomem = true;
        return search_radius_impl(ix, queries, n_queries, radii, masks, results, handles);
    }
    if (rc || call.redo.empty()) return rc;
    // the queries handed over: ONE call of the float32 path, with their masks and handles (no entry in the top-k auto
    // window, sk_hist: radius hand-overs say nothing about top-k certificates)
    const int m = (int)call.redo.size();
    std::vector<double> q2((size_t)m * ix->dim), r2(m);
    std::vector<const uint64_t *> m2(m);
    std::vector<const szg_mask *> h2(handles ? m : 0);
    bool any = false;
    for (int i = 0; i < m; i++) {
        memcpy(&q2[(size_t)i * ix->dim], queries + (size_t)call.redo[i] * ix->dim, sizeof(double) * ix->dim);
        r2[i] = radii[call.redo[i]];
        m2[i] = call.mask_of(call.redo[i]);
        if (handles) h2[i] = handles[call.redo[i]];
        any |= m2[i] != nullptr;
    }
    std::vector<std::vector<HeapItem>> hits2;
    rc = search_radius_impl(ix, q2.data(), m, r2.data(), !handles && any ? m2.data() : nullptr, &hits2,
                            handles && any ? h2.data() : nullptr, call.redo.data());
    if (rc) return rc;
    for (int i = 0; i < m; i++) (*results)[call.redo[i]].swap(hits2[i]);
    return SZG_OK;
}

int search_radius_impl(szg_index *ix, const double *queries, int n_queries, const double *radii,
                       const uint64_t *const *masks, std::vector<std::vector<HeapItem>> *results,
                       const szg_mask *const *handles, const int *trace_index)
{
    RadiusCall call{ix, queries, n_queries, radii, QueryMasks(ix, nullptr, masks, handles), results, ix->shards.size(),
                    cert_tracing(ix), trace_index};
    results->assign(n_queries, {});
    return run_batches<RadiusBatch>(call);
}

}  // namespace szgi
