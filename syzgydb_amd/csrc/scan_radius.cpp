// scan_radius.cpp -- radius search, Search{Precision:"exact", Radius > 0} (K is ignored: collection.go:598-605).
//
// A radius search is a COLLECT sweep: every row whose scan key is at or below a threshold derived from the radius
// (plus the key's error bound) is appended to the query's buffer, the hits are re-ranked in float64 and the
// reference's exact predicate `distance <= Radius` (:598) decides.  The sweeps of a batch are walked query-major by
// ONE launch (per-sweep threshold, buffer and counter in ScanArgs), the re-rank reads the hit counters on the
// device, and up to three batches are in flight per shard -- no launch gap and no host round trip between the sweeps
// of a batch, which is what a single query per launch per caller used to cost (5.7 of 6.9 TB/s on cfg5's shard).
// RadiusCall sweeps the handle's own rows, SketchRadiusCall (option sketch_radius) the 8-bit sketch of float32 rows: what
// a batch is on the device and how it is read back exists once, in the collect core; its arithmetic is collect_plan.h.
#include "collect_plan.h"
#include "sample_plan.h"
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

static_assert(sizeof(szg::RerankOut) == kCollectEntryBytes, "collect_plan.h sizes the hit buffers in entries of this size");

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

// ---- the collect core: one batch of collect sweeps on the device and back -----------------------------------------------
// Per shard a batch holds nq buffers of cap entries in d_collect (the sweeps append row and key), the same in d_out (the
// re-rank's float64 distances, sorted per query) and one counter per query in d_count.  The callers differ in which
// index is swept, how the counters start and which launches make the sweeps; everything else is here.

constexpr uint32_t kNoKeyUkey = 0xFFFFFFFFu;  // "ordered key" of the entries staged ahead of the sweep: a sweep's keys
                                              // are clamped to 3e38, so none of them orders that high

struct CollectBatch : Batch {
    std::vector<float> thr;       // key threshold per query, of the sweep that runs
    std::vector<size_t> cap;      // per shard: entries per query of this batch's buffers
    std::vector<uint8_t> copied;  // per shard: the block of re-ranked hits was copied back at enqueue time
    std::vector<QMeta> meta;      // each query's constants with the flags of the sweep that runs (float32 path: traced calls only)
    void size() { thr.assign(nq, 0.0f), cap.assign(ctx.size(), 0), copied.assign(ctx.size(), 0); }  // (once planned)
};

// the buffers of batch t on shard s: cap follows the largest hit count the context has seen (collect_cap has the rules)
// (floor: entries per query the caller's plan asks for from the first batch on -- the sample plan's; 0: none)
int collect_buffers(CollectBatch &t, size_t s, bool limited, size_t head_max, size_t floor = 0)
{
    Ctx *c = t.ctx[s];
    const size_t cap = t.cap[s] = collect_cap(std::max(c->radius_cap, floor), t.nq, limited, head_max);
    const size_t n = collect_block_entries(cap, t.nq);
    // (small buffers -- the usual hundreds of hits per query: the whole block follows the sweeps, finish() needs one wait)
    t.copied[s] = collect_block_copied(cap, t.nq);
    int rc = c->d_collect.ensure(n);
    if (rc == SZG_OK) rc = c->d_out.ensure(n);
    if (rc == SZG_OK && t.copied[s]) rc = c->h_out.ensure(n);
    return rc;
}

// collect launches of up to qpl sweeps for queries [q0, q1) of the batch, back to back on the shard's scan chain; `after`
// goes on once they are done.  wide: the call takes wide batches -- its launches take the matrix sweep whatever their
// count, as top-k's; norms: the shard's resident row norms for the launches that read them (null: none does)
int collect_sweeps(szg_index *ix, Shard *sh, Ctx *c, const CollectBatch &t, size_t cap, int q0, int q1, int qpl,
                   hipStream_t after, int part, bool wide = false, const float *norms = nullptr)
{
    const LaunchGeom g = scan_geometry(ix, sh, 0);
    std::vector<szg::ScanArgs> a((q1 - q0 + qpl - 1) / qpl);
    for (int j0 = q0; j0 < q1; j0 += qpl) {
        szg::ScanArgs &x = a[(j0 - q0) / qpl];
        fill_collect_args(ix, sh, c, t.any_mask, j0, std::min(qpl, q1 - j0), &t.thr[j0], c->d_collect + (size_t)j0 * cap, cap,
                          c->d_count + (size_t)j0 * szg::kCandCountStride, true, &x);
        if (wide && x.matrix == 0) x.matrix = 2;
        if (norms && szg::scan_wants_norms(ix->bits, x, g.block)) x.row_norm = norms;
    }
    return launch_scans_chained(ix, sh, c, a, g, after, part);
}

// the device tail of queries [q0, q1) on stream tl: the float64 distances of what was collected -- on the rows of shard
// `rows` of index `on`: the sweep's own, or the float32 shard a sketch shard stands for --, the counts staying on the
// device; each query's hits sorted by distance there too (lists of up to kSortHitsMax: the host only filters); the
// counters and, where the block is small, the hits on their way back
int collect_tail(const szg_index *on, const Shard *rows, Ctx *c, const CollectBatch &t, size_t s, int q0, int q1, hipStream_t tl)
{
    const uint32_t stride = szg::kCandCountStride;
    const size_t cap = t.cap[s];
    const int nqp = q1 - q0;
    uint32_t *count = c->d_count + (size_t)q0 * stride;
    szg::RerankOut *out = c->d_out + (size_t)q0 * cap;
    HIPCHK(szg::launch_rerank(on->bits, on->metric, rows->rows, on->layout, on->dim, c->d_q64 + (size_t)q0 * on->dim,
                              c->d_collect + (size_t)q0 * cap, count, (uint32_t)cap, nqp, out, tl, stride));
    HIPCHK(szg::launch_sort_hits(out, count, stride, (uint32_t)cap, nqp, tl));
    HIPCHK(hipMemcpyAsync(c->h_count + (size_t)q0 * stride, count, sizeof(uint32_t) * (size_t)nqp * stride, hipMemcpyDeviceToHost, tl));
    if (t.copied[s])
        HIPCHK(hipMemcpyAsync(c->h_out + (size_t)q0 * cap, out, collect_block_entries(cap, nqp) * sizeof(szg::RerankOut),
                              hipMemcpyDeviceToHost, tl));
    return SZG_OK;
}

// what finish() reads off a batch, per query
struct Collected {
    std::vector<std::vector<HeapItem>> cands;         // the hits proper: `distance <= Radius` (collection.go:598) applied here
    std::vector<uint8_t> over;                        // more candidates on some shard than the batch's buffers hold
    std::vector<uint8_t> presorted;                   // the query's hits come from ONE shard's device-sorted list
    std::vector<std::vector<szg_cert_entry>> traced;  // traced calls: every collected entry, before the predicate
    std::vector<uint8_t> untraced;                    // the query's record will not fit the trace: nothing is gathered
    std::vector<std::vector<uint64_t>> nan_rows;      // rows staged ahead of the sweep whose distance is NaN (top-k through
                                                      // the sketch: one among the query's first k rows decides everything)
    double t_wait = 0;                                // of the time spent gathering: waiting for the device
    const bool tracing;
    Collected(int nq, bool tr) : cands(nq), over(nq, 0), presorted(nq, 1), traced(tr ? nq : 0), untraced(tr ? nq : 0, 0), nan_rows(nq), tracing(tr) {}
};

// Wait for batch t shard by shard and gather its queries' hits.  ix: the handle the call was made on (row numbers, the
// trace); swept: the index whose contexts ran the sweeps and whose key_eps bounds their keys (ix, or its sketch index);
// handed: null, or per query "collected nothing by design"; exc: null, or sorted rows whose swept entries mean nothing --
// only an entry staged ahead of the sweep (kNoKeyUkey) counts for them.  A failure leaves the contexts to the caller.
int collect_gather(szg_index *ix, szg_index *swept, const CollectBatch &t, const double *radii, const uint8_t *handed,
                   const std::vector<uint64_t> *exc, Collected *out)
{
    const bool tracing = out->tracing;
    std::vector<uint8_t> lists(t.nq, 0);
    CollectLayout at;
    for (size_t s = 0; s < t.ctx.size(); s++) {
        Ctx *c = t.ctx[s];
        if (!c) continue;
        const Shard *sh = ix->shards[s];
        const double tw = now_us();
        hipError_t e = hipSetDevice(sh->device);
        if (e == hipSuccess) e = hipStreamSynchronize(c->pass.work);
        // (a short call's early part ran its tail on the context's own stream)
        if (e == hipSuccess && c->pass.early_n > 0 && c->pass.early_n < t.nq) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
        int rc = finish_timing(swept, c);
        if (rc) return rc;
        const size_t cap = t.cap[s];
        collect_layout(c->h_count, szg::kCandCountStride, t.nq, cap, t.copied[s] != 0, &at);
        // the next batch on this context starts with room for what this one saw (and shrinks again slowly)
        c->radius_cap = collect_next_cap(c->radius_cap, at.most);
        if (!t.copied[s] && at.host_entries) {
            // exact-size copies of each query's re-ranked hits, back to back in the pinned buffer
            rc = c->h_out.ensure(at.host_entries);
            if (rc) return rc;
            for (int j = 0; j < t.nq && e == hipSuccess; j++)
                if (at.cnt[j])
                    e = hipMemcpyAsync(c->h_out + at.off[j], c->d_out + (size_t)j * cap, at.cnt[j] * sizeof(szg::RerankOut),
                                       hipMemcpyDeviceToHost, c->pass.work);
            if (e == hipSuccess) e = hipStreamSynchronize(c->pass.work);
            if (e != hipSuccess) return fail(SZG_E_DEVICE, "hipMemcpyAsync(radius hits)", e);
        }
        out->t_wait += now_us() - tw;
        for (int j = 0; j < t.nq; j++) {
            if (at.over[j]) out->over[j] = 1;
            if (out->over[j] || (handed && handed[j])) continue;
            const size_t cnt = at.cnt[j];
            std::vector<HeapItem> &cands = out->cands[j];
            cands.reserve(cands.size() + cnt);
            if (cnt && (cnt > (size_t)szg::kSortHitsMax || ++lists[j] > 1)) out->presorted[j] = 0;
            const double rad = radii[t.first + j];
            if (tracing && !out->untraced[j] && !cert_room(ix, out->traced[j].size() + cnt)) {
                out->untraced[j] = 1;
                std::vector<szg_cert_entry>().swap(out->traced[j]);
            }
            const bool keep = tracing && !out->untraced[j];
            for (size_t i = at.off[j]; i < at.off[j] + cnt; i++) {
                const szg::RerankOut &r = c->h_out[i];
                const uint64_t row = sh->first + r.row;
                const bool no_key = r.ukey == kNoKeyUkey;
                // (the bytes that stand in a sketch shard for a row without a usable sketch mean nothing: should the
                // sweep collect such a row, the staged entry is the one that counts)
                if (exc && !no_key && std::binary_search(exc->begin(), exc->end(), row)) continue;
                if (r.dist <= rad) cands.push_back(HeapItem{row, r.dist});  // (a NaN distance is never a hit)
                else if (no_key && std::isnan(r.dist)) out->nan_rows[j].push_back(row);
                if (!keep) continue;
                if (no_key) {
                    out->traced[j].push_back(szg_cert_entry{row, r.dist, 0.0, 0.0f, SZG_CERT_ENTRY_NO_KEY});
                } else {
                    const float key = szg::key_from_ordered(r.ukey);
                    out->traced[j].push_back(szg_cert_entry{row, r.dist, (double)key + key_eps(swept, key, t.meta[j]), key, 0u});
                }
            }
        }
    }
    return SZG_OK;
}

// the certificate record of query j of batch t: what was collected for it on every shard, under its sweep's threshold
void collect_record(szg_index *ix, const szg_index *swept, const CollectBatch &t, int j, int traced_as, int pass, int keys,
                    int sweep, double D, double slack, const std::vector<szg_cert_entry> &entries)
{
    szg_cert_record rec = cert_record(traced_as, pass);
    rec.keys = keys;
    rec.sweep = sweep;
    for (const Shard *sh : ix->shards) rec.row_hi = std::max<uint64_t>(rec.row_hi, sh->first + sh->n_rows);
    rec.thr = (double)t.thr[j];
    rec.eps = key_eps(swept, t.thr[j], t.meta[j]);
    rec.D = D;
    rec.slack = slack;
    cert_emit(ix, rec, entries);
}

// the one end of finish(): the contexts go back -- drained first after a failure --, and under the stats lock the host's
// share of the time is noted and, after a success, count(stats) bumps the caller's counters
template <class Count>
int collect_end(szg_index *ix, CollectBatch &t, int rc, double t0, double t_wait, Count &&count)
{
    if (rc) t.drain();
    else t.release();
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->stats.host_finish_us += now_us() - t0 - t_wait;
    if (rc == SZG_OK) count(ix->stats);
    return rc;
}

// ---- radius searches on the handle's own rows ------------------------------------------------------------------------------

struct RadiusBatch : CollectBatch {
    std::vector<float> thr_single;  // threshold of the single-query collect sweep (a query that overflows is swept again on its own)
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
    t.size();
    t.thr_single.assign(t.nq, 0.0f);
    return t;
}

int RadiusCall::enqueue_shard(RadiusBatch &t, size_t s)
{
    Shard *sh = ix->shards[s];
    Ctx *c = t.ctx[s];
    HIPCHK(hipSetDevice(sh->device));
    // (a shared sweep's batch is up to 96 queries: its buffers keep within the batch limit; a query with more hits than
    // its share is swept again on its own)
    int rc = collect_buffers(t, s, t.nb > 0, 0);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_count, 0, sizeof(uint32_t) * (size_t)t.nq * szg::kCandCountStride, c->pass.work));
    HIPCHK(hipEventRecord(c->ev_up, c->pass.work));  // the sweeps must see the queries, the masks and the zeroed counters
    if (t.nb > 0) {  // one shared sweep for the whole batch
        rc = enqueue_collect_mq(ix, sh, c, t.nq, t.nb, t.any_mask, t.thr.data(), t.cap[s]);
    } else {  // launches of <= 16 sweeps, back to back
        const int qpl = std::max(1, std::min(ix->queries_per_launch, szg::kMaxSweepsPerLaunch));
        rc = collect_sweeps(ix, sh, c, t, t.cap[s], 0, t.nq, qpl, c->pass.work, 0);
    }
    if (rc) return rc;
    return collect_tail(ix, sh, c, t, s, 0, t.nq, c->pass.work);
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
    const double t0 = now_us();
    Collected got(t.nq, tracing);
    int rc = collect_gather(ix, ix, t, radii, nullptr, nullptr, &got);
    for (int j = 0; j < t.nq && rc == SZG_OK; j++) {
        std::vector<HeapItem> &cands = got.cands[j];
        if (got.over[j]) {  // more hits than the batch's buffers hold: the query is swept again on its own
            cands.clear();
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
            got.t_wait += now_us() - tw;
            if (rc) break;
            const double rad = radii[t.first + j];
            for (const Cand &c : all)
                if (c.dist <= rad) cands.push_back(HeapItem{c.row, c.dist});
            got.presorted[j] = 0;
        } else if (tracing && !got.untraced[j]) {
            collect_record(ix, ix, t, j, traced_as(t.first + j), t.nb > 0 ? SZG_CERT_RADIUS_SHARED : SZG_CERT_RADIUS_SINGLE, -1,
                           t.nb == 0 ? 0 : (t.meta[j].mq_bf16 ? 2 : 1), NAN, NAN, got.traced[j]);
        }
        radius_assemble(cands, got.presorted[j] != 0, &(*results)[t.first + j]);
    }
    return collect_end(ix, t, rc, t0, got.t_wait, [&](szg_stats &st) { st.queries += t.nq; });
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
// drop bound.  The batch is a collect batch like RadiusCall's, on the sketch index's contexts and in the sketch
// pre-pass's call and batch plan (sketch_call_plan, sketch_plan_batch); launches of three queries or more without masks
// or tombstones share each row read on the matrix cores (kernels_scan_mx.hip, the collect form), the others keep
// scan_kernel's collect form: a quarter of the bytes either way.  Rows without a usable sketch (sk_exc) are staged as
// the head of each query's collect buffer, the counter starting at their count.  A zero query under cosine, a
// non-finite query or radius, D >= 1 under cosine and a query whose candidates overflow the batch's buffers are handed
// to search_radius_impl, all of a call as ONE call.

struct SketchRadiusBatch : CollectBatch {
    std::vector<double> D;        // the sketch-distance radius per query (real units)
    std::vector<uint8_t> handed;  // handed over before any sweep (its slot collects nothing)
};

struct SketchRadiusCall {
    szg_index *ix;  // the float32 handle (rows, masks, results, trace)
    szg_index *sk;  // its sketch index (contexts, sweeps)
    const double *queries;
    int n_queries;
    const double *radii;
    QueryMasks mask_of;
    std::vector<std::vector<HeapItem>> *results;
    std::vector<int> redo;  // queries handed over to search_radius_impl, ascending
    bool tracing = false;
    SketchPlan p;  // gs, slack and whether the call takes wide batches: as the top-k pre-pass's
    std::vector<double> q_sk;

    int run();
    SketchRadiusBatch plan(int q0);
    int stage(SketchRadiusBatch &t);
    int enqueue_shard(SketchRadiusBatch &t, size_t s, const std::vector<const uint64_t *> &masks);
    int finish(SketchRadiusBatch &t);
};

int SketchRadiusCall::run()
{
    tracing = cert_tracing(ix);
    p = sketch_call_plan(ix, n_queries, 0);
    sk->timing = ix->timing;
    return run_batches<SketchRadiusBatch>(*this);
}

SketchRadiusBatch SketchRadiusCall::plan(int q0)
{
    SketchRadiusBatch t;
    sketch_plan_batch(ix, n_queries, q0, p.wide, &t);
    t.size();
    t.D.assign(t.nq, 0.0);
    t.handed.assign(t.nq, 0);
    t.meta.assign(t.nq, QMeta{});
    return t;
}

int SketchRadiusCall::stage(SketchRadiusBatch &t)
{
    const double t0 = now_us();
    const int dim = ix->dim;
    const double gs = p.gs;
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
        const double D = R * (1.0 + 1e-9) + p.slack;
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
    for (size_t s = 0; s < t.ctx.size() && rc == SZG_OK; s++) {
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

// One shard's part of a collect batch through the sketch, behind its uploads: head[j] -- the entries staged ahead of the
// sweep in query j's buffer (kNoKeyUkey << 32 | shard-local row) -- and the counters that start at their counts, the
// collect sweeps over sketch shard s of sk under t.thr, and the tail on the rows of shard s of ix.  p: the call's plan;
// handed: per query "collects nothing"; floor: collect_buffers'.
int sketch_collect_enqueue(szg_index *ix, szg_index *sk, const SketchPlan &p, CollectBatch &t, size_t s,
                           const std::vector<std::vector<uint64_t>> &head, size_t floor)
{
    Shard *h = sk->shards[s];
    const Shard *a = ix->shards[s];
    Ctx *c = t.ctx[s];
    HIPCHK(hipSetDevice(h->device));
    const uint32_t stride = szg::kCandCountStride;
    size_t head_max = 0;
    for (int j = 0; j < t.nq; j++) head_max = std::max(head_max, head[j].size());
    int rc = collect_buffers(t, s, true, head_max, floor);  // (every batch keeps within the batch limit)
    if (rc == SZG_OK && head_max) rc = c->h_sent.ensure(head_max * (size_t)t.nq);
    if (rc) return rc;
    const size_t cap = t.cap[s];
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
    // launches that may share their row reads on the matrix cores take the rows' norms from the resident array
    const float *norms = nullptr;
    if (!masked && sk->scan_group == 0 && sk->sketch_matrix != 1 &&
        (p.wide || t.nq >= szg::kMatrixMinQueries || sk->sketch_matrix == 2)) {
        int nrc = SZG_OK;
        norms = scan_row_norms(sk, h, &nrc);
        if (nrc) return nrc;
    }
    const LaunchGeom g = scan_geometry(sk, h, 0);
    const int qpl = sketch_collect_launches(sketch_shape(ix, sk), g.grid, g.block, h->has_dead, p.wide, norms != nullptr, t.nq,
                                            std::max(1, std::min(sk->queries_per_launch, szg::kMaxSweepsPerLaunch))).qpl;
    // one part -- or, for a short call (Pass::early_n), two, as enqueue_topk: the first queries' re-rank, sort and
    // copy-back leave the scan stream for the context's own and run beside the call's last sweeps
    const int early = c->pass.early_n > 0 && c->pass.early_n < t.nq ? c->pass.early_n : 0;
    for (int part = early ? 1 : 0; part >= 0 && rc == SZG_OK; part--) {
        const int q0 = part ? 0 : early, q1 = part ? early : t.nq;
        hipStream_t tl = part ? c->stream : c->pass.work;
        rc = collect_sweeps(sk, h, c, t, cap, q0, q1, qpl, tl, part, p.wide != 0, norms);
        // (the re-rank reads the FLOAT32 shard's rows)
        if (rc == SZG_OK) rc = collect_tail(ix, a, c, t, s, q0, q1, tl);
    }
    return rc;
}

int SketchRadiusCall::enqueue_shard(SketchRadiusBatch &t, size_t s, const std::vector<const uint64_t *> &masks)
{
    // the shard's eligible rows without a usable sketch, per query: the head of its collect buffer
    std::vector<std::vector<uint64_t>> head(t.nq);
    for (int j = 0; j < t.nq; j++) {
        if (t.handed[j]) continue;
        sketchless_rows(ix, ix->shards[s], masks[j], [&](uint64_t l, bool ok) {
            if (ok) head[j].push_back(((uint64_t)kNoKeyUkey << 32) | l);
        });
    }
    return sketch_collect_enqueue(ix, sk, p, t, s, head, 0);
}

int SketchRadiusCall::finish(SketchRadiusBatch &t)
{
    if (t.failed) {
        t.drain();
        return SZG_OK;
    }
    const double t0 = now_us();
    Collected got(t.nq, tracing);
    const int rc = collect_gather(ix, sk, t, radii, t.handed.data(), ix->sk_exc.empty() ? nullptr : &ix->sk_exc, &got);
    uint64_t settled = 0, fb = 0;
    for (int j = 0; j < t.nq && rc == SZG_OK; j++) {
        if (got.over[j] || t.handed[j]) {  // (more candidates than the batch's buffers hold: handed over as well)
            redo.push_back(t.first + j);
            fb++;
            continue;
        }
        settled++;
        if (tracing && !got.untraced[j])
            collect_record(ix, sk, t, j, t.first + j, SZG_CERT_SKETCH_RADIUS, SZG_CERT_KEYS_SINGLE, 0, t.D[j], p.slack, got.traced[j]);
        radius_assemble(got.cands[j], got.presorted[j] != 0, &(*results)[t.first + j]);
    }
    return collect_end(ix, t, rc, t0, got.t_wait, [&](szg_stats &st) {
        st.queries += settled;
        st.sketch_radius_queries += settled;
        st.sketch_radius_fallbacks += fb;
    });
}

// ---- top-k of large k through the sketch (option sketch_topk_collect) ------------------------
//
// A top-k search lacks a radius, and a sample gives one with certainty.  Per sketch shard a SAMPLE pass scores every
// stride-th tile of 16 rows against the batch's queries on the matrix cores (kernels_sample_mx.hip; sample_plan.h) and a
// radix select returns w, the (k + e)-th smallest key of the query's eligible sample rows -- e of which are rows without a
// usable sketch, whose dummy bytes may hold any of the smallest keys: at least k of those k + e rows are sketched rows.
// Their real-number sketch keys are at most U = w + key_eps(w): key + key_eps(key) does not fall as the key grows (the
// two-plane integer bound is a constant under cosine and c + 2^-21 |key| under Euclid), so the bound at w covers every
// smaller key.  U implies a sketch distance D_s (rounded up, the mirror image of SketchCall::settle's D_lb), the triangle
// inequality gives d(q, x) <= D_s + slack = tau_s for those k rows, so the query's k-th distance over ALL rows is at most
// tau = min over the shards of tau_s.  A radius search at tau through the sketch -- SketchRadiusCall's collect sweep at
// D = tau (1 + 1e-9) + slack, its re-rank and its gather -- therefore contains the whole answer, ties at the k-th distance
// included; consider() is replayed over what it found, together with the query's first k eligible rows (the reference's
// NaN rule) and the rows without a sketch, staged as the head of the collect buffer.  The thresholds come back in one small
// copy per shard and batch, which stage() waits for: the previous batches' collect sweeps run on the device meanwhile.
// Handed to search_topk_impl, all of a call as ONE call: a NaN among the first k rows or history-dependent candidates
// (tie_mode 0), a zero query under cosine, a non-finite query, D >= 1 under cosine, no shard with k + e eligible sample
// rows, more candidates than the batch's buffers hold.

struct SketchTopkBatch : CollectBatch {
    std::vector<double> D;         // the sketch-distance radius of the collect sweep per query
    std::vector<double> U;         // the bound on the real-number sketch key of k eligible sampled rows (best shard's)
    std::vector<uint8_t> handed;   // handed over before the collect sweep (its slot collects nothing)
    std::vector<std::vector<uint64_t>> firstk;  // per query: its first k eligible rows (index-level)
};

struct SketchTopkCall {
    szg_index *ix;  // the float32 / float64 handle (rows, masks, results, trace)
    szg_index *sk;  // its sketch index (contexts, sweeps)
    const double *queries;
    int n_queries, k;
    QueryMasks mask_of;
    uint64_t *out_rows;
    double *out_dist;
    int32_t *out_count;
    std::vector<int> redo;    // queries handed over to search_topk_impl, ascending
    std::vector<double> tau;  // per query of the call: the radius the sample implies (what collect_gather filters by)
    bool tracing = false;
    SketchPlan p;
    std::vector<double> q_sk;
    std::vector<uint64_t> firstk_open;
    std::vector<Cand> cands;
    std::vector<HeapItem> res;
    std::vector<double> dd;

    int run();
    SketchTopkBatch plan(int q0);
    int stage(SketchTopkBatch &t);
    int enqueue_sample(SketchTopkBatch &t, size_t s, const std::vector<const uint64_t *> &masks);
    void radius_of(SketchTopkBatch &t, int j);
    int finish(SketchTopkBatch &t);
};

// the sample plan of sketch shard h of sk for k and a launch of nq queries
SamplePlan shard_sample_plan(const szg_index *sk, const Shard *h, int k, int nq)
{
    SamplePlanIn in;
    in.rows = h->n_rows;
    in.k = k;
    in.n_queries = nq;
    in.bits = sk->bits;
    in.planes = scan_planes(sk);
    in.tiled = sk->layout.tiled != 0;
    in.steps = sk->layout.steps;
    in.r16 = (uint32_t)sk->map.r16;
    SamplePlan sp = sample_plan(in);
    // (the image of one column block has to fit the LDS)
    if (sp.serves && szg::sample_mx_lds_bytes(in.steps, 1) > 64u * 1024u) sp = SamplePlan{};
    return sp;
}

int SketchTopkCall::run()
{
    tracing = cert_tracing(ix);
    p = sketch_call_plan(ix, n_queries, 0);
    sk->timing = ix->timing;
    tau.assign(n_queries, NAN);
    first_eligible_rows(ix, nullptr, k, &firstk_open);
    return run_batches<SketchTopkBatch>(*this);
}

SketchTopkBatch SketchTopkCall::plan(int q0)
{
    SketchTopkBatch t;
    sketch_plan_batch(ix, n_queries, q0, p.wide, &t);
    t.size();
    t.D.assign(t.nq, NAN);
    t.U.assign(t.nq, NAN);
    t.handed.assign(t.nq, 0);
    t.meta.assign(t.nq, QMeta{});
    t.firstk.assign(t.nq, {});
    return t;
}

// the sample pass of batch t on shard s: the launches (16 queries per row read, 32 where the two-block image fits the
// LDS and the collect form's two-block rules hold) on the shard's scan chain, the select and the copy back behind them
int SketchTopkCall::enqueue_sample(SketchTopkBatch &t, size_t s, const std::vector<const uint64_t *> &masks)
{
    Shard *h = sk->shards[s];
    const Shard *a = ix->shards[s];
    Ctx *c = t.ctx[s];
    HIPCHK(hipSetDevice(h->device));
    const SamplePlan sp = shard_sample_plan(sk, h, k, std::min(t.nq, szg::kMatrixWideQueries));
    if (!sp.serves) return fail(SZG_E_INVALID, "sketch_topk_collect: the sample plan does not serve the shard");
    int nrc = SZG_OK;
    const float *norms = scan_row_norms(sk, h, &nrc);
    if (nrc) return nrc;
    if (!norms) return fail(SZG_E_NOMEM, "sketch_topk_collect: no resident row norms");
    const size_t n_out = 2 * (size_t)kMaxBatch;
    int rc = c->d_keys.ensure((size_t)t.nq * sp.slots);
    if (rc == SZG_OK) rc = c->d_thr.ensure(n_out);
    if (rc == SZG_OK) rc = c->h_thr.ensure(n_out);
    if (rc) return rc;
    uint32_t *keys = reinterpret_cast<uint32_t *>(c->d_keys.data());
    uint32_t *d_sel = reinterpret_cast<uint32_t *>(c->d_thr.data());
    const bool masked = t.any_mask || h->has_dead;
    const LaunchGeom g = scan_geometry(sk, h, 0);
    // (wide launches: the sample's two-block image has to fit LDS as well)
    const CollectLaunches cl = sketch_collect_launches(sketch_shape(ix, sk), g.grid, g.block, h->has_dead, p.wide,
                                                       !masked && szg::sample_mx_lds_bytes(sk->layout.steps, 2) <= 64u * 1024u,
                                                       t.nq, szg::kMatrixQueries);
    const int qpl = cl.qpl;
    std::vector<szg::SampleArgs> launches;
    for (int j0 = 0; j0 < t.nq; j0 += qpl) {
        szg::SampleArgs x;
        fill_scan_args(sk, h, c, t.any_mask, j0, std::min(qpl, t.nq - j0), &x.a);
        x.a.row_norm = norms;
        x.stride = sp.stride;
        x.tiles = (uint32_t)sp.tiles;
        x.slots = (uint32_t)sp.slots;
        x.keys = keys + (size_t)j0 * sp.slots;
        launches.push_back(x);
    }
    const int block = 256;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((sp.tiles + 3) / 4, (uint64_t)h->cu_count * 8));
    rc = chain_sweeps(sk, h, c, c->pass.work, 0, (int)launches.size(), "szg::launch_sample_mx", [&](hipStream_t st) {
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < launches.size() && e == hipSuccess; i++)
            e = szg::launch_sample_mx(sk->metric, launches[i], cl.wide32 ? 2 : 1, grid, block, st);
        return e;
    });
    if (rc) return rc;
    // the rank asked of the shard: k + the shard's eligible rows without a usable sketch that lie in the sample
    szg::SampleSelectArgs sel{};
    sel.keys = keys;
    sel.slots = (uint32_t)sp.slots;
    sel.out = d_sel;
    for (int j0 = 0; j0 < t.nq; j0 += szg::kMatrixWideQueries) {
        const int n = std::min(szg::kMatrixWideQueries, t.nq - j0);
        for (int j = 0; j < n; j++) {
            uint32_t e = 0;
            sketchless_rows(ix, a, masks[j0 + j], [&](uint64_t l, bool ok) { e += ok && ((l >> 4) % sp.stride) == 0 ? 1u : 0u; });
            sel.rank[j] = t.handed[j0 + j] ? 0u : (uint32_t)k + e;
        }
        sel.keys = keys + (size_t)j0 * sp.slots;
        sel.out = d_sel + 2 * (size_t)j0;
        HIPCHK(szg::launch_sample_select(sel, n, c->pass.work));
    }
    HIPCHK(hipMemcpyAsync(c->h_thr.data(), d_sel, sizeof(uint32_t) * 2 * (size_t)t.nq, hipMemcpyDeviceToHost, c->pass.work));
    {
        std::lock_guard<std::mutex> lk(sk->stats_mu);
        sk->stats.scan_launches += launches.size();
        sk->stats.scan_bytes += (uint64_t)launches.size() * sp.sample_rows * (uint64_t)sk->row_bytes;
    }
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->sk_topk.sample_rows += (uint64_t)launches.size() * sp.sample_rows;
    return SZG_OK;
}

// query j of batch t, once every shard's sample keys are back: U, tau and D -- or the hand-over
void SketchTopkCall::radius_of(SketchTopkBatch &t, int j)
{
    if (t.handed[j]) return;
    double best = INFINITY, best_U = NAN;
    for (size_t s = 0; s < t.ctx.size(); s++) {
        const Ctx *c = t.ctx[s];
        if (!c) continue;
        const uint32_t uk = reinterpret_cast<const uint32_t *>(c->h_thr.data())[2 * j];
        if (uk == kSampleNoKey) continue;  // fewer eligible sample rows than the rank: the shard bounds nothing
        const double w = (double)szg::key_from_ordered(uk);
        const double U = w + key_eps(sk, w, t.meta[j]);
        double Ds;
        if (p.gs > 0.0) {
            Ds = p.gs * std::sqrt(std::max(U, 0.0)) / 255.0 * (1.0 + 1e-9);
        } else {
            const double x = -U - 1e-15;  // (a lower bound of the cosine, rounding included)
            Ds = x >= 1.0 ? 0.0 : (x <= -1.0 ? 1.0 : std::acos(x) / M_PI * (1.0 + 1e-12));
        }
        const double ts = Ds + p.slack;
        if (ts < best) best = ts, best_U = U;
    }
    const double D = best * (1.0 + 1e-9) + p.slack;  // the collect sweep's sketch-distance radius, as SketchRadiusCall's
    tau[t.first + j] = best;
    t.U[j] = best_U;
    if (!std::isfinite(best) || !std::isfinite(D) || (p.gs <= 0.0 && D >= 1.0)) {
        t.handed[j] = 1;
        return;
    }
    t.D[j] = D;
}

int SketchTopkCall::stage(SketchTopkBatch &t)
{
    const double t0 = now_us();
    const int dim = ix->dim;
    const double gs = p.gs;
    const double *q = queries + (size_t)t.first * dim;
    const std::vector<const uint64_t *> masks = t.masks(mask_of);
    const std::vector<const szg_mask *> handles = t.handles(mask_of);
    // the query forms of the sketch: q / gscale under Euclid; a query that is handed over sweeps as zeros and collects nothing
    q_sk.assign((size_t)t.nq * dim, 0.0);
    for (int j = 0; j < t.nq; j++) {
        const double *qj = q + (size_t)j * dim;
        double m1 = 0.0;
        bool finite = true;
        for (int i = 0; i < dim; i++) {
            finite = finite && std::isfinite(qj[i]);
            m1 += qj[i] * qj[i];
        }
        t.handed[j] = !finite || !std::isfinite(m1) || (gs <= 0.0 && m1 == 0.0);
        if (t.handed[j]) continue;
        for (int i = 0; i < dim; i++) q_sk[(size_t)j * dim + i] = gs > 0.0 ? qj[i] / gs : qj[i];
        if (masks[j]) first_eligible_rows(ix, masks[j], k, &t.firstk[j]);
        else t.firstk[j] = firstk_open;
    }
    int rc = stage_query_forms(sk, t, q_sk.data(), false, [&](int j, QMeta &meta) { t.meta[j] = meta; });
    if (rc) return rc;
    const double t1 = now_us();
    // the uploads and the sample pass on every shard
    for (size_t s = 0; s < t.ctx.size() && rc == SZG_OK; s++) {
        if (!t.ctx[s]) continue;
        rc = enqueue_queries(sk, sk->shards[s], t.ctx[s], q, t.nq, t.any_mask ? masks.data() : nullptr, true,
                             handles.empty() ? nullptr : handles.data(), s);
        if (rc == SZG_OK) rc = enqueue_sample(t, s, masks);
    }
    // the one wait of the batch: the sample keys (earlier batches' collect sweeps and tails run on meanwhile)
    for (size_t s = 0; s < t.ctx.size() && rc == SZG_OK; s++) {
        if (!t.ctx[s]) continue;
        hipError_t e = hipSetDevice(sk->shards[s]->device);
        if (e == hipSuccess) e = hipStreamSynchronize(t.ctx[s]->pass.work);
        if (e != hipSuccess) rc = fail(SZG_E_DEVICE, "hipStreamSynchronize(sample keys)", e);
    }
    if (rc) return rc;
    for (int j = 0; j < t.nq; j++) {
        radius_of(t, j);
        // (radius_key_threshold on the sketch handle, as SketchRadiusCall; a slot that is handed over: below every key)
        t.thr[j] = t.handed[j] ? -FLT_MAX : radius_key_threshold(sk, gs > 0.0 ? t.D[j] / gs : t.D[j], t.meta[j]);
    }
    // the collect sweeps at the radii found: the head of each query's buffer holds its eligible rows without a usable
    // sketch and its first k eligible rows
    for (size_t s = 0; s < t.ctx.size() && rc == SZG_OK; s++) {
        if (!t.ctx[s]) continue;
        const Shard *a = ix->shards[s];
        std::vector<std::vector<uint64_t>> head(t.nq);
        size_t floor = 0;
        for (int j = 0; j < t.nq; j++) {
            if (t.handed[j]) continue;
            sketchless_rows(ix, a, masks[j], [&](uint64_t l, bool ok) {
                if (ok) head[j].push_back(((uint64_t)kNoKeyUkey << 32) | l);
            });
            for (uint64_t r : t.firstk[j])
                if (r >= a->first && r < a->first + a->n_rows) head[j].push_back(((uint64_t)kNoKeyUkey << 32) | (r - a->first));
        }
        floor = shard_sample_plan(sk, sk->shards[s], k, std::min(t.nq, szg::kMatrixWideQueries)).cap;
        rc = sketch_collect_enqueue(ix, sk, p, t, s, head, floor);
    }
    note_stage_times(ix, t0, t1);
    return rc;
}

int SketchTopkCall::finish(SketchTopkBatch &t)
{
    if (t.failed) {
        t.drain();
        return SZG_OK;
    }
    const double t0 = now_us();
    Collected got(t.nq, tracing);
    const int rc = collect_gather(ix, sk, t, tau.data(), t.handed.data(), ix->sk_exc.empty() ? nullptr : &ix->sk_exc, &got);
    uint64_t settled = 0, fb = 0, over = 0, n_cands = 0;
    for (int j = 0; j < t.nq && rc == SZG_OK; j++) {
        const int qi = t.first + j;
        bool ok = !t.handed[j] && !got.over[j];
        if (got.over[j] && !t.handed[j]) over++;
        if (ok) {
            // a NaN among the query's first k rows decides everything in the reference's heap; elsewhere it never enters
            bool nan_first = false;
            for (uint64_t r : got.nan_rows[j])
                nan_first = nan_first || std::find(t.firstk[j].begin(), t.firstk[j].end(), r) != t.firstk[j].end();
            n_cands += got.cands[j].size();
            // The candidates number a few k stride, the answer k: only the nearest matter.  A first-k row that the sweep
            // collected as well is there twice -- at most k such pairs -- so the 2 k + 1 nearest entries hold the k + 1
            // nearest ROWS; among distances without a tie there (and no NaN: none is ever a hit) the reference's heap ends
            // with the k nearest whatever it saw on the way, so consider() is replayed over those rows alone.
            auto load = [&](size_t keep) {
                cands.clear();
                for (const HeapItem &h : got.cands[j]) cands.push_back(Cand{h.row, h.priority, 0.0f, 0.0});
                if (cands.size() > keep) {
                    auto nearer = [](const Cand &x, const Cand &y) { return x.dist < y.dist || (x.dist == y.dist && x.row < y.row); };
                    std::nth_element(cands.begin(), cands.begin() + keep, cands.end(), nearer);
                    cands.resize(keep);
                }
                std::sort(cands.begin(), cands.end(), [](const Cand &x, const Cand &y) { return x.row < y.row; });
                cands.erase(std::unique(cands.begin(), cands.end(), [](const Cand &x, const Cand &y) { return x.row == y.row; }),
                            cands.end());
            };
            load(2 * (size_t)k + 1);
            dd.clear();
            for (const Cand &c : cands) dd.push_back(c.dist);
            const bool tied = history_dependent(dd.data(), dd.size(), k);
            if (tied && ix->tie_mode != 0) load(SIZE_MAX);  // (the fast answer is kept: the heap sees every candidate)
            replay_topk(cands, k, &res);
            // every row that was not collected is farther than tau: final with k results at or below it; equal distances
            // among the best k + 1 under tie_mode 0: the full-precision path replays every row
            ok = (!nan_first || ix->tie_mode != 0) && (!tied || ix->tie_mode != 0) && (int)res.size() == k &&
                 res.back().priority <= tau[qi];
        }
        const bool swept = !t.handed[j], gathered = swept && !got.over[j];
        if (tracing && !(gathered && got.untraced[j])) {
            szg_cert_record rec = cert_record(qi, SZG_CERT_SKETCH_TOPK_COLLECT);
            rec.keys = SZG_CERT_KEYS_SINGLE;
            rec.sweep = 0;
            rec.certified = ok ? 1 : 0;
            rec.k = k;
            for (const Shard *sh : ix->shards) rec.row_hi = std::max<uint64_t>(rec.row_hi, sh->first + sh->n_rows);
            rec.slack = p.slack;
            rec.kmax = t.U[j];
            rec.thr_min = tau[qi];
            if (gathered) {  // (a query handed over before the sweep, or whose candidates overflowed: no sweep on record)
                rec.thr = (double)t.thr[j];
                rec.eps = key_eps(sk, t.thr[j], t.meta[j]);
                rec.D = t.D[j];
            }
            static const std::vector<szg_cert_entry> none;
            cert_emit(ix, rec, gathered ? got.traced[j] : none);
        }
        if (!ok) {
            redo.push_back(qi);
            fb++;
            continue;
        }
        settled++;
        emit_topk(ix, res, k, qi, out_rows, out_dist, out_count);
    }
    return collect_end(ix, t, rc, t0, got.t_wait, [&](szg_stats &st) {
        st.queries += settled;
        ix->sk_topk.queries += settled;
        ix->sk_topk.fallbacks += fb;
        ix->sk_topk.overflows += over;
        ix->sk_topk.candidates += n_cands;
    });
}

}  // namespace

bool sketch_topk_collect_serves(const szg_index *ix, int k)
{
    const szg_index *sk = ix->sketch;
    if (!sk || sk->scan_norms == 1) return false;  // (the sample pass reads the rows' resident norms)
    bool any = false;
    for (const Shard *h : sk->shards) {
        if (h->n_rows == 0) continue;
        any = true;
        if (!shard_sample_plan(sk, h, k, 1).serves) return false;
    }
    return any;
}

int search_topk_collect(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                        uint64_t *out_rows, double *out_dist, int32_t *out_count, const uint64_t *const *allow_ptrs,
                        const szg_mask *const *handles)
{
    int rc = sketch_sync_for_search(ix);
    if (rc) return rc;
    // (a shard the plan does not serve: the path the call takes without the option -- not a fallback, not counted)
    if (ix->sk_disabled || ix->sk_nomem || !sketch_topk_collect_serves(ix, k))
        return search_topk_impl(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles);
    SketchTopkCall call{ix, ix->sketch, queries, n_queries, k, QueryMasks(ix, allow_bits, allow_ptrs, handles), out_rows,
                        out_dist, out_count};
    rc = call.run();
    if (rc && ix->sketch_on == 2) {
        // (a failure inside the pipeline: the sketch index stays until the next load, the whole call goes the
        // full-precision way -- as search_topk_sketch)
        ix->sk_nomem = true;
        return search_topk_impl(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles);
    }
    if (rc || call.redo.empty()) return rc;
    // the queries handed over: ONE call of the full-precision path (no entry in the pre-pass's automatic window)
    std::sort(call.redo.begin(), call.redo.end());
    const int m = (int)call.redo.size();
    const HandedOver h(ix, queries, call.mask_of, call.redo);
    std::vector<uint64_t> r2((size_t)m * k);
    std::vector<double> d2((size_t)m * k);
    std::vector<int32_t> c2(m);
    rc = search_topk_impl(ix, h.q.data(), m, k, nullptr, r2.data(), d2.data(), c2.data(), h.mask_ptrs(), h.handle_ptrs(),
                          call.redo.data());
    if (rc) return rc;
    for (int i = 0; i < m; i++) {
        memcpy(out_rows + (size_t)call.redo[i] * k, &r2[(size_t)i * k], sizeof(uint64_t) * k);
        memcpy(out_dist + (size_t)call.redo[i] * k, &d2[(size_t)i * k], sizeof(double) * k);
        if (out_count) out_count[call.redo[i]] = c2[i];
    }
    return SZG_OK;
}

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
    const HandedOver h(ix, queries, call.mask_of, call.redo);
    std::vector<double> r2(m);
    for (int i = 0; i < m; i++) r2[i] = radii[call.redo[i]];
    std::vector<std::vector<HeapItem>> hits2;
    rc = search_radius_impl(ix, h.q.data(), m, r2.data(), h.mask_ptrs(), &hits2, h.handle_ptrs(), call.redo.data());
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

using szgi::fail;

extern "C" {

int szg_index_sketch_topk_stats(szg_index *ix, szg_sketch_topk_stats *out)
{
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    *out = ix->sk_topk;
    return SZG_OK;
}

// the sample plan of a top-k search through the sketch (sample_plan.h), for a shard of the given shape
int szg_debug_sample_plan(uint64_t shard_rows, int k, int n_queries, int dim, int quant_bits, int planes, szg_sample_plan *out)
{
    SZG_TRY
    using namespace szgi;
    if (!out) return fail(SZG_E_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    if (n_queries < 1 || n_queries > szg::kMatrixWideQueries) return fail(SZG_E_INVALID, "n_queries out of range");
    RowFormat f;
    const int rc = row_format(dim, quant_bits, &f);
    if (rc == SZG_E_INVALID) return rc;
    if (rc) return SZG_OK;  // (a query that does not fit the scan's LDS: not served)
    SamplePlanIn in;
    in.rows = shard_rows;
    in.k = k;
    in.n_queries = n_queries;
    in.bits = quant_bits;
    in.planes = planes;
    in.tiled = f.layout.tiled != 0;
    in.steps = f.layout.steps;
    in.r16 = (uint32_t)f.map.r16;
    const SamplePlan sp = sample_plan(in);
    if (!sp.serves || szg::sample_mx_lds_bytes(in.steps, 1) > 64u * 1024u) return SZG_OK;
    out->serves = 1;
    out->stride = (int32_t)sp.stride;
    out->blocks = n_queries > szg::kMatrixQueries && szg::sample_mx_lds_bytes(in.steps, 2) <= 64u * 1024u ? 2 : 1;
    out->tiles = sp.tiles;
    out->sample_rows = sp.sample_rows;
    out->slots = sp.slots;
    out->key_bytes = sp.key_bytes;
    out->cap = sp.cap;
    out->lds_bytes = szg::sample_mx_lds_bytes(in.steps, out->blocks);
    return SZG_OK;
    SZG_CATCH
}

}  // extern "C"
