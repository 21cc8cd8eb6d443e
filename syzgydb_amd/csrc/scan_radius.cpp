// scan_radius.cpp -- radius search, Search{Precision:"exact", Radius > 0} (K is ignored: collection.go:598-605).
//
// A radius search is a COLLECT sweep: every row whose scan key is at or below a threshold derived from the radius
// (plus the key's error bound) is appended to the query's buffer, the hits are re-ranked in float64 and the
// reference's exact predicate `distance <= Radius` (:598) decides.  The sweeps of a batch are walked query-major by
// ONE launch (per-sweep threshold, buffer and counter in ScanArgs), the re-rank reads the hit counters on the
// device, and up to three batches are in flight per shard -- no launch gap and no host round trip between the sweeps
// of a batch, which is what a single query per launch per caller used to cost (5.7 of 6.9 TB/s on cfg5's shard).
// RadiusCall sweeps the handle's own rows, SketchRadiusCall (option sketch_radius) the 8-bit sketch of float32 rows: what
// a batch is on the device and how it is read back exists once, in the collect core (scan_collect.h: top-k of large k
// through the sketch, scan_sketch_topk.cpp, is its third caller); its arithmetic is collect_plan.h.
#include "scan_collect.h"

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

// ---- the collect core (scan_collect.h): one batch of collect sweeps on the device and back ------------------------------

int collect_buffers(CollectBatch &t, size_t s, bool limited, size_t head_max, size_t floor)
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

int collect_sweeps(szg_index *ix, Shard *sh, Ctx *c, const CollectBatch &t, size_t cap, int q0, int q1, int qpl,
                   hipStream_t after, int part, bool wide, const float *norms)
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

void collect_record(szg_index *ix, const szg_index *swept, const CollectBatch &t, int j, int traced_as, int pass, int keys,
                    int sweep, double D, double slack, const std::vector<szg_cert_entry> &entries)
{
    szg_cert_record rec = cert_record(ix, traced_as, pass);
    rec.keys = keys;
    rec.sweep = sweep;
    rec.thr = (double)t.thr[j];
    rec.eps = key_eps(swept, t.thr[j], t.meta[j]);
    rec.D = D;
    rec.slack = slack;
    cert_emit(ix, rec, entries);
}

void sketchless_head(const szg_index *ix, const Shard *a, const uint64_t *m, std::vector<uint64_t> *head)
{
    sketchless_rows(ix, a, m, [&](uint64_t l, bool ok) {
        if (ok) head->push_back(((uint64_t)kNoKeyUkey << 32) | l);
    });
}

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

namespace {

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
//     d(q, x) <= R   =>   d(q, s) <= d(q, x) + d(x, s) <= R + A <= D = sketch_collect_radius(R, slack)
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
    results->assign(n_queries, {});
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
    for (int j = 0; j < t.nq; j++) {
        // (a non-finite radius gives a non-finite D)
        t.D[j] = sketch_collect_radius(radii[t.first + j], p.slack);
        t.handed[j] = sketch_query_handed(q + (size_t)j * dim, dim, gs) || sketch_radius_handed(gs, t.D[j]);
    }
    int rc = sketch_stage_forms(sk, gs, t, q, t.handed.data(), &q_sk, [&](int j, QMeta &meta) {
        t.meta[j] = meta;
        // (radius_key_threshold on the sketch handle, with the sketch's constants: key_eps is the two-plane integer bound;
        // a slot that is handed over: below every key)
        t.thr[j] = t.handed[j] ? -FLT_MAX : radius_key_threshold(sk, sketch_key_radius(gs, t.D[j]), meta);
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

int SketchRadiusCall::enqueue_shard(SketchRadiusBatch &t, size_t s, const std::vector<const uint64_t *> &masks)
{
    // the shard's eligible rows without a usable sketch, per query: the head of its collect buffer
    std::vector<std::vector<uint64_t>> head(t.nq);
    for (int j = 0; j < t.nq; j++)
        if (!t.handed[j]) sketchless_head(ix, ix->shards[s], masks[j], &head[j]);
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
    SketchRadiusCall call{ix, nullptr, queries, n_queries, radii, QueryMasks(ix, nullptr, masks, handles), results};
    return sketch_served_call(
        ix, call, [] { return true; },
        [&] { return search_radius_impl(ix, queries, n_queries, radii, masks, results, handles); },
        // (no entry in the top-k auto window, sk_hist: radius hand-overs say nothing about top-k certificates)
        [&](const HandedOver &h, const std::vector<int> &redo) {
            const int m = (int)redo.size();
            std::vector<double> r2(m);
            for (int i = 0; i < m; i++) r2[i] = radii[redo[i]];
            std::vector<std::vector<HeapItem>> hits2;
            const int rc = search_radius_impl(ix, h.q.data(), m, r2.data(), h.mask_ptrs(), &hits2, h.handle_ptrs(), redo.data());
            if (rc) return rc;
            for (int i = 0; i < m; i++) (*results)[redo[i]].swap(hits2[i]);
            return (int)SZG_OK;
        });
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
