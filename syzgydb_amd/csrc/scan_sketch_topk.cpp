// scan_sketch_topk.cpp -- top-k of large k through the 8-bit sketch (option sketch_topk_collect).
//
// A top-k search lacks a radius, and a sample gives one with certainty.  Per sketch shard a SAMPLE pass scores every
// stride-th tile of 16 rows against the batch's queries on the matrix cores (kernels_sample_mx.hip; sample_plan.h) and a
// radix select returns w, the (k + e)-th smallest key of the query's eligible sample rows -- e of which are rows without a
// usable sketch, whose dummy bytes may hold any of the smallest keys: at least k of those k + e rows are sketched rows.
// Their real-number sketch keys are at most U = w + key_eps(w): key + key_eps(key) does not fall as the key grows (the
// two-plane integer bound is a constant under cosine and c + 2^-21 |key| under Euclid), so the bound at w covers every
// smaller key.  U implies a sketch distance D_s (sketch_dist_above, sketch_bound.h: rounded up), the triangle
// inequality gives d(q, x) <= D_s + slack = tau_s for those k rows, so the query's k-th distance over ALL rows is at most
// tau = min over the shards of tau_s.  A radius search at tau through the sketch -- SketchRadiusCall's collect sweep at
// D = sketch_collect_radius(tau, slack), its re-rank and its gather (the collect core, scan_collect.h) -- therefore
// contains the whole answer, ties at the k-th distance
// included; consider() is replayed over what it found, together with the query's first k eligible rows (the reference's
// NaN rule) and the rows without a sketch, staged as the head of the collect buffer.  The thresholds come back in one small
// copy per shard and batch, which stage() waits for: the previous batches' collect sweeps run on the device meanwhile.
// Handed to search_topk_impl, all of a call as ONE call: a NaN among the first k rows or history-dependent candidates
// (tie_mode 0), a zero query under cosine, a non-finite query, D >= 1 under cosine, no shard with k + e eligible sample
// rows, more candidates than the batch's buffers hold.
#include "sample_plan.h"
#include "scan_collect.h"

namespace szgi {

namespace {

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
        const double ts = sketch_dist_above(p.gs, U) + p.slack;
        if (ts < best) best = ts, best_U = U;
    }
    const double D = sketch_collect_radius(best, p.slack);  // the collect sweep's sketch-distance radius, as SketchRadiusCall's
    tau[t.first + j] = best;
    t.U[j] = best_U;
    if (sketch_radius_handed(p.gs, D)) {  // (no shard bounds anything, or an overflowing one: a non-finite D)
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
    for (int j = 0; j < t.nq; j++) {
        t.handed[j] = sketch_query_handed(q + (size_t)j * dim, dim, gs);
        if (t.handed[j]) continue;
        if (masks[j]) first_eligible_rows(ix, masks[j], k, &t.firstk[j]);
        else t.firstk[j] = firstk_open;
    }
    int rc = sketch_stage_forms(sk, gs, t, q, t.handed.data(), &q_sk, [&](int j, QMeta &meta) { t.meta[j] = meta; });
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
        t.thr[j] = t.handed[j] ? -FLT_MAX : radius_key_threshold(sk, sketch_key_radius(gs, t.D[j]), t.meta[j]);
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
            sketchless_head(ix, a, masks[j], &head[j]);
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
                unique_rows(cands);
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
            szg_cert_record rec = cert_record(ix, qi, SZG_CERT_SKETCH_TOPK_COLLECT);
            rec.keys = SZG_CERT_KEYS_SINGLE;
            rec.sweep = 0;
            rec.certified = ok ? 1 : 0;
            rec.k = k;
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
    SketchTopkCall call{ix, nullptr, queries, n_queries, k, QueryMasks(ix, allow_bits, allow_ptrs, handles), out_rows, out_dist,
                        out_count};
    return sketch_served_call(
        ix, call, [&] { return sketch_topk_collect_serves(ix, k); },  // (every shard's sample plan)
        [&] { return search_topk_impl(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles); },
        [&](const HandedOver &h, const std::vector<int> &redo) {
            return search_topk_handed(ix, h, redo, k, out_rows, out_dist, out_count);
        });
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
