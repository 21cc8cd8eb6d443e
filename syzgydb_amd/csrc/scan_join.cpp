// scan_join.cpp -- neighbours of stored rows (szg_index_neighbors).
//
// Entry i is what szg_search_topk_masked answers on the handle for the float64 decode of stored row q_i.  Two routes:
//   the parent's route, for every handle: the rows are decoded on the card (launch_fetch) into the handle's conversion
//     buffer, copied to its pinned twin and handed to the masked search as ONE call;
//   the join, where join_plan serves (a handle that keeps a tiled 8-bit sketch, kp <= 96, one device, at least
//     join_min queries -- by default no call: kJoinMinQueries, join_plan.h): per launch of up to kJoinBatch queries the query rows' sketch rows are packed from the
//     resident sketch (launch_gather_rows), swept against every sketch shard on the matrix cores (kernels_join.hip),
//     the slices' lists merged (launch_merge_short), and ONE float64 re-rank per shard on the real rows -- the queries'
//     float64 image is launch_fetch's decode, on the card -- settles the query by the pre-pass's certificate with 2 A for
//     A: d(x_j, x_i) >= d(s_j, s_i) - d(x_j, s_j) - d(x_i, s_i).  What it does not settle takes the parent's route, ONE call.
// Everything runs on the null stream under ix->join_mu; the scratch is kept between calls.
#include "scan_internal.h"

namespace szgi {

namespace {

// |float32 key - real-number sketch key| of the join's arithmetic (kernels_join.hip).  Euclid: the key is an exact
// integer rounded once to float32 (exact below 2^24).  Cosine: the exact integer dot rounded once, two factors
// 1 / |n| rounded once each from float64, two products: five roundings of a value of at most 1 in magnitude.
double join_key_eps(int metric, double key)
{
    if (metric == SZG_COSINE) return 6.0 * 0x1p-24;
    return std::fabs(key) * 0x1p-23 + 1e-30;  // (a row meets its own sketch at key 0: the bound stays positive, as key_bound's)
}

struct JoinCall {
    szg_index *ix;
    szg_index *sk;
    const uint64_t *qrows;  // index-level rows (no row base), n_queries of them
    int n_queries, k;
    const szg_mask *mask;
    uint64_t *out_rows;
    double *out_dist;
    int32_t *out_count;
    std::vector<int> redo;

    int kp = 0;
    SketchPlan p;
    bool masked = false, tracing = false;
    std::vector<int> extra;            // per shard: the drop bound's slot, k first rows, remembered rows
    std::vector<size_t> cand_off;      // per shard: its first entry in a query-major record of `stride` entries
    size_t stride = 0;                 // entries per query over all shards
    std::vector<uint64_t> firstk;
    std::vector<size_t> stat_off;      // per shard: its first row in row_stat
    std::vector<Cand> cands;
    std::vector<HeapItem> res;
    std::vector<double> dd;
    uint64_t launches = 0, bytes = 0;

    int run();
    int batch(int q0, int nq);
    void settle(int qi, const szg::RerankOut *rec);
};

template <class T>
int on_device(DevMem<T> &m, int device, size_t n, const char *what)
{
    if (m.device() != device) m = DevMem<T>(device);
    return m.ensure(n, what);
}

int JoinCall::run()
{
    const size_t n_sh = ix->shards.size();
    const int dim = ix->dim, device = ix->shards[0]->device;
    JoinScratch &s = ix->join;
    tracing = cert_tracing(ix);
    const int kk = k + ix->sketch_extra;
    kp = kk + std::max(ix->slack_min, kk / 2);
    p = sketch_call_plan(ix, n_queries, kp);
    const uint64_t *mw = mask ? mask_host_words(mask) : nullptr;
    first_eligible_rows(ix, mw, k, &firstk);
    extra.assign(n_sh, 0);
    cand_off.assign(n_sh, 0);
    stat_off.assign(n_sh, 0);
    size_t rows_total = 0;
    stride = 0;
    for (size_t i = 0; i < n_sh; i++) {
        const Shard *a = ix->shards[i];
        size_t exc = 0;
        for (uint64_t r : ix->sk_exc) exc += (r >= a->first && r < a->first + a->n_rows) ? 1 : 0;
        extra[i] = 1 + k + (int)exc;
        cand_off[i] = stride;
        if (a->n_rows) stride += (size_t)kp + extra[i];
        stat_off[i] = rows_total;
        rows_total += (size_t)((a->n_rows + 15) & ~15ull);
        masked = masked || a->has_dead;
    }
    masked = masked || mask != nullptr;
    HIPCHK(hipSetDevice(device));
    const size_t B = (size_t)std::min(n_queries, szg::kJoinBatch), Bt = (B + 15) / 16;
    int rc = on_device(s.row_stat, device, rows_total, "hipMalloc(join row sums)");
    if (rc == SZG_OK) rc = on_device(s.q_stat, device, Bt * 16, "hipMalloc(join query sums)");
    if (rc == SZG_OK) rc = on_device(s.qtiles, device, Bt * 16 * (size_t)dim, "hipMalloc(join query tiles)");
    if (rc == SZG_OK) rc = on_device(s.q64, device, B * (size_t)dim, "hipMalloc(join queries)");
    if (rc == SZG_OK) rc = on_device(s.qlist, device, 2 * B, "hipMalloc(join query rows)");
    if (rc == SZG_OK) rc = on_device(s.lists, device, B * szg::kJoinMaxSlices * szg::kRowListMax, "hipMalloc(join lists)");
    if (rc == SZG_OK) rc = on_device(s.cand, device, B * stride, "hipMalloc(join candidates)");
    if (rc == SZG_OK) rc = on_device(s.out, device, B * stride, "hipMalloc(join distances)");
    if (rc == SZG_OK) rc = s.h_qlist.ensure(2 * B, "hipHostMalloc(join query rows)");
    if (rc == SZG_OK) rc = s.h_cand.ensure(B * stride, "hipHostMalloc(join candidates)");
    if (rc == SZG_OK) rc = s.h_out.ensure(B * stride, "hipHostMalloc(join distances)");
    if (rc) return rc;
    for (size_t i = 0; i < n_sh; i++) {
        const Shard *h = sk->shards[i];
        if (h->n_rows == 0) continue;
        HIPCHK(szg::launch_join_row_stats(h->rows, (uint32_t)h->n_rows, sk->layout.steps, dim, s.row_stat + stat_off[i], nullptr));
    }
    redo.reserve(n_queries);
    for (int q0 = 0; q0 < n_queries && rc == SZG_OK; q0 += szg::kJoinBatch) rc = batch(q0, std::min(szg::kJoinBatch, n_queries - q0));
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->nb.join_queries += (uint64_t)n_queries;
    ix->nb.join_fallbacks += redo.size();
    ix->nb.join_launches += launches;
    ix->nb.join_bytes += bytes;
    ix->stats.queries += (uint64_t)n_queries - redo.size();
    return rc;
}

// queries [q0, q0 + nq) of the call: one launch of the join per sketch shard
int JoinCall::batch(int q0, int nq)
{
    const size_t n_sh = ix->shards.size();
    const int dim = ix->dim;
    JoinScratch &s = ix->join;
    // the launch's queries grouped by the shard that holds their row (a gather packs one shard's rows back to back):
    // pos[j] = the place of query q0 + j in the launch
    std::vector<int> pos(nq);
    std::vector<size_t> first_pos(n_sh + 1, 0);
    {
        std::vector<size_t> count(n_sh, 0);
        std::vector<int> shard_of_q(nq);
        for (int j = 0; j < nq; j++) {
            size_t i = 0;
            while (!(qrows[q0 + j] >= ix->shards[i]->first && qrows[q0 + j] < ix->shards[i]->first + ix->shards[i]->n_rows)) i++;
            shard_of_q[j] = (int)i;
            count[i]++;
        }
        for (size_t i = 0; i < n_sh; i++) first_pos[i + 1] = first_pos[i] + count[i];
        std::vector<size_t> at(first_pos.begin(), first_pos.end() - 1);
        for (int j = 0; j < nq; j++) pos[j] = (int)at[shard_of_q[j]]++;
        for (int j = 0; j < nq; j++) {
            const Shard *a = ix->shards[shard_of_q[j]];
            s.h_qlist[pos[j]] = qrows[q0 + j] - a->first;  // shard-local: the gather's list
            s.h_qlist[nq + pos[j]] = qrows[q0 + j];        // index-level: the fetch's list
        }
    }
    HIPCHK(hipMemcpyAsync(s.qlist, s.h_qlist, sizeof(uint64_t) * 2 * nq, hipMemcpyHostToDevice, nullptr));
    for (size_t i = 0; i < n_sh; i++) {
        const Shard *a = ix->shards[i], *h = sk->shards[i];
        const size_t n = first_pos[i + 1] - first_pos[i];
        if (n == 0) continue;
        HIPCHK(szg::launch_fetch(ix->bits, a->rows, ix->layout, dim, n, s.qlist + nq + first_pos[i], a->first, a->n_rows, 0,
                                 s.q64 + first_pos[i] * (size_t)dim, 0, (uint64_t)dim, nullptr));
        HIPCHK(szg::launch_gather_rows(h->rows, sk->layout, s.qtiles, sk->layout, (uint32_t)(dim / 16), s.qlist + first_pos[i], n,
                                       first_pos[i], nullptr));
    }
    HIPCHK(szg::launch_join_row_stats(s.qtiles, (uint32_t)nq, sk->layout.steps, dim, s.q_stat, nullptr));
    // behind each shard's list: the drop bound's slot, the first k eligible rows that fall into the shard, its
    // eligible rows without a usable sketch -- the same for every query (one mask)
    const uint64_t *mw = mask ? mask_host_words(mask) : nullptr;
    for (size_t i = 0; i < n_sh; i++) {
        const Shard *a = ix->shards[i];
        if (a->n_rows == 0) continue;
        uint64_t *o = s.h_cand + cand_off[i];
        for (int e = 0; e < kp + extra[i]; e++) o[e] = szg::kInvalidCand;
        uint64_t *x = o + kp + 1;
        rows_in_shard(a, firstk, x);  // (the rest of the k slots stay kInvalidCand)
        size_t n = (size_t)k;
        sketchless_rows(ix, a, mw, [&](uint64_t l, bool ok) { x[n++] = ok ? l : szg::kInvalidCand; });
    }
    for (int j = 1; j < nq; j++) memcpy(s.h_cand + (size_t)j * stride, s.h_cand, sizeof(uint64_t) * stride);
    HIPCHK(hipMemcpyAsync(s.cand, s.h_cand, sizeof(uint64_t) * stride * nq, hipMemcpyHostToDevice, nullptr));
    for (size_t i = 0; i < n_sh; i++) {
        const Shard *a = ix->shards[i], *h = sk->shards[i];
        if (h->n_rows == 0) continue;
        const szg::JoinPlan jp = szg::join_plan(dim, nq, kp, masked, h->cu_count, h->n_rows);
        szg::JoinArgs ja{};
        ja.rows = h->rows;
        ja.n_rows = (uint32_t)h->n_rows;
        ja.steps = sk->layout.steps;
        ja.dim = dim;
        ja.qtiles = s.qtiles;
        ja.n_queries = (uint32_t)nq;
        ja.row_stat = s.row_stat + stat_off[i];
        ja.q_stat = s.q_stat;
        ja.live = masked && h->has_dead ? h->live_bits.data() : nullptr;
        ja.allow = mask ? mask_shard_words(mask, i) : nullptr;
        if (masked && !ja.live && !ja.allow) ja.live = h->live_bits.data();  // (another shard's tombstones: one form per call)
        ja.query_blocks = (uint32_t)jp.query_blocks;
        ja.slices = (uint32_t)jp.slices;
        ja.tiles_per_slice = (uint32_t)jp.tiles_per_slice;
        ja.m = jp.m;
        ja.lists = s.lists;
        hipError_t e = szg::launch_join(sk->metric, ja, jp, nullptr);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "szg::launch_join", e);
        // (one merge and one re-rank per shard: the records are query-major, `stride` entries apart, so each query's
        // part is launched on its own view -- out_stride and n_cands_max are the shard's, the base moves with the query)
        const int st = kp + extra[i];
        if (n_sh == 1) {
            e = szg::launch_merge_short(s.lists, jp.slices, jp.m, kp, nq, s.cand, st, nullptr);
            if (e == hipSuccess)
                e = szg::launch_rerank(ix->bits, ix->metric, a->rows, ix->layout, dim, s.q64, s.cand, nullptr, (uint32_t)st, nq, s.out, nullptr);
        } else {
            for (int j = 0; j < nq && e == hipSuccess; j++) {
                uint64_t *cj = s.cand + (size_t)j * stride + cand_off[i];
                e = szg::launch_merge_short(s.lists + (size_t)j * jp.slices * jp.m, jp.slices, jp.m, kp, 1, cj, st, nullptr);
                if (e == hipSuccess)
                    e = szg::launch_rerank(ix->bits, ix->metric, a->rows, ix->layout, dim, s.q64 + (size_t)j * dim, cj, nullptr,
                                           (uint32_t)st, 1, s.out + (size_t)j * stride + cand_off[i], nullptr);
            }
        }
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "join merge / re-rank", e);
        launches++;
        bytes += (uint64_t)jp.query_blocks * h->n_rows * (uint64_t)dim;
    }
    HIPCHK(hipMemcpyAsync(s.h_out, s.out, sizeof(szg::RerankOut) * stride * nq, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    for (int j = 0; j < nq; j++) settle(q0 + j, s.h_out + (size_t)pos[j] * stride);
    return SZG_OK;
}

// one query: its answer, or a hand-over to the parent's route (SketchCall::settle with the join's key bound and 2 A)
void JoinCall::settle(int qi, const szg::RerankOut *rec)
{
    const size_t n_sh = ix->shards.size();
    cands.clear();
    double lb = INFINITY;
    bool nan_first = false;
    std::vector<szg_cert_entry> traced;
    // a query row without a usable sketch (no direction -- a zero query under cosine -- or a non-finite element)
    bool ok = !std::binary_search(ix->sk_exc.begin(), ix->sk_exc.end(), qrows[qi]);
    for (size_t i = 0; i < n_sh && ok; i++) {
        const Shard *a = ix->shards[i];
        if (a->n_rows == 0) continue;
        const szg::RerankOut *o = rec + cand_off[i];
        int valid = 0;
        float worst = -INFINITY;
        for (int e = 0; e < kp; e++) {
            if (o[e].row == 0xFFFFFFFFu) continue;
            valid++;
            const float key = szg::key_from_ordered(o[e].ukey);
            worst = std::max(worst, key);
            const double ub = (double)key + join_key_eps(ix->metric, key);
            cands.push_back(Cand{a->first + o[e].row, o[e].dist, key, ub});
            if (tracing) traced.push_back(szg_cert_entry{a->first + o[e].row, o[e].dist, ub, key, 0u});
        }
        if (valid == kp) lb = std::min(lb, (double)worst - join_key_eps(ix->metric, worst));
        if (o[kp].row != 0xFFFFFFFFu) {  // the drop bound: every row a block did not output is at or above it
            const float key = szg::key_from_ordered(o[kp].ukey);
            lb = std::min(lb, (double)key - join_key_eps(ix->metric, key));
        }
        for (int e = kp + 1; e < kp + extra[i]; e++) {
            if (o[e].row == 0xFFFFFFFFu) continue;
            if (std::isnan(o[e].dist) && e < kp + 1 + k) nan_first = true;
            cands.push_back(Cand{a->first + o[e].row, o[e].dist, 0.0f, 0.0});
            if (tracing) traced.push_back(szg_cert_entry{a->first + o[e].row, o[e].dist, 0.0, 0.0f, SZG_CERT_ENTRY_NO_KEY});
        }
    }
    cands.erase(std::remove_if(cands.begin(), cands.end(), [](const Cand &c) { return std::isnan(c.dist); }), cands.end());
    unique_rows(cands);
    replay_topk(cands, k, &res);
    ok = ok && (!nan_first || ix->tie_mode != 0);
    double D_used = NAN;
    if (ok && lb < INFINITY) {
        D_used = sketch_dist_below(p.gs, lb);
        ok = (int)res.size() == k && sketch_settles(res.back().priority, D_used, 2.0 * p.slack);
    }
    if (ok && ix->tie_mode == 0) {
        dd.clear();
        for (const Cand &c : cands) dd.push_back(c.dist);
        if (history_dependent(dd.data(), dd.size(), k)) ok = false;
    }
    if (tracing) {
        szg_cert_record r = cert_record(ix, qi, SZG_CERT_JOIN);
        r.keys = SZG_CERT_KEYS_SINGLE;
        r.sweep = 0;
        r.certified = ok ? 1 : 0;
        r.k = k;
        r.thr_min = lb;
        r.D = D_used;
        r.slack = 2.0 * p.slack;
        cert_emit(ix, r, traced);
    }
    if (!ok) {
        redo.push_back(qi);
        return;
    }
    emit_topk(ix, res, k, qi, out_rows, out_dist, out_count);
}

// The parent's route for queries sel[0, n) of the call (null: all of them): decode on the card into the handle's
// conversion buffer, one copy to its pinned twin, ONE masked search; chunks only where the float64 batch would pass 1 GiB.
int route_rows(szg_index *ix, const uint64_t *qrows, const int *sel, int n, int k, const szg_mask *mask, uint64_t *out_rows,
               double *out_dist, int32_t *out_count)
{
    const size_t dim = (size_t)ix->dim;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, (1ull << 27) / dim));
    std::vector<uint64_t> r2;
    std::vector<double> d2;
    std::vector<int32_t> c2;
    std::vector<uint64_t> list;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = std::min(chunk, n - c0);
        std::unique_lock<std::mutex> lock(ix->dq_mu);
        if (int rc = ix->dq_host.ensure((size_t)m * dim, "hipHostMalloc(device queries)")) return rc;
        // per device: the rows its shards hold, decoded back to back, then moved to their places in the batch
        std::vector<int> devices;
        for (const Shard *sh : ix->shards)
            if (sh->n_rows && std::find(devices.begin(), devices.end(), sh->device) == devices.end()) devices.push_back(sh->device);
        std::vector<double> part;
        for (int device : devices) {
            std::vector<int> at;
            list.clear();
            for (int j = 0; j < m; j++) {
                const uint64_t r = qrows[sel ? sel[c0 + j] : c0 + j];
                uint64_t local = 0;
                if (shard_of(ix, r, &local)->device != device) continue;
                at.push_back(j);
                list.push_back(r);
            }
            if (list.empty()) continue;
            const size_t elems = list.size() * dim;
            if (ix->dq_dev.device() != device) ix->dq_dev = DevMem<double>(device);
            if (int rc = ix->dq_dev.ensure(elems + list.size(), "hipMalloc(device queries)")) return rc;
            uint64_t *d_list = reinterpret_cast<uint64_t *>(ix->dq_dev.data() + elems);
            HIPCHK(hipMemcpy(d_list, list.data(), list.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
            for (const Shard *sh : ix->shards)
                if (sh->n_rows && sh->device == device)
                    HIPCHK(szg::launch_fetch(ix->bits, sh->rows, ix->layout, ix->dim, list.size(), d_list, sh->first, sh->n_rows, 0,
                                             ix->dq_dev.data(), 0, (uint64_t)dim, nullptr));
            if (devices.size() == 1) {  // (every row: the batch is in order already)
                HIPCHK(hipMemcpy(ix->dq_host.data(), ix->dq_dev.data(), elems * sizeof(double), hipMemcpyDeviceToHost));
                continue;
            }
            part.resize(elems);
            HIPCHK(hipMemcpy(part.data(), ix->dq_dev.data(), elems * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < at.size(); i++) memcpy(ix->dq_host.data() + (size_t)at[i] * dim, &part[i * dim], dim * sizeof(double));
        }
        const szg_mask *const *masks = mask ? &mask : nullptr;
        if (!sel) {
            const int rc = szg_search_topk_masked(ix, ix->dq_host.data(), m, k, masks, mask ? 1 : 0, out_rows + (size_t)c0 * k,
                                                  out_dist + (size_t)c0 * k, out_count ? out_count + c0 : nullptr);
            if (rc) return rc;
            continue;
        }
        r2.resize((size_t)m * k), d2.resize((size_t)m * k), c2.resize(m);
        const int rc = szg_search_topk_masked(ix, ix->dq_host.data(), m, k, masks, mask ? 1 : 0, r2.data(), d2.data(), c2.data());
        if (rc) return rc;
        for (int j = 0; j < m; j++) {
            const size_t q = (size_t)sel[c0 + j];
            memcpy(out_rows + q * k, &r2[(size_t)j * k], sizeof(uint64_t) * k);
            memcpy(out_dist + q * k, &d2[(size_t)j * k], sizeof(double) * k);
            if (out_count) out_count[q] = c2[j];
        }
    }
    return SZG_OK;
}

// does the join serve the call?  (the sketch in sync)
bool join_serves(const szg_index *ix, int n_queries, int k)
{
    const szg_index *sk = ix->sketch;
    if (!sk || ix->sk_disabled || ix->sk_nomem || n_queries < ix->join_min) return false;
    if (!sk->layout.tiled || (int)sk->layout.steps * 64 != ix->dim) return false;
    const int kk = k + ix->sketch_extra, kp = kk + std::max(ix->slack_min, kk / 2);
    bool any = false;
    for (const Shard *h : sk->shards) {
        if (h->device != sk->shards[0]->device) return false;
        if (h->n_rows == 0) continue;
        any = true;
        if (!szg::join_plan(ix->dim, std::min(n_queries, szg::kJoinBatch), kp, 0, h->cu_count, h->n_rows).served) return false;
    }
    return any;
}

}  // namespace

}  // namespace szgi

using szgi::fail;

extern "C" {

int szg_index_neighbors(szg_index *ix, const uint64_t *rows, uint64_t first_row, uint64_t n_queries, int k, const szg_mask *mask,
                        uint64_t *out_rows, double *out_dist, int32_t *out_count)
{
    SZG_TRY
    using namespace szgi;
    if (!ix || !out_rows || !out_dist) return fail(SZG_E_INVALID, "null argument");
    if (k <= 0) return fail(SZG_E_INVALID, "k must be > 0 (K==0 is listing mode, collection.go:633)");
    if (n_queries > (uint64_t)INT32_MAX) return fail(SZG_E_INVALID, "too many queries for one call");
    if (mask)
        if (int rc = mask_check(ix, mask)) return rc;
    const uint64_t total = szg_index_rows(ix), base = ix->row_base;
    std::vector<uint64_t> q((size_t)n_queries);
    if (rows) {
        for (uint64_t i = 0; i < n_queries; i++) {
            if (rows[i] < base || rows[i] - base >= total) return fail(SZG_E_RANGE, "row out of bounds");
            q[i] = rows[i] - base;
        }
    } else {
        if (first_row < base || first_row - base > total || n_queries > total - (first_row - base))
            return fail(SZG_E_RANGE, "row range out of bounds");
        for (uint64_t i = 0; i < n_queries; i++) q[i] = first_row - base + i;
    }
    if (n_queries == 0) return SZG_OK;
    const int n = (int)n_queries;
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->nb.queries += n_queries;
    }
    bool served = n >= ix->join_min && sketch_applies(ix, k);
    if (served) {
        if (int rc = sketch_sync_for_search(ix)) return rc;
        served = join_serves(ix, n, k);
    }
    if (!served) return route_rows(ix, q.data(), nullptr, n, k, mask, out_rows, out_dist, out_count);
    JoinCall call{ix, ix->sketch, q.data(), n, k, mask, out_rows, out_dist, out_count};
    {
        std::lock_guard<std::mutex> lk(ix->join_mu);
        if (int rc = call.run()) return rc;
    }
    if (call.redo.empty()) return SZG_OK;
    std::sort(call.redo.begin(), call.redo.end());
    return route_rows(ix, q.data(), call.redo.data(), (int)call.redo.size(), k, mask, out_rows, out_dist, out_count);
    SZG_CATCH
}

int szg_index_neighbors_stats(szg_index *ix, szg_neighbors_stats *out)
{
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    *out = ix->nb;
    return SZG_OK;
}

// test and measurement hook: calls of at least min_queries queries on the handle try the join (0: the default again)
int szg_debug_join_min_queries(szg_index *ix, int min_queries)
{
    if (!ix || min_queries < 0) return fail(SZG_E_INVALID, "null handle or a negative count");
    ix->join_min = min_queries == 0 ? szg::kJoinMinQueries : min_queries;
    return SZG_OK;
}

// host only: join_plan for one launch on a shard of that shape
int szg_debug_join_plan(int dim, int n_queries, int kp, int masked, int cu_count, uint64_t shard_rows, szg_join_plan *out)
{
    if (!out) return fail(SZG_E_INVALID, "null argument");
    memset(out, 0, sizeof(*out));
    const szg::JoinPlan p = szg::join_plan(dim, n_queries, kp, masked, cu_count ? cu_count : 256, shard_rows);
    out->served = p.served;
    if (!p.served) return SZG_OK;
    out->qb = p.qb;
    out->areg = p.areg;
    out->masked = p.masked;
    out->query_blocks = p.query_blocks;
    out->slices = p.slices;
    out->tiles_per_slice = p.tiles_per_slice;
    out->m = p.m;
    out->lds_bytes = p.lds_bytes;
    out->min_queries = szg::kJoinMinQueries;
    return SZG_OK;
}

}  // extern "C"
