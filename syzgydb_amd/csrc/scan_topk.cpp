// scan_topk.cpp -- the batch pipeline of search calls (scan_internal.h) and the one-sweep-per-query top-k pipeline:
// enqueue, certification, escalation, exact replay.
#include "scan_internal.h"

namespace szgi {

LaunchGeom scan_geometry(int bits, const szg::RowMap &map, uint32_t row_bytes, bool tiled, uint64_t n_rows, int cu_count,
                         int kp)
{
    int block = szg_index::block_threads;
    // keep query + per-wave lists within 64 KiB of LDS
    while (block > 64 && szg::scan_lds_bytes(bits, map, kp, block) > 64u * 1024u) block >>= 1;
    const int nwaves = block / 64;
    const uint64_t rows_per_block = (uint64_t)nwaves * map.gpw;
    uint64_t need = (n_rows + rows_per_block - 1) / rows_per_block;
    int waves_per_cu = szg_index::blocks_per_cu * nwaves;
    if (szg_index::blocks_per_cu <= 0) {
        // Measured on MI355X (scripts/dev_bpc.sh, scripts/readbw): HBM streams fastest with
        // 6-8 MB of reads in flight; more requests only lengthen the DRAM queues.  8 waves
        // per CU for float rows of >= 1 KB and for LDS-resident candidate lists (kp > 64);
        // the integer / 16-bit decodes and short rows need 12 to hide their ALU work.
        // (4 waves per CU is another 0.5 % faster on 3 KB rows at 1M rows but 10 % slower
        // on a 125 K-row shard, where the sweep's ramp-up and tail weigh more.)
        // Collect sweeps (kp == 0: radius search, escalation) keep no lists; on short 4-bit rows (cfg5's 192 bytes)
        // they stream best with 8 (same-box A/B, scripts/ab_opts.sh: 6.2-6.7 -> 6.85-6.91 TB/s; top-k on the same rows
        // wants its 12: 6.8-6.9 against 6.5).
        const bool short_collect = kp == 0 && bits == 4 && row_bytes <= 256;
        if (kp > 64 || short_collect || (bits >= 32 && row_bytes >= 1024) || (bits == 8 && tiled))
            waves_per_cu = 8;
        else
            waves_per_cu = 12;
    }
    uint64_t grid = (uint64_t)cu_count * (uint64_t)std::max(1, waves_per_cu / nwaves);
    if (need < grid) grid = need;
    if (grid < 1) grid = 1;
    return LaunchGeom{(int)grid, block, (int)rows_per_block};
}

LaunchGeom scan_geometry(const szg_index *ix, const Shard *sh, int kp)
{
    return scan_geometry(ix->bits, ix->map, ix->row_bytes, ix->layout.tiled != 0, sh->n_rows, sh->cu_count, kp);
}

size_t shard_words(const Shard *sh) { return (size_t)((sh->n_rows + 63) / 64); }

// ---- option query_prep: a batch's queries prepared on the card (scan_internal.h) ----------------------------------------
int enqueue_query_prep(szg_index *ix, Ctx *c, int nq, double gs)
{
    if (ix->bits != 8 || nq < 1 || nq > kMaxBatch) return fail(SZG_E_INVALID, "query_prep: an 8-bit index's batch");
    int rc = c->d_meta.ensure((size_t)kMaxBatch * szg::kQueryPrepMeta);
    if (rc == SZG_OK) rc = c->h_meta.ensure((size_t)kMaxBatch * szg::kQueryPrepMeta);
    if (rc) return rc;
    HIPCHK(szg::launch_query_prep(c->d_q64, nq, ix->dim, gs, ix->metric == SZG_COSINE ? 1 : 0, scan_planes(ix), ix->map.r16,
                                  (uint32_t)ix->qsw_bytes, c->d_qsw, c->d_meta, c->pass.work));
    c->pass.prep_n = nq;
    c->pass.prep_taken = false;
    return SZG_OK;
}

int enqueue_card_meta_copy(Ctx *c)
{
    HIPCHK(hipMemcpyAsync(c->h_meta, c->d_meta, sizeof(double) * szg::kQueryPrepMeta * (size_t)c->pass.prep_n,
                          hipMemcpyDeviceToHost, c->pass.work));
    return SZG_OK;
}

void take_card_meta(Ctx *c)
{
    if (!c->pass.prep_n || c->pass.prep_taken) return;
    for (int j = 0; j < c->pass.prep_n; j++) {
        const double *m = c->h_meta + (size_t)j * szg::kQueryPrepMeta;
        QMeta &o = c->meta[j];
        o = QMeta{};
        o.qnorm = m[szg::kQpQnorm];
        o.m1 = m[szg::kQpM1];
        o.qscale = m[szg::kQpQscale];
        o.qconst = m[szg::kQpQconst];
        o.qnorm2 = m[szg::kQpQnorm2];
    }
    c->pass.prep_taken = true;
}

// Enqueue H2D of nq prepared queries (+ their masks) on the ctx stream.
// masks: nullptr (no query of the batch is filtered), or nq pointers to index-level masks
// ((total_rows + 63) / 64 words each); a null entry allows every row.
// The masks reach the sweeps by one of three routes (Pass::allow_base / allow_stride say where they are):
//   every query holds the SAME resident mask   its shard words are read in place, stride 0, nothing is copied
//   resident masks that differ, or some null   one mask_gather launch fills the batch's d_allow slots card-to-card
//   words from the host                        staged in pinned memory and uploaded, as before
int enqueue_queries(szg_index *ix, Shard *sh, Ctx *c, const double *q, int nq, const uint64_t *const *masks,
                    bool with_single_form, const szg_mask *const *handles, size_t shard_no, const double *card_prep)
{
    HIPCHK(hipSetDevice(sh->device));
    memcpy(c->h_q64, q, sizeof(double) * ix->dim * nq);
    if (ix->timing >= 2) {
        SiteScope t_(10);
        HIPCHK(hipEventRecord(c->ev_all0, c->pass.work));
    }
    {
        SiteScope t_(0);
        if (with_single_form)
            HIPCHK(hipMemcpyAsync(c->d_qsw, c->h_qsw, ix->qsw_bytes * nq, hipMemcpyHostToDevice, c->pass.work));
        HIPCHK(hipMemcpyAsync(c->d_q64, c->h_q64, sizeof(double) * ix->dim * nq, hipMemcpyHostToDevice,
                              c->pass.work));
    }
    if (card_prep) {  // (the sweeps wait for ev_up below: the images and the constants they read are there by then)
        if (with_single_form) return fail(SZG_E_INVALID, "query_prep: the batch's images come from one side");
        int rc = enqueue_query_prep(ix, c, nq, *card_prep);
        if (rc) return rc;
    }
    if (masks && handles) {
        bool same = handles[0] != nullptr;
        for (int i = 1; i < nq && same; i++) same = handles[i] == handles[0];
        for (int i = 0; i < nq; i++)
            c->mask_count[i] = handles[i] ? (int64_t)mask_shard_count(handles[i], shard_no) : (int64_t)sh->n_rows;
        if (same) {
            c->pass.allow_base = mask_shard_words(handles[0], shard_no);
            c->pass.allow_stride = 0;
            ix->mask_shared++;
        } else {
            const size_t slot = mask_slot_words(sh);
            int rc = c->d_allow.ensure(slot * nq);
            if (rc) return rc;
            szg::MaskGatherTable t{};
            for (int i = 0; i < nq; i++) t.src[i] = handles[i] ? mask_shard_words(handles[i], shard_no) : nullptr;
            HIPCHK(szg::launch_mask_gather(t, nq, c->d_allow, slot / 2, c->pass.work));
            c->pass.allow_base = c->d_allow;
            c->pass.allow_stride = (uint32_t)slot;
            ix->mask_d2d += (uint64_t)slot * nq * sizeof(uint64_t);
        }
    } else if (masks) {
        const size_t words = shard_words(sh);
        int rc = c->d_allow.ensure(words * nq);
        if (rc) return rc;
        c->pass.allow_base = c->d_allow;
        c->pass.allow_stride = (uint32_t)words;
        ix->mask_h2d += (uint64_t)words * nq * sizeof(uint64_t);
        std::fill(c->mask_count, c->mask_count + nq, (int64_t)-1);
        rc = c->h_allow.ensure(words * nq);
        if (rc) return rc;
        for (int i = 0; i < nq; i++) {
            if (masks[i])
                memcpy(c->h_allow + (size_t)i * words, masks[i] + sh->first / 64, words * sizeof(uint64_t));
            else
                memset(c->h_allow + (size_t)i * words, 0xFF, words * sizeof(uint64_t));
        }
        HIPCHK(hipMemcpyAsync(c->d_allow, c->h_allow, words * nq * sizeof(uint64_t),
                              hipMemcpyHostToDevice, c->pass.work));
    }
    // what the sweeps wait for ends here: work enqueued on this stream afterwards (the first-k
    // rows' distances) runs beside the sweeps
    HIPCHK(hipEventRecord(c->ev_up, c->pass.work));
    if (card_prep) return enqueue_card_meta_copy(c);  // (the host needs them when it settles: beside the sweeps)
    return SZG_OK;
}

// scan arguments for queries [slot, slot+nq) of the ctx's staged batch
void fill_scan_args(const szg_index *ix, const Shard *sh, const Ctx *c, bool has_allow, int slot,
                    int nq, szg::ScanArgs *a)
{
    memset(a, 0, sizeof(*a));
    a->rows = sh->rows;
    a->n_rows = (uint32_t)sh->n_rows;
    a->pitch = ix->pitch;
    a->tiled = ix->layout.tiled;
    a->steps = ix->layout.steps;
    a->dim = ix->dim;
    a->map = ix->map;
    a->live_bits = sh->has_dead ? sh->live_bits : nullptr;
    a->allow_stride = c->pass.allow_stride;
    a->allow_bits = has_allow ? c->pass.allow_base + (size_t)slot * a->allow_stride : nullptr;
    a->query_stride = (uint32_t)ix->qsw_bytes;
    a->query = c->d_qsw + (size_t)slot * ix->qsw_bytes;
    a->n_queries = nq;
    // (prepared on the card: the kernels read the constants where the card wrote them, the arrays stay zero)
    if (c->pass.prep_n) a->qmeta = c->d_meta + (size_t)slot * szg::kQueryPrepMeta;
    for (int j = 0; j < nq && j < szg::kMatrixWideQueries && !c->pass.prep_n; j++) {
        a->qscale[j] = (float)c->meta[slot + j].qscale;
        a->qconst[j] = (float)c->meta[slot + j].qconst;
        a->qnorm2[j] = (float)c->meta[slot + j].qnorm2;
    }
    a->norm_bias = ix->norm_bias;
    a->no_shape_kernels = ix->shape_kernels ? 0 : 1;
    a->ring = ix->ring;
    a->group = ix->scan_group;
    a->group_ring = ix->scan_group_ring;
    a->planes = scan_planes(ix);  // (as prep_query quantized the staged queries)
    a->matrix = ix->sketch_matrix;
    a->select = ix->sketch_select;
    a->wide = ix->sketch_wide;
    a->bulk = ix->sketch_bulk;
}

// Masked sweeps: when most rows pass (a few tombstones, a mild filter) every row is read and the masks decide at the
// row finish -- the predicate-free dense phase; a selective filter keeps the form that tests a row before issuing its
// loads.  The launch's queries [slot, slot+nq) vote: the lowest pass rate decides.
static int mask_dense_vote(const szg_index *ix, const Shard *sh, const Ctx *c, bool has_allow, int slot, int nq)
{
    if (!(has_allow || sh->has_dead) || !ix->mask_dense) return 0;
    double lowest = 1.0;
    for (int j = slot; j < slot + nq; j++) lowest = std::min(lowest, mask_pass_rate(sh, c, has_allow, j));
    return lowest >= 0.5 ? 1 : 0;
}

void fill_collect_args(const szg_index *ix, const Shard *sh, const Ctx *c, bool has_allow, int slot, int nq, const float *thr,
                       uint64_t *buf, size_t cap, uint32_t *count, bool dense_vote, szg::ScanArgs *a)
{
    fill_scan_args(ix, sh, c, has_allow, slot, nq, a);
    a->collect = 1;
    for (int j = 0; j < nq; j++) szg::scan_thr_ukey(*a, j) = szg::ordered_key(thr[j]);
    a->collect_buf = buf;
    a->collect_cap = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu);
    a->collect_count = count;
    if (dense_vote) a->mask_dense = mask_dense_vote(ix, sh, c, has_allow, slot, nq);
}

// Launch the fused scan for each of the batch's queries (n = a->size()) as the
// next links of the shard's scan chain; the ctx stream resumes after the last.
int launch_scans_chained(szg_index *ix, Shard *sh, Ctx *c, const std::vector<szg::ScanArgs> &a,
                         const LaunchGeom &g, hipStream_t after, int part, const std::vector<szg::ScanShareHi> *hi)
{
    const int n = (int)a.size();
    if (hi && (int)hi->size() != n) return fail(SZG_E_INVALID, "shared launches: one record per launch");
    auto shared = [&](int j) { return hi && a[j].n_queries > szg::kMatrixWideQueries; };
    // launches with masks that take a masked form of the matrix sweep (option sketch_masked; szg::launch_scan_masked)
    std::vector<char> mxm(n, 0);
    for (int j = 0; j < n; j++) mxm[j] = scan_takes_masked_form(ix, a[j], g.block) ? 1 : 0;
    szg::ScanShareHi no_hi;
    memset(&no_hi, 0, sizeof(no_hi));
    no_hi.share = ix->sketch_share;
    // (ev_up: recorded by enqueue_queries)
    int rc = chain_sweeps(ix, sh, c, after ? after : c->pass.work, part, n, "szg::launch_scan", [&](hipStream_t st) {
        hipError_t e = hipSuccess;
        for (int j = 0; j < n && e == hipSuccess; j++)
            e = mxm[j] ? szg::launch_scan_masked(ix->bits, ix->metric, a[j], hi ? (*hi)[j] : no_hi, ix->sketch_masked, g.grid,
                                                 g.block, st)
                       : (shared(j) ? szg::launch_scan_share(ix->bits, ix->metric, a[j], (*hi)[j], g.grid, g.block, st)
                                    : szg::launch_scan(ix->bits, ix->metric, a[j], g.grid, g.block, st));
        return e;
    });
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    uint64_t sweeps = 0;  // passes over the rows (launch_passes), of the variant the launcher above took
    for (int j = 0; j < n; j++) {
        sweeps += (uint64_t)launch_passes(mxm[j] ? szg::scan_masked_plan_in(ix->bits, a[j], ix->sketch_share, ix->sketch_masked, g.block)
                                          : (shared(j) ? szg::scan_share_plan_in(ix->bits, a[j], (*hi)[j], g.block)
                                                       : szg::scan_plan_in(ix->bits, a[j], g.block)));
        if (mxm[j]) {
            ix->mx_masked_launches++;
            ix->mx_masked_queries += (uint64_t)a[j].n_queries;
            if (!a[j].allow_bits || a[j].allow_stride == 0) ix->mx_masked_skip++;
        }
    }
    ix->stats.scan_launches += n;
    ix->stats.scan_bytes += sweeps * sh->n_rows * (uint64_t)ix->row_bytes;
    return SZG_OK;
}

bool scan_takes_masked_form(const szg_index *ix, const szg::ScanArgs &a, int block)
{
    // (the sketch index's top-k launches: plain 8-bit handles and collect launches stay as they are)
    if (ix->sketch_masked != 1 || !ix->is_sketch || ix->bits != 8 || a.collect || !szg::scan_masked(a) || !a.row_norm) return false;
    const szg::ScanVariant v = szg::scan_variant(szg::scan_masked_plan_in(ix->bits, a, ix->sketch_share, ix->sketch_masked, block));
    return v.matrix != 0 && v.masked != 0;
}

// A resident mask knows its exact count; the pass rate of words that came from the host is estimated from a sample.
double mask_pass_rate(const Shard *sh, const Ctx *c, bool has_allow, int slot)
{
    const double live = sh->n_rows ? (double)sh->n_live / (double)sh->n_rows : 1.0;
    if (!has_allow) return live;
    if (c->mask_count[slot] >= 0) return live * (double)c->mask_count[slot] / (double)sh->n_rows;
    const size_t words = shard_words(sh);
    const uint64_t *m = c->h_allow + (size_t)slot * words;
    const size_t step = std::max<size_t>(1, words / 256);
    uint64_t ones = 0, seen = 0;
    for (size_t w = 0; w < words; w += step) {
        ones += (uint64_t)__builtin_popcountll(m[w]);
        seen += 64;
    }
    return live * (seen ? (double)ones / (double)seen : 1.0);
}

SketchShape sketch_shape(const szg_index *ix, const szg_index *sk)
{
    SketchShape s{};
    s.bits = sk->bits;
    s.map = sk->map;
    s.tiled = sk->layout.tiled != 0;
    s.ring = sk->ring;
    s.no_shape_kernels = !sk->shape_kernels;
    s.scan_group = sk->scan_group;
    s.planes = scan_planes(sk);
    s.scan_group_ring = sk->scan_group_ring;
    s.sketch_matrix = sk->sketch_matrix;
    s.sketch_select = sk->sketch_select;
    s.sketch_wide = sk->sketch_wide;
    s.sketch_share = sk->sketch_share;
    s.sketch_masked = sk->sketch_masked;
    s.sketch_list = ix->sketch_list;
    s.query_batch = ix->query_batch;
    s.queries_per_launch = sk->queries_per_launch;
    s.norms = true;
    return s;
}

bool sketch_wide_serves(const szg_index *sk, const Shard *sh, int kp, int list_opt)
{
    SketchShape s = sketch_shape(sk, sk);
    s.sketch_list = list_opt;
    const LaunchGeom g = scan_geometry(sk, sh, kp);
    return sketch_wide_serves(s, g.grid, g.block, sh->has_dead, kp);
}

bool sketch_share_serves(const szg_index *sk, const Shard *sh, int kp, int list_opt)
{
    SketchShape s = sketch_shape(sk, sk);
    s.sketch_list = list_opt;
    const LaunchGeom g = scan_geometry(sk, sh, kp);
    return sketch_share_serves(s, g.grid, g.block, sh->has_dead, kp);
}

// top-k pass for the nq staged queries of one shard: scan -> merges -> rerank -> D2H (async)
// on (the sketch pre-pass): sh is a sketch shard; the last merge writes each query's list in front of the extra rows
// staged in c->d_sent, and ONE rerank on on->sh's rows takes both.  Its sweeps keep lists of m < kp entries per wave
// and block where they can; ONE merge launch per part then selects the kp best and writes the drop bound to entry kp
// (a candidate like the others: the rerank returns its key).
int enqueue_topk(szg_index *ix, Shard *sh, Ctx *c, int kp, int nq, bool has_allow, const RerankOn *on)
{
    const int stride = kp + (on ? on->extra : 0);  // entries per query in d_out / h_out
    c->pass.kp = kp;
    c->pass.out_stride = stride;
    c->pass.keys = ListKeys::Single;
    HIPCHK(hipSetDevice(sh->device));
    // the batch's launches on this shard (sketch_plan.h): parts, forms, queries per launch, grid and lists
    LaunchGeom g = scan_geometry(ix, sh, kp);
    const SketchLaunches L = sketch_batch_launches(sketch_shape(on ? on->ix : ix, ix), on != nullptr, g.grid, g.block, kp, nq,
                                                   c->pass.early_n, has_allow || sh->has_dead, on && on->wide, on && on->share);
    const bool share = L.share;
    const int lists0 = L.lists0, m = L.m, qpl = L.qpl;
    g.grid = L.grid;
    if (on && on->extra < 1) return fail(SZG_E_INVALID, "sketch: no slot for the drop bound");
    int rc = c->ensure_lists((size_t)nq * lists0 * m);
    if (rc == SZG_OK) rc = c->d_out.ensure((size_t)nq * stride);
    if (rc == SZG_OK) rc = c->h_out.ensure((size_t)nq * stride);
    if (rc) return rc;
    if (on && c->d_sent.capacity() < (size_t)nq * stride) return fail(SZG_E_INVALID, "sketch candidates not staged");

    for (int part = L.first_part(); part >= 0; part--) {
        const int q0 = L.q0(part), q1 = L.q1(part), nqp = q1 - q0;
        hipStream_t tl = part ? c->stream : c->pass.work;
        std::vector<szg::ScanArgs> args(L.n_launches(part));
        std::vector<szg::ScanShareHi> hi(share ? args.size() : 0);
        for (int j = q0; j < q1; j += qpl) {  // one sweep per query, results side by side
            szg::ScanArgs &a = args[(j - q0) / qpl];
            fill_scan_args(ix, sh, c, has_allow, j, L.count(part, j), &a);
            a.mask_dense = mask_dense_vote(ix, sh, c, has_allow, j, a.n_queries);
            a.kp = m;
            a.matrix = L.matrix;
            a.block_lists = c->d_lists_a + (size_t)j * lists0 * m;
            if (share) {  // the constants of the launch's queries 32 .. 63, and the option
                szg::ScanShareHi &h = hi[(j - q0) / qpl];
                memset(&h, 0, sizeof(h));
                for (int x = szg::kMatrixWideQueries; x < a.n_queries && !c->pass.prep_n; x++) {
                    h.qscale[x - szg::kMatrixWideQueries] = (float)c->meta[j + x].qscale;
                    h.qconst[x - szg::kMatrixWideQueries] = (float)c->meta[j + x].qconst;
                    h.qnorm2[x - szg::kMatrixWideQueries] = (float)c->meta[j + x].qnorm2;
                }
                h.share = ix->sketch_share;
            }
        }
        // launches that score groups of queries per row read -- the grouped kernels and the matrix sweep, which cannot do
        // without -- take the rows' norms from the resident array (complete before the sweeps are enqueued; it only has
        // work to do after rows were added)
        const float *norms = nullptr;
        bool asked = false;
        for (szg::ScanArgs &a : args) {
            bool wants = szg::scan_wants_norms(ix->bits, a, g.block);
            if (!wants && ix->sketch_masked == 1 && szg::scan_masked(a)) {  // (a masked form of the matrix sweep reads them too)
                szg::ScanPlanIn in = szg::scan_masked_plan_in(ix->bits, a, ix->sketch_share, ix->sketch_masked, g.block);
                in.norms = true;
                wants = szg::scan_variant(in).matrix != 0;
            }
            if (!wants) continue;
            if (!asked) {
                int nrc = SZG_OK;
                norms = scan_row_norms(ix, sh, &nrc);
                if (nrc) return nrc;
            }
            asked = true;
            a.row_norm = norms;
        }
        rc = launch_scans_chained(ix, sh, c, args, g, tl, part, share ? &hi : nullptr);
        if (rc) return rc;

        int n_lists = lists0;
        uint64_t *src = c->d_lists_a + (size_t)q0 * lists0 * m, *dst = c->d_lists_b + (size_t)q0 * lists0 * m;
        const int fan = szg::merge_fan(kp);
        {
            SiteScope t_(6);
            if (m < kp) {
                uint64_t *cand = c->d_sent + (size_t)q0 * stride;
                HIPCHK(szg::launch_merge_short(src, n_lists, m, kp, nqp, cand, stride, tl));
                src = cand;
            }
            while (m == kp && (n_lists > 1 || on)) {
                if (on && (n_lists + fan - 1) / fan == 1) {  // (at least this one merge, even of a single list)
                    uint64_t *cand = c->d_sent + (size_t)q0 * stride;
                    HIPCHK(szg::launch_merge(src, n_lists, kp, nqp, cand, tl, stride));
                    src = cand;
                    break;
                }
                HIPCHK(szg::launch_merge(src, n_lists, kp, nqp, dst, tl));
                n_lists = (n_lists + fan - 1) / fan;
                std::swap(src, dst);
            }
        }
        {
            SiteScope t_(7);
            const szg_index *rx = on ? on->ix : ix;
            HIPCHK(szg::launch_rerank(rx->bits, rx->metric, on ? on->sh->rows : sh->rows, rx->layout, rx->dim,
                                      c->d_q64 + (size_t)q0 * ix->dim, src, nullptr, (uint32_t)stride, nqp,
                                      c->d_out + (size_t)q0 * stride, tl));
        }
        {
            SiteScope t_(8);
            HIPCHK(hipMemcpyAsync(c->h_out + (size_t)q0 * stride, c->d_out + (size_t)q0 * stride,
                                  sizeof(szg::RerankOut) * stride * nqp, hipMemcpyDeviceToHost, tl));
        }
    }
    if (ix->timing >= 2) {
        SiteScope t_(10);
        HIPCHK(hipEventRecord(c->ev_all1, c->pass.work));
    }
    return SZG_OK;
}

int finish_timing(szg_index *ix, Ctx *c)
{
    if (!ix->timing) return SZG_OK;
    Pass &p = c->pass;
    float ms_scan = 0, ms_all = 0, ms_part = 0;
    if (p.timed_n) HIPCHK(hipEventElapsedTime(&ms_scan, c->ev_scan0, c->ev_scan1));
    if (p.timed_part_n) HIPCHK(hipEventElapsedTime(&ms_part, c->ev_p0, c->ev_p1));  // the early part of a short call
    if (ix->timing >= 2) HIPCHK(hipEventElapsedTime(&ms_all, c->ev_all0, c->ev_all1));
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->stats.scan_ms += ms_scan + ms_part;
    ix->stats.timed_launches += p.timed_n + p.timed_part_n;
    ix->stats.total_ms += ms_all;
    p.timed_n = p.timed_part_n = 0;  // (consumed: an escalation or a rerun on this context records anew)
    return SZG_OK;
}

// ListKeys as the certificate trace names them (SZG_CERT_KEYS_*)
static int cert_keys(ListKeys k)
{
    switch (k) {
    case ListKeys::Single: return SZG_CERT_KEYS_SINGLE;
    case ListKeys::SharedInt8: return SZG_CERT_KEYS_SHARED_INT8;
    case ListKeys::SharedBf16: return SZG_CERT_KEYS_SHARED_BF16;
    case ListKeys::Bf16Band: return SZG_CERT_KEYS_BF16_BAND;
    case ListKeys::Bf16Rescored: return SZG_CERT_KEYS_BF16_RESCORED;
    }
    return -1;
}

// candidates of staged query `slot` from a finished top-k pass, each with the upper bound of its
// real-number key; *lb = a lower bound of the real-number key of every eligible row of the shard that
// is NOT among them (+inf if every eligible row is).  `m` = the query's constants with the flags
// of the path the ticket was prepared for; the shard's context says which arithmetic actually
// produced the keys (Pass::keys).  (The first Pass::kp entries of the query in h_out: more may ride behind them.)
void gather_topk(const szg_index *ix, const Shard *sh, const Ctx *c, const QMeta &m, int slot,
                 std::vector<Cand> *cands, double *lb)
{
    const int kp = c->pass.kp;
    QMeta lm = m;  // class of the list's keys
    bool thr_bound = false, band_bound = false;  // rows left out ahead of the lists, by their bfloat16 key
    switch (c->pass.keys) {
    case ListKeys::Single:
    case ListKeys::SharedInt8: break;  // (what the ticket was prepared for)
    case ListKeys::SharedBf16: lm.mq_bf16 = true; break;
    case ListKeys::Bf16Band: band_bound = true; [[fallthrough]];
    case ListKeys::Bf16Rescored:
        lm.mq_bf16 = false;
        thr_bound = true;
        break;
    }
    int valid = 0;
    float worst = -INFINITY;
    for (int i = 0; i < kp; i++) {
        const szg::RerankOut &r = c->out(slot, i);
        if (r.row == 0xFFFFFFFFu) continue;
        valid++;
        const float key = szg::key_from_ordered(r.ukey);
        worst = std::max(worst, key);
        double ub = (double)key + key_eps(ix, key, lm);
        // a row forced in (key -2: float32 norm under- or overflowed) carries no information in its key;
        // its float64 distance does: -cos(pi d) is the real-number key
        if (ix->metric == SZG_COSINE && key <= -1.5f && !std::isnan(r.dist)) ub = -std::cos(M_PI * r.dist) + 1e-9;
        cands->push_back(Cand{sh->first + r.row, r.dist, key, ub});
    }
    *lb = valid == kp ? (double)worst - key_eps(ix, worst, lm) : INFINITY;
    if (thr_bound) {
        // rows the bfloat16 sweep did not collect: bfloat16 key above the prefix threshold
        QMeta bm = m;
        bm.mq_bf16 = true;
        const float thr = c->h_thr[slot];
        if (thr < 3.0e38f) *lb = std::min(*lb, (double)thr - key_eps(ix, thr, bm));
        // collected, but outside the band that was scored again in float32: bfloat16 key above the band's edge
        if (band_bound) {
            const float edge = c->h_thr[128 + slot];
            if (edge < 3.0e38f) *lb = std::min(*lb, (double)edge - key_eps(ix, edge, bm));
        }
    }
}

// collect pass (radius search / escalation) for staged query `slot`: every row
// with key <= thr_key, reranked exactly.  Synchronous; grows the buffer and
// reruns on overflow.
int run_collect(szg_index *ix, Shard *sh, Ctx *c, int slot, float thr_key, bool has_allow,
                std::vector<Cand> *cands, const CertTag *tag)
{
    HIPCHK(hipSetDevice(sh->device));
    if (sh->n_rows == 0) return SZG_OK;
    // certificate trace: the sweep's threshold and every hit with its key, as the single-query kernel produced them
    auto trace = [&](uint32_t count) {
        if (!cert_room(ix, count)) return;  // (counted as dropped: nothing is gathered for a record that cannot be kept)
        szg_cert_record rec = cert_record(tag->query, tag->pass);
        rec.sweep = 0;
        rec.row_lo = sh->first;
        rec.row_hi = sh->first + sh->n_rows;
        rec.thr = (double)thr_key;
        QMeta single = c->meta[slot];
        single.mq = single.mq_int = single.mq_bf16 = false;
        rec.eps = key_eps(ix, thr_key, single);
        std::vector<szg_cert_entry> ent(count);
        for (uint32_t i = 0; i < count; i++) {
            const szg::RerankOut &r = c->h_out[i];
            const float key = szg::key_from_ordered(r.ukey);
            ent[i] = szg_cert_entry{sh->first + r.row, r.dist, (double)key + key_eps(ix, key, single), key, 0u};
        }
        cert_emit(ix, rec, ent);
    };
    size_t want = std::max<size_t>(c->d_collect.capacity(), 1u << 16);
    for (;;) {
        int rc = c->d_collect.ensure(want);
        if (rc) return rc;
        if (ix->timing >= 2) HIPCHK(hipEventRecord(c->ev_all0, c->pass.work));
        HIPCHK(hipMemsetAsync(c->d_count, 0, sizeof(uint32_t), c->pass.work));
        HIPCHK(hipEventRecord(c->ev_up, c->pass.work));  // the sweep must see the zeroed counter
        std::vector<szg::ScanArgs> a(1);
        fill_collect_args(ix, sh, c, has_allow, slot, 1, &thr_key, c->d_collect, c->d_collect.capacity(), c->d_count, false, &a[0]);
        rc = launch_scans_chained(ix, sh, c, a, scan_geometry(ix, sh, 0));
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(c->h_count, c->d_count, sizeof(uint32_t), hipMemcpyDeviceToHost,
                              c->pass.work));
        if (ix->timing >= 2) HIPCHK(hipEventRecord(c->ev_all1, c->pass.work));
        HIPCHK(hipStreamSynchronize(c->pass.work));
        rc = finish_timing(ix, c);
        if (rc) return rc;
        const uint32_t count = c->h_count[0];
        if (count > c->d_collect.capacity()) {
            want = (size_t)count + count / 8 + 1024;
            continue;
        }
        if (count == 0) {
            if (tag) trace(0);
            return SZG_OK;
        }
        rc = c->d_out.ensure((size_t)count);
        if (rc) return rc;
        rc = c->h_out.ensure((size_t)count);
        if (rc) return rc;
        HIPCHK(szg::launch_rerank(ix->bits, ix->metric, sh->rows, ix->layout, ix->dim,
                                  c->d_q64 + (size_t)slot * ix->dim, c->d_collect, nullptr, count, 1,
                                  c->d_out, c->pass.work));
        HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, sizeof(szg::RerankOut) * count,
                              hipMemcpyDeviceToHost, c->pass.work));
        HIPCHK(hipStreamSynchronize(c->pass.work));
        cands->reserve(cands->size() + count);
        for (uint32_t i = 0; i < count; i++) {
            const szg::RerankOut &r = c->h_out[i];
            cands->push_back(Cand{sh->first + r.row, r.dist, szg::key_from_ordered(r.ukey), 0.0});
        }
        if (tag) trace(count);
        return SZG_OK;
    }
}

// Exact replay of the reference loop over EVERY row (collection.go:672-684 with
// consider(), :583-629): float64 distances for all rows on the device, then the
// heap on the host in visit order.  Bit-faithful in every case, used only when
// history_dependent() says the fast answer could differ.
// (h: the heap to continue -- empty for a search of this handle alone; row_add: what makes a row of this handle global)
static int replay_all_rows(szg_index *ix, std::vector<Ctx *> &ctx, int slot, const uint64_t *allow, int k, GoHeap &h,
                           uint64_t row_add)
{
    for (size_t s = 0; s < ix->shards.size(); s++) {
        Shard *sh = ix->shards[s];
        if (sh->n_rows == 0) continue;
        Ctx *c = ctx[s];
        HIPCHK(hipSetDevice(sh->device));
        const size_t n = sh->n_rows;
        int rc = c->d_out.ensure(n);
        if (rc) return rc;
        rc = c->h_out.ensure(n);
        if (rc) return rc;
        HIPCHK(szg::launch_rerank(ix->bits, ix->metric, sh->rows, ix->layout, ix->dim,
                                  c->d_q64 + (size_t)slot * ix->dim, nullptr, nullptr, (uint32_t)n, 1,
                                  c->d_out, c->pass.work));
        HIPCHK(hipMemcpyAsync(c->h_out, c->d_out, sizeof(szg::RerankOut) * n, hipMemcpyDeviceToHost,
                              c->pass.work));
        std::vector<uint64_t> live((n + 63) / 64, ~0ull);
        if (sh->has_dead)
            HIPCHK(hipMemcpyAsync(live.data(), sh->live_bits, live.size() * sizeof(uint64_t),
                                  hipMemcpyDeviceToHost, c->pass.work));
        HIPCHK(hipStreamSynchronize(c->pass.work));
        const uint64_t *aw = allow ? allow + sh->first / 64 : nullptr;
        for (size_t r = 0; r < n; r++) {
            if (!((live[r >> 6] >> (r & 63)) & 1)) continue;       // removed record
            if (aw && !((aw[r >> 6] >> (r & 63)) & 1)) continue;   // collection.go:592-594
            h.consider_topk(sh->first + r + row_add, c->h_out[r].dist, k);
        }
    }
    return SZG_OK;
}

int run_full_replay(szg_index *ix, std::vector<Ctx *> &ctx, int slot, const uint64_t *allow, int k,
                    std::vector<HeapItem> *res)
{
    GoHeap h;
    const int rc = replay_all_rows(ix, ctx, slot, allow, k, h, 0);
    if (rc) return rc;
    h.drain(res);
    return SZG_OK;
}

// consider()'s top-k branch over every row of this handle in visit order, CONTINUING the heap `h` (rows global:
// + row_base) -- one link of the rank-to-rank chain that settles equal distances across shards (scan_comm.cpp)
int replay_rows_into_heap(szg_index *ix, const double *query, const uint64_t *allow, int k, GoHeap *h)
{
    Batch b;
    b.ix = ix;
    b.ctx.assign(ix->shards.size(), nullptr);
    (void)b.acquire(true);
    for (size_t s = 0; s < ix->shards.size(); s++) {
        Ctx *c = b.ctx[s];
        if (!c) continue;
        HIPCHK(hipSetDevice(ix->shards[s]->device));
        memcpy(c->h_q64, query, sizeof(double) * ix->dim);
        HIPCHK(hipMemcpyAsync(c->d_q64, c->h_q64, sizeof(double) * ix->dim, hipMemcpyHostToDevice, c->pass.work));
    }
    const int rc = replay_all_rows(ix, b.ctx, 0, allow, k, *h, ix->row_base);
    if (rc == SZG_OK) {
        b.release();  // (replay_all_rows has waited for every stream)
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->stats.full_replays++;
    }
    return rc;
}

// The first k eligible rows of a query in visit order are pushed by consider() whatever their
// distance (collection.go:608, `len < K`); a NaN among them -- an antipodal or parallel row
// under the unclamped acos (:831), a NaN / Inf element -- sits in the reference's heap and
// decides what is accepted afterwards.  Such a row need not be anywhere near the best keys,
// so the scan's candidates do not show it: the exact distances of these k rows are computed
// beside every batch and a NaN sends the query to the exact replay.
// rows_out: index-level rows, ascending; at most k.
void first_eligible_rows(const szg_index *ix, const uint64_t *allow, int k, std::vector<uint64_t> *rows_out)
{
    rows_out->clear();
    for (const Shard *sh : ix->shards) {
        if ((int)rows_out->size() >= k) break;
        if (sh->n_rows == 0) continue;
        if (!allow && !sh->has_dead) {
            for (uint64_t r = 0; r < sh->n_rows && (int)rows_out->size() < k; r++) rows_out->push_back(sh->first + r);
            continue;
        }
        const uint64_t words = (sh->n_rows + 63) / 64;
        const uint64_t *aw = allow ? allow + sh->first / 64 : nullptr;
        for (uint64_t w = 0; w < words && (int)rows_out->size() < k; w++) {
            uint64_t m = sh->live_host[w];
            if (aw) m &= aw[w];
            const uint64_t left = sh->n_rows - w * 64;
            if (left < 64) m &= (1ull << left) - 1ull;
            while (m && (int)rows_out->size() < k) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                rows_out->push_back(sh->first + w * 64 + (uint64_t)b);
            }
        }
    }
}

size_t rows_in_shard(const Shard *sh, const std::vector<uint64_t> &rows, uint64_t *out)
{
    size_t n = 0;
    for (uint64_t r : rows) {
        if (r < sh->first || r >= sh->first + sh->n_rows) continue;
        if (out) out[n] = r - sh->first;
        n++;
    }
    return n;
}

int launch_sentinel_rerank(szg_index *ix, Shard *sh, Ctx *c, int nq, hipStream_t stream)
{
    const size_t total = (size_t)c->pass.sent_n * (size_t)nq;
    if (!total) return SZG_OK;
    int rc = c->h_sent_out.ensure(total);
    if (rc) return rc;
    rc = c->d_sent_out.ensure(total);
    if (rc) return rc;
    HIPCHK(szg::launch_rerank(ix->bits, ix->metric, sh->rows, ix->layout, ix->dim, c->d_q64, c->d_sent, nullptr,
                              (uint32_t)c->pass.sent_n, nq, c->d_sent_out, stream));
    HIPCHK(hipMemcpyAsync(c->h_sent_out, c->d_sent_out, total * sizeof(szg::RerankOut), hipMemcpyDeviceToHost, stream));
    c->pass.sent = Sentinels::Own;
    return SZG_OK;
}

// Stage the sentinel rows of the batch that fall into this shard and enqueue their float64
// distances on the ctx stream (lists: one vector of index-level rows per staged query).
// defer: only stage the rows (the batch's tail computes their distances in its one rerank launch).
// The sentinels always ride on the context's OWN stream: they have the whole batch's sweeps to finish in, so when
// the batch itself runs on the scan stream (a short call) they wait for its uploads through an event and stay off
// the critical path.
int enqueue_sentinels(szg_index *ix, Shard *sh, Ctx *c, const std::vector<std::vector<uint64_t>> &lists, int nq, bool defer)
{
    size_t most = 0;
    for (int j = 0; j < nq; j++) most = std::max(most, rows_in_shard(sh, lists[j], nullptr));
    if (most == 0) return SZG_OK;
    SiteScope t_(9);
    HIPCHK(hipSetDevice(sh->device));
    const size_t total = most * (size_t)nq;
    int rc = c->h_sent.ensure(total);
    if (rc) return rc;
    rc = c->d_sent.ensure(total);
    if (rc) return rc;
    for (int j = 0; j < nq; j++) {
        uint64_t *o = c->h_sent + (size_t)j * most;
        std::fill(o + rows_in_shard(sh, lists[j], o), o + most, szg::kInvalidCand);
    }
    hipStream_t st = c->pass.work;
    if (!defer && c->pass.work != c->stream) {
        st = c->stream;
        c->pass.sent_own_stream = true;
        HIPCHK(hipStreamWaitEvent(st, c->ev_up, 0));  // the queries are up (recorded by enqueue_queries on the work stream)
    }
    HIPCHK(hipMemcpyAsync(c->d_sent, c->h_sent, total * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    c->pass.sent_n = (int)most;
    c->pass.sent = Sentinels::Staged;
    if (defer) return SZG_OK;
    return launch_sentinel_rerank(ix, sh, c, nq, st);
}

// ---- the batch pipeline (scan_internal.h) -------------------------------------------------------------------------

bool Batch::acquire(bool may_block)
{
    const bool on_scan_stream = single && ix->serialize_scans;
    if (!on_scan_stream) early_n = 0;  // (the early part's tail needs a second stream to run on)
    for (size_t s = 0; s < ctx.size(); s++) {
        Shard *sh = ix->shards[s];
        if (sh->n_rows == 0) continue;
        Ctx *c = may_block ? ctx_acquire(sh, ctx_limit) : ctx_try_acquire(sh, ctx_limit);
        if (!c) {
            release();
            return false;
        }
        // A call that is ONE batch has nothing to overlap with: uploads, sweeps, merges, re-rank and copy-back go
        // onto the shard's scan stream in order.  On the context's own stream every hand-over to and from the scan
        // stream is a cross-queue event wait, and those cost 20-100 us each on this platform (rocprofv3 timeline of
        // 20-query calls on a 125 K-row shard: the sweeps of a call's batches sat 24-105 us apart).
        if (on_scan_stream) {
            c->pass.work = sh->scan_stream;
            c->pass.early_n = early_n;
        }
        ctx[s] = c;
    }
    return true;
}

void Batch::release()
{
    for (size_t s = 0; s < ctx.size(); s++)
        if (ctx[s]) ctx_release(ix->shards[s], ctx[s]);
    std::fill(ctx.begin(), ctx.end(), nullptr);
}

void Batch::drain()
{
    for (size_t s = 0; s < ctx.size(); s++) {
        if (!ctx[s]) continue;
        (void)hipSetDevice(ix->shards[s]->device);
        (void)hipStreamSynchronize(ctx[s]->pass.work);
        (void)hipStreamSynchronize(ctx[s]->stream);
    }
    release();
}

std::vector<const uint64_t *> Batch::masks(const QueryMasks &mask_of)
{
    std::vector<const uint64_t *> m(nq);
    for (int j = 0; j < nq; j++) {
        m[j] = mask_of(first + j);
        any_mask |= m[j] != nullptr;
    }
    return m;
}

std::vector<const szg_mask *> Batch::handles(const QueryMasks &mask_of) const
{
    std::vector<const szg_mask *> h;
    if (!mask_of.handles) return h;
    h.resize(nq);
    for (int j = 0; j < nq; j++) h[j] = mask_of.handle(first + j);
    return h;
}

void plan_batch(szg_index *ix, int n_queries, int q0, int nb, const BatchRules &r, Batch *b)
{
    const int left = n_queries - q0;
    b->ix = ix;
    b->first = q0;
    b->nb = nb;
    b->ctx.assign(ix->shards.size(), nullptr);
    b->ctx_limit = nb == 0 && ix->serialize_scans ? one_sweep_contexts(ix) : 0;
    if (nb > 0) {
        // (int8 sweeps: two groups of 48 per launch when that many queries are waiting and both images fit LDS)
        const bool two_groups = nb == 3 && mq_uses_i8(ix, r.radius, left) && left > 48 &&
                                szg::mq_i8_lds_bytes(ix->bits, ix->map.r16, 3, 2) <= 160u * 1024u;
        b->nq = std::min(left, 16 * nb * (two_groups ? 2 : 1));
        return;
    }
    // one sweep per query (sketch_plan.h): a short call is ONE batch on the scan stream, from 8 queries on in two parts
    b->nq = one_sweep_batch_size(n_queries, q0, r);
    b->single = q0 == 0 && n_queries <= r.short_max;
    static const bool no_early = getenv("SZG_NO_EARLY_TAIL") != nullptr;  // (A/B hook of scripts/dev_short.py)
    if (b->single && !no_early) b->early_n = short_call_early(n_queries, r, ix->serialize_scans != 0);
}

int stage_query_forms(szg_index *ix, Batch &b, const double *q, bool int_planes,
                      const std::function<void(int, QMeta &)> &adjust)
{
    // (a shared sweep stages its own image: the single-query form is built by stage_single_form for a query that
    // needs it.  Building it here for every query was 1.4 us of the 2.5 us of host preparation per query of a cfg5
    // radius batch.)
    const bool single_form = b.nb == 0;
    Ctx *c0 = nullptr;
    for (Ctx *c : b.ctx) {
        if (!c) continue;
        if (int_planes) c->h_mqQ.resize((size_t)kMaxBatch * ix->dim);  // (grows once per context; bad_alloc: SZG_CATCH)
        if (c0) {
            if (single_form) memcpy(c->h_qsw, c0->h_qsw, ix->qsw_bytes * (size_t)b.nq);
            if (int_planes) memcpy(c->h_mqQ.data(), c0->h_mqQ.data(), sizeof(int32_t) * (size_t)b.nq * ix->dim);
            std::copy(c0->meta, c0->meta + b.nq, c->meta);
            continue;
        }
        c0 = c;
        for (int j = 0; j < b.nq; j++) {
            const double *qj = q + (size_t)j * ix->dim;
            if (single_form) prep_query(ix, qj, c->h_qsw + (size_t)j * ix->qsw_bytes, &c->meta[j]);
            else prep_query_meta(ix, qj, &c->meta[j]);
            if (int_planes) prep_mq_int(ix, qj, &c->meta[j], c->h_mqQ.data() + (size_t)j * ix->dim);
            adjust(j, c->meta[j]);
        }
    }
    return SZG_OK;
}

int stage_single_form(szg_index *ix, Batch &b, const double *q, int j, QMeta *meta)
{
    const size_t off = (size_t)j * ix->qsw_bytes;
    Ctx *c0 = nullptr;
    for (size_t s = 0; s < b.ctx.size(); s++) {
        Ctx *c = b.ctx[s];
        if (!c) continue;
        if (c0) {
            memcpy(c->h_qsw + off, c0->h_qsw + off, ix->qsw_bytes);
        } else {
            c0 = c;
            prep_query(ix, q, c->h_qsw + off, meta);
        }
        c->meta[j] = *meta;
        HIPCHK(hipSetDevice(ix->shards[s]->device));
        HIPCHK(hipMemcpyAsync(c->d_qsw + off, c->h_qsw + off, ix->qsw_bytes, hipMemcpyHostToDevice, c->pass.work));
    }
    return SZG_OK;
}

void emit_topk(const szg_index *ix, const std::vector<HeapItem> &res, int k, int qi, uint64_t *out_rows, double *out_dist,
               int32_t *out_count)
{
    for (int i = 0; i < k; i++) {
        const bool have = i < (int)res.size();
        out_rows[(size_t)qi * k + i] = have ? res[i].row + ix->row_base : UINT64_MAX;
        out_dist[(size_t)qi * k + i] = have ? res[i].priority : 0.0;
    }
    if (out_count) out_count[qi] = (int32_t)res.size();
}

void note_stage_times(szg_index *ix, double t_prep0, double t_enq0)
{
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    const double t_end = now_us();
    ix->stats.host_prep_us += t_enq0 - t_prep0;
    ix->stats.host_enqueue_us += t_end - t_enq0;
}

// ---- one szg_search_topk call -------------------------------------------------------------------------------------
//
// stage() prepares and enqueues a batch on every shard; finish() waits for it and runs the reference's result
// assembly per query (settle()).
struct TopkBatch : Batch {
    std::vector<uint8_t> traced;  // certificate trace: the query's first pass is on record (a deferred query settles twice)
    std::vector<QMeta> meta;  // the queries' constants, with the flags of the path the batch was staged for
    bool bf16 = false;        // the shared sweep is the bfloat16 one
    int kp_wide = 0;          // candidates per query of lists that hold bfloat16-sweep keys
};

struct TopkCall {
    szg_index *ix;
    const double *queries;
    int n_queries, k;
    QueryMasks mask_of;
    uint64_t *out_rows;
    double *out_dist;
    int32_t *out_count;

    const int *trace_index = nullptr;  // certificate trace: the queries' indexes in the call this one was made for

    size_t n_sh = 0;
    int kp = 0;
    bool replay_all = false;  // K beyond the fused selection: every query takes the exact replay
    bool tracing = false;     // the handle's certificate trace is on (read once per call)

    int run();
    TopkBatch plan(int q0);
    int stage(TopkBatch &t);
    int wait_shards(TopkBatch &t);
    void gather(TopkBatch &t, std::vector<std::vector<Cand>> *all, std::vector<double> *thr_min,
                std::vector<uint8_t> *nan_first, int j0, int j1);
    int settle(TopkBatch &t, int j, std::vector<Cand> &cands, double thr_min, bool nan_first, double *t_dev,
               std::vector<HeapItem> *res, bool *defer = nullptr);
    int finish(TopkBatch &t);
};

TopkBatch TopkCall::plan(int q0)
{
    TopkBatch t;
    const int nb = replay_all ? 0 : mq_blocks(ix, n_queries - q0);  // > 0: the batch shares one sweep
    const int batch = std::max(1, std::min(ix->query_batch, kMaxBatch));
    plan_batch(ix, n_queries, q0, nb, BatchRules{batch, kFirstBatch, std::min(kShortCall, kMaxBatch), true, false}, &t);
    t.bf16 = nb > 0 && mq_uses_bf16(ix, false, t.nq);
    // lists of bfloat16-sweep keys (matrix form): the error band holds more rows than the float32 one's, keep
    // enough candidates for the k-th result to clear it
    t.kp_wide = t.bf16 ? std::min(4096, std::max(kp, k + std::max(ix->mq_bf16_slack, k / 2))) : kp;
    t.meta.assign(t.nq, QMeta{});
    return t;
}

// prepare the batch's queries ONCE (swizzled / digit-plane forms, constants; the other shards get copies) and
// enqueue uploads, the first-k rows' distances and the sweeps on every shard
int TopkCall::stage(TopkBatch &t)
{
    const double *q = queries + (size_t)t.first * ix->dim;
    const std::vector<const uint64_t *> masks = t.masks(mask_of);
    const uint64_t *const *mptr = t.any_mask ? masks.data() : nullptr;
    const std::vector<const szg_mask *> handles = t.handles(mask_of);
    const szg_mask *const *hptr = handles.empty() ? nullptr : handles.data();
    const double t_prep0 = now_us();
    const bool int_planes = t.nb > 0 && mq_uses_i8(ix, false, t.nq);
    int rc = stage_query_forms(ix, t, q, int_planes, [&](int j, QMeta &m) {
        m.mq = t.nb > 0 && !int_planes;  // the integer sweeps keep the integer bound
        m.mq_bf16 = t.bf16;
        t.meta[j] = m;
    });
    // rows consider() pushes unconditionally: the first k eligible ones per query
    std::vector<std::vector<uint64_t>> sent;
    if (rc == SZG_OK && ix->tie_mode == 0 && !replay_all) {
        sent.resize(t.nq);
        for (int j = 0; j < t.nq; j++) {
            if (j > 0 && !masks[j] && !masks[j - 1]) sent[j] = sent[j - 1];
            else first_eligible_rows(ix, masks[j], k, &sent[j]);
        }
    }
    const double t_enq0 = now_us();
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        Shard *sh = ix->shards[s];
        if (sh->n_rows == 0) continue;
        rc = enqueue_queries(ix, sh, t.ctx[s], q, t.nq, mptr, t.nb == 0, hptr, s);
        // (before the sweeps: on the context's stream this runs while the scan stream sweeps; a shared sweep whose
        // tail is the refine launch takes the rows along in its one rerank instead)
        if (rc == SZG_OK && !sent.empty())
            rc = enqueue_sentinels(ix, sh, t.ctx[s], sent, t.nq,
                                   t.nb > 0 && mq_tail_takes_sentinels(ix, sh, kp, t.kp_wide, t.nq, t.nb));
        if (rc == SZG_OK && !replay_all)
            rc = t.nb ? enqueue_topk_mq(ix, sh, t.ctx[s], kp, t.kp_wide, t.nq, t.nb, t.any_mask)
                      : enqueue_topk(ix, sh, t.ctx[s], kp, t.nq, t.any_mask);
        if (rc == SZG_OK && replay_all && ix->timing >= 2) {
            const hipError_t e = hipEventRecord(t.ctx[s]->ev_all1, t.ctx[s]->pass.work);
            if (e != hipSuccess) rc = fail(SZG_E_DEVICE, "hipEventRecord", e);
        }
    }
    note_stage_times(ix, t_prep0, t_enq0);
    return rc;
}

// wait for the batch's device work; a shared sweep whose candidate buffer overflowed (threshold from the prefix too
// loose: duplicates, sorted corpora) is redone through the score matrix
int TopkCall::wait_shards(TopkBatch &t)
{
    int rc = SZG_OK;
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        Shard *sh = ix->shards[s];
        if (sh->n_rows == 0) continue;
        hipError_t e = hipSetDevice(sh->device);
        if (e == hipSuccess) e = hipStreamSynchronize(t.ctx[s]->pass.work);
        if (e == hipSuccess && (t.ctx[s]->pass.sent_own_stream || t.early_n > 0)) e = hipStreamSynchronize(t.ctx[s]->stream);
        if (e != hipSuccess) rc = fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
        if (rc == SZG_OK) rc = finish_timing(ix, t.ctx[s]);
        Ctx *c = t.ctx[s];
        if (rc != SZG_OK || !c->pass.cand_cap) continue;  // (not the fused selection: nothing to overflow)
        bool overflow = false;
        for (int j = 0; j < t.nq; j++) overflow |= c->h_cand_count[j * szg::kCandCountStride] > c->pass.cand_cap;
        if (!overflow) continue;
        {
            std::lock_guard<std::mutex> lk(ix->stats_mu);
            ix->stats.mq_launches -= (uint64_t)((t.nq + 16 * c->pass.nb - 1) / (16 * c->pass.nb));  // counted again by the rerun
            ix->stats.mq_queries -= (uint64_t)t.nq;
            ix->stats.mq_bf16_sweeps -= from_bf16_sweep(c->pass.keys) ? 1 : 0;
            ix->stats.mq_fallbacks += 1;
        }
        rc = enqueue_topk_mq(ix, sh, c, kp, t.kp_wide, t.nq, c->pass.nb, c->pass.has_allow, true);
        if (rc == SZG_OK) {
            e = hipStreamSynchronize(c->pass.work);
            if (e != hipSuccess) rc = fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
        }
        if (rc == SZG_OK) rc = finish_timing(ix, c);
    }
    return rc;
}

// every query's candidates, the lists' lower bound and the first-k NaN flag -- taken before anything else, since the
// escalation and replay paths reuse the contexts' output buffers
void TopkCall::gather(TopkBatch &t, std::vector<std::vector<Cand>> *all, std::vector<double> *thr_min,
                      std::vector<uint8_t> *nan_first, int j0, int j1)
{
    for (int j = j0; j < j1; j++) {
        for (size_t s = 0; s < n_sh; s++) {
            Shard *sh = ix->shards[s];
            if (sh->n_rows == 0) continue;
            double lb;
            gather_topk(ix, sh, t.ctx[s], t.meta[j], j, &(*all)[j], &lb);
            (*thr_min)[j] = std::min((*thr_min)[j], lb);
            const Ctx *c = t.ctx[s];
            for (int i = 0; i < c->pass.sent_n; i++) {
                const szg::RerankOut &r = c->sentinel(j, i);
                if (r.row != 0xFFFFFFFFu && std::isnan(r.dist)) (*nan_first)[j] = 1;
            }
        }
    }
}

// One query of a finished batch: consider() replayed over its candidates, certification against the rows the lists
// left out, escalation (a collect sweep) when that fails, the exact replay when the reference's answer depends on its
// heap history.  *t_dev accumulates the time spent waiting on device passes.
// defer (non-null): no device pass may be started now (the call's last sweeps are still running and own the
// contexts' buffers) -- a query that needs one is reported back and settled again once everything has been gathered
int TopkCall::settle(TopkBatch &t, int j, std::vector<Cand> &cands, double thr_min, bool nan_first, double *t_dev,
                     std::vector<HeapItem> *res, bool *defer)
{
    const uint64_t *allow = mask_of(t.first + j);
    int rc = SZG_OK;
    // A NaN distance outside the query's first k eligible rows never enters the reference's heap
    // (`distance < worst` is false, collection.go:608-619); rows with an Inf / NaN element are forced
    // into the lists by the kernels (their float32 norm is not finite) and leave here.  A NaN among
    // the first k rows is the sentinels' business (nan_first: exact replay).
    auto drop_nan = [&](std::vector<Cand> &v) {
        if (nan_first) return;
        v.erase(std::remove_if(v.begin(), v.end(), [](const Cand &c) { return std::isnan(c.dist); }), v.end());
    };
    std::vector<szg_cert_entry> traced;  // the candidates as the pass delivered them (the forced-in rows still among them)
    const bool trace_now = tracing && !(j < (int)t.traced.size() && t.traced[j]);
    if (trace_now) {
        traced.reserve(cands.size());
        for (const Cand &c : cands) traced.push_back(szg_cert_entry{c.row, c.dist, c.ub, c.key, 0u});
    }
    drop_nan(cands);
    replay_topk(cands, k, res);
    // certification: every row outside the lists has a real-number key >= thr_min (the lists' own lower bound),
    // so the result is final once the upper bound of its worst key stays below that
    bool certified = true;
    double kmax = -INFINITY;  // upper bound of the real-number key of the worst result
    const bool zero_query = ix->metric == SZG_COSINE && t.meta[j].m1 == 0;  // all distances 1.0
    if (thr_min < INFINITY && !zero_query) {
        std::vector<std::pair<uint64_t, double>> by_row;  // cands are sorted by row now
        by_row.reserve(cands.size());
        for (const Cand &c : cands) by_row.emplace_back(c.row, c.ub);
        for (const HeapItem &h : *res) {
            auto it = std::lower_bound(by_row.begin(), by_row.end(), std::make_pair(h.row, (double)-INFINITY));
            kmax = std::max(kmax, it->second);
        }
        certified = (int)res->size() == k && kmax < thr_min;
    }
    if (ix->force_escalate && thr_min < INFINITY) certified = false;
    if (nan_first && ix->tie_mode == 0) certified = true;  // answered by the replay below
    const int q_call = trace_index ? trace_index[t.first + j] : t.first + j;
    if (trace_now) {
        szg_cert_record rec = cert_record(ix, q_call, SZG_CERT_TOPK);
        for (size_t s = 0; s < n_sh; s++)
            if (t.ctx[s]) rec.keys = (int32_t)cert_keys(t.ctx[s]->pass.keys);
        rec.sweep = t.nb == 0 ? 0 : (t.bf16 ? 2 : 1);
        rec.certified = certified ? 1 : 0;
        rec.k = k;
        rec.thr_min = thr_min;
        rec.kmax = kmax;
        cert_emit(ix, rec, traced);
        if (t.traced.empty()) t.traced.assign(t.nq, 0);
        t.traced[j] = 1;
    }
    if (!certified) {
        if (defer) {
            *defer = true;
            return SZG_OK;
        }
        {
            std::lock_guard<std::mutex> lk(ix->stats_mu);
            ix->stats.escalations++;
        }
        // kmax bounds the worst result's real-number key; the collect sweep (always the single-query kernel) adds
        // its own error on the rows it tests
        double thr = INFINITY;
        cands.clear();
        const double td = now_us();
        if (t.nb > 0) {  // the escalation sweep is the single-query kernel: it wants the query in ITS form
            QMeta m;
            rc = stage_single_form(ix, t, queries + (size_t)(t.first + j) * ix->dim, j, &m);
            if (rc) return rc;
            t.meta[j].qscale = m.qscale;
            t.meta[j].qconst = m.qconst;
        }
        if ((int)res->size() == k && std::isfinite(kmax) && !zero_query) {
            QMeta single = t.meta[j];  // (now with the single-query path's quantization step)
            single.mq = false;
            single.mq_int = false;
            single.mq_bf16 = false;
            const double e2 = key_eps(ix, kmax, single);
            thr = kmax + 1.05 * e2 + 0.05 * std::fabs(kmax) * 0x1p-20;
        }
        const float thr_f = !(thr < 3.0e38) ? 3.0e38f : std::nextafter((float)thr, INFINITY);
        for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
            Shard *sh = ix->shards[s];
            if (sh->n_rows == 0) continue;
            const CertTag tag{q_call, SZG_CERT_ESCALATION};
            rc = run_collect(ix, sh, t.ctx[s], j, thr_f, t.any_mask, &cands, tracing ? &tag : nullptr);
        }
        *t_dev += now_us() - td;
        if (rc) return rc;
        drop_nan(cands);
        replay_topk(cands, k, res);
    }
    if (ix->tie_mode == 0) {
        std::vector<double> d(cands.size());
        for (size_t i = 0; i < cands.size(); i++) d[i] = cands[i].dist;
        // (a zero cosine query is at distance exactly 1.0 from every row, collection.go:828-830: one big tie, whether or
        // not the candidate list is long enough to show two of its members)
        if (nan_first || zero_query || history_dependent(d.data(), d.size(), k)) {
            if (defer) {
                *defer = true;
                return SZG_OK;
            }
            {
                std::lock_guard<std::mutex> lk(ix->stats_mu);
                ix->stats.full_replays++;
            }
            const double td = now_us();
            rc = run_full_replay(ix, t.ctx, j, allow, k, res);
            *t_dev += now_us() - td;
        }
    }
    return rc;
}

// result assembly for one finished batch
int TopkCall::finish(TopkBatch &t)
{
    if (t.failed) {  // enqueueing failed part-way: drain and release; the enqueue error is already the call's return code
        t.drain();
        return SZG_OK;
    }
    double t_dev = 0;  // time spent waiting on escalation / replay passes (device work)
    double t_early = 0;  // host time of the early phase
    std::vector<std::vector<Cand>> all(t.nq);
    std::vector<double> thr_min(t.nq, INFINITY);
    std::vector<uint8_t> nan_first(t.nq, 0);  // a NaN distance among the query's first k eligible rows
    std::vector<uint8_t> done(t.nq, 0);
    std::vector<HeapItem> res;
    auto emit = [&](int j) { emit_topk(ix, res, k, t.first + j, out_rows, out_dist, out_count); };
    int rc = SZG_OK;
    // A short call's early part (Batch::early_n): those queries' lists and the sentinel rows' distances are complete once
    // the contexts' own streams are; they are assembled here while the scan streams run the call's last sweeps.  A
    // query that needs a device pass of its own (escalation, exact replay) waits for the second phase.
    const int early = replay_all ? 0 : t.early_n;
    if (early > 0) {
        for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
            if (!t.ctx[s]) continue;
            hipError_t e = hipSetDevice(ix->shards[s]->device);
            if (e == hipSuccess) e = hipStreamSynchronize(t.ctx[s]->stream);
            if (e != hipSuccess) rc = fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
        }
        const double te0 = now_us();
        if (rc == SZG_OK) gather(t, &all, &thr_min, &nan_first, 0, early);
        for (int j = 0; j < early && rc == SZG_OK; j++) {
            bool deferred = false;
            rc = settle(t, j, all[j], thr_min[j], nan_first[j] != 0, &t_dev, &res, &deferred);
            if (rc == SZG_OK && !deferred) {
                emit(j);
                done[j] = 1;
            }
        }
        t_early = now_us() - te0;
    }
    if (rc == SZG_OK) rc = wait_shards(t);
    else (void)wait_shards(t);
    const double t_fin0 = now_us() - t_early;
    if (rc == SZG_OK && !replay_all) gather(t, &all, &thr_min, &nan_first, early, t.nq);
    for (int j = 0; j < t.nq && rc == SZG_OK; j++) {
        if (done[j]) continue;
        const int qi = t.first + j;
        if (replay_all) {
            const double td = now_us();
            rc = run_full_replay(ix, t.ctx, j, mask_of(qi), k, &res);
            t_dev += now_us() - td;
            if (rc == SZG_OK) {
                std::lock_guard<std::mutex> lk(ix->stats_mu);
                ix->stats.full_replays++;
            }
        } else {
            rc = settle(t, j, all[j], thr_min[j], nan_first[j] != 0, &t_dev, &res);
        }
        if (rc) break;
        emit(j);
    }
    {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        ix->stats.host_finish_us += now_us() - t_fin0 - t_dev;
        if (rc == SZG_OK) ix->stats.queries += t.nq;
    }
    t.release();
    return rc;
}

int TopkCall::run()
{
    n_sh = ix->shards.size();
    tracing = cert_tracing(ix);
    kp = k + std::max(ix->slack_min, k / 2);
    // The reference bounds K by nothing (collection.go:606-619).  The fused selection keeps kp candidates per wave in
    // LDS; beyond that (kp > 4096 or 64 KiB of lists) every query of the call takes the exact replay: float64
    // distances of all rows on the device, consider() over them on the host.
    for (Shard *s : ix->shards) {
        if (s->n_rows == 0 || replay_all) continue;
        const LaunchGeom g = scan_geometry(ix, s, kp);
        if (szg::scan_lds_bytes(ix->bits, ix->map, kp, g.block) > 64u * 1024u || kp > 4096) replay_all = true;
    }
    if (replay_all) kp = 1;  // the batches only stage their queries

    // A call of several shared-sweep batches is bound by its host work (3-4 us per query against 2.7-3.7 us of GPU
    // time for the int8 and 16-bit sweeps): a second thread takes the finished batches (Finisher, scan_internal.h)
    // while this one prepares and enqueues.
    Finisher<TopkBatch> fin;
    bool threaded = false;
    {
        const int nb0 = replay_all ? 0 : mq_blocks(ix, n_queries);
        threaded = ix->finish_thread && nb0 > 0 && n_queries > 2 * 16 * nb0 * (mq_uses_i8(ix, false, n_queries) ? 2 : 1);
    }
    if (threaded) threaded = fin.start([this](TopkBatch &t) { return finish(t); });
    int rc = run_batches<TopkBatch>(*this, threaded ? fin.hand_over() : nullptr);
    if (threaded) rc = fin.join(rc);
    return rc;
}

int search_topk_impl(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                     uint64_t *out_rows, double *out_dist, int32_t *out_count, const uint64_t *const *allow_ptrs,
                     const szg_mask *const *handles, const int *trace_index)
{
    TopkCall call{ix, queries, n_queries, k, QueryMasks(ix, allow_bits, allow_ptrs, handles), out_rows, out_dist, out_count,
                  trace_index};
    return call.run();
}

}  // namespace szgi
