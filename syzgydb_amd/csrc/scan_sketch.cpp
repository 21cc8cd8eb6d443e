// scan_sketch.cpp -- 8-bit sketch pre-pass for float32 collections (option "sketch", automatic by default) and, under
// option sketch_f64, for float64 ones.
#include "scan_internal.h"

namespace szgi {

// ---- 8-bit sketch pre-pass (float32 rows; float64 rows under sketch_f64 = 1) ---------------------------------------
//
// The reference's "cosine" distance IS the angle (acos(cos)/pi, collection.go:821-832), a metric on directions:
// |d(q, x) - d(q, s)| <= d(x, s) for any sketch s of the row x (Euclidean distance likewise).  The library keeps an
// 8-bit sketch of every float32 row (a quarter of the bytes) as an internal 8-bit index over the same row ranges.
// A query sweeps the sketch shards for their kp best sketch keys (the one-sweep pipeline of scan_topk.cpp on the
// sketch index: sweep, device merges), and ONE rerank launch per batch and shard computes the float64 distances of
// those rows -- on the float32 rows -- together with the query's first k eligible rows and the rows that have no
// usable sketch.  consider() is replayed over them on the host.  With A = max over the rows of d(row, sketch)
// (measured when the sketch is built) and D_lb = a lower bound of the sketch distance of every row outside the
// lists (from the kp-th merged key and its error bound), d(q, x) >= D_lb - A for every row that was not re-ranked:
// the answer is final when its k-th distance is below that.  Otherwise -- and for equal distances or a NaN among the
// first k rows, where the reference's answer depends on its heap history -- the query takes the float32 path.
//
// Option sketch_f64 = 1 gives a float64 handle (the reference's default quantization) the same second index: an eighth
// of its rows' bytes.  Nothing above depends on the width: the build kernel reads doubles (sketch_build_f64_kernel), the
// rerank is launch_rerank on the handle's own 64-bit rows, and "the float32 path" below is, for such a handle, its own
// full-precision path.

constexpr uint64_t kAutoMinRows = 65536;  // auto mode: smaller collections keep no second index
constexpr int kAutoWindow = 64;           // auto mode steps aside once kAutoFallbacks of the last kAutoWindow
constexpr int kAutoFallbacks = 16;        // eligible queries were handed over to the full sweep

bool sketch_applies(const szg_index *ix, int k)
{
    if (!sketch_applies_rows(ix)) return false;
    // the sketch sweep must keep its lists short: 8-bit rows pass four times as fast as float32 rows, and with
    // LDS-resident lists of hundreds (k = 100: 1.35 ms per sweep) the pre-pass is slower than the sweep it replaces
    const int kk = k + ix->sketch_extra;
    return kk + std::max(ix->slack_min, kk / 2) <= 96;
}

bool sketch_applies_rows(const szg_index *ix)
{
    if (!ix->sketch_on || ix->sk_disabled) return false;
    if (ix->bits != 32 && !(ix->bits == 64 && ix->sketch_f64 == 1)) return false;
    uint64_t n = 0;
    for (const Shard *sh : ix->shards) n += sh->n_rows;
    uint64_t min_rows = (uint64_t)ix->sketch_min_rows;
    if (ix->sketch_on == 2) {
        // the test hooks drive rare branches of the full-precision path: a default must not steer around them
        if (ix->force_escalate || ix->force_matrix || ix->force_no_refine) return false;
        if (ix->sk_nomem || ix->sk_off_gen.load(std::memory_order_relaxed) == ix->gen) return false;
        min_rows = std::max(min_rows, kAutoMinRows);
    }
    return n >= min_rows;
}

void sketch_rearm(szg_index *ix)
{
    ix->sk_need_full = true;
    ix->sk_disabled = false;
    if (ix->sk_nomem && ix->sketch) {  // (a step aside after a failure in the pipeline kept the sketch index)
        szg_index_destroy(ix->sketch);
        ix->sketch = nullptr;
    }
    ix->sk_nomem = false;
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->sk_hist = 0;
    ix->sk_hist_n = 0;
}

// auto mode, before the first build: the sketch (a dim-byte row per row, in 64-byte steps, plus its contexts) must
// leave an eighth of every card's memory -- at least 1 GiB -- free
static bool sketch_fits(const szg_index *ix)
{
    std::vector<std::pair<int, uint64_t>> need;  // device, bytes
    for (const Shard *sh : ix->shards) {
        const uint64_t b = sh->n_rows * (((uint64_t)ix->dim + 63) & ~63ull) + (64ull << 20);
        auto it = std::find_if(need.begin(), need.end(), [&](const std::pair<int, uint64_t> &p) { return p.first == sh->device; });
        if (it == need.end()) need.emplace_back(sh->device, b);
        else it->second += b;
    }
    for (const auto &p : need) {
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(p.first) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
        const uint64_t margin = std::max<uint64_t>(total_b / 8, 1ull << 30);
        if ((uint64_t)free_b < p.second + margin) return false;
    }
    return true;
}

// bring the sketch index up to date with the rows (callers hold ix->sk_mu)
int sketch_sync(szg_index *ix)
{
    if (ix->sk_gen == ix->gen && ix->sketch) return SZG_OK;
    if (!ix->sketch) {
        if (ix->sketch_on == 2 && !sketch_fits(ix)) return fail(SZG_E_NOMEM, "sketch: over the memory rule");
        std::vector<int> devs;
        for (Shard *sh : ix->shards) devs.push_back(sh->device);
        int rc = szg_index_create(&ix->sketch, ix->dim, 8, ix->metric, devs.data(), (int)devs.size());
        if (rc) return rc;
        ix->sk_need_full = true;
        ix->sketch->is_sketch = true;  // (its queries take two digit planes: scan_planes)
        ix->sketch->timing = ix->timing;
        options_replay(ix, ix->sketch);
    }
    szg_index *sk = ix->sketch;
    const size_t n_sh = ix->shards.size();
    bool full = ix->sk_need_full;
    for (size_t s = 0; s < n_sh && !full; s++) {
        const Shard *a = ix->shards[s], *b = sk->shards[s];
        if (b->n_rows > a->n_rows || (b->n_rows && b->first != a->first)) full = true;
    }
    if (ix->sk_dirty_rows.size() > 4096) full = true;
    const bool euclid = ix->metric != SZG_COSINE;
    // Euclidean collections share ONE scale (the largest |x_i|): rows beyond it force a rebuild.  The scale pass reports
    // the bits of a float for float32 rows and of a double for float64 rows.
    auto max_abs = [&](bool only_new, double *out) -> int {
        double g = 0.0;
        for (size_t s = 0; s < n_sh; s++) {
            Shard *a = ix->shards[s], *b = sk->shards[s];
            const uint64_t have = only_new ? b->n_rows : 0;
            if (a->n_rows <= have) continue;
            HIPCHK(hipSetDevice(a->device));
            unsigned long long bits = 0;
            DevBuf<unsigned long long> d_max;
            if (int rc = d_max.ensure(2)) return rc;
            hipError_t e = hipMemset(d_max, 0, 16);
            if (e == hipSuccess)
                e = szg::launch_sketch_build(a->rows, ix->layout, ix->bits, ix->dim, nullptr, sk->layout, have,
                                             a->n_rows - have, nullptr, d_max, nullptr, nullptr, 0, 0.0, 1, nullptr);
            if (e == hipSuccess) e = hipMemcpy(&bits, d_max, sizeof(bits), hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail(SZG_E_DEVICE, "sketch scale pass", e);
            double v;
            if (ix->bits == 64) {
                memcpy(&v, &bits, 8);
            } else {
                const uint32_t fb = (uint32_t)bits;
                float f;
                memcpy(&f, &fb, 4);
                v = (double)f;
            }
            g = std::max(g, v);
        }
        *out = g;
        return SZG_OK;
    };
    if (euclid && !full) {
        double g = 0.0;
        int rc = max_abs(true, &g);
        if (rc) return rc;
        if (g > ix->sk_gscale) full = true;
    }
    if (full) {
        std::vector<uint64_t> counts;
        for (Shard *sh : ix->shards) counts.push_back(sh->n_rows);
        int rc = reset_shards(sk, counts);
        if (rc) return rc;
        ix->sk_max_ang = 0.0;
        ix->sk_exc.clear();
        ix->sk_dirty_rows.clear();
        ix->sk_live_dirty = true;
        ix->sk_gscale = 0.0;
        if (euclid) {
            double g = 0.0;
            rc = max_abs(false, &g);
            if (rc) return rc;
            ix->sk_gscale = g > 0.0 ? g : 1.0;
        }
    }
    const uint32_t exc_cap = 4096;
    for (size_t s = 0; s < n_sh; s++) {
        Shard *a = ix->shards[s], *b = sk->shards[s];
        if (a->n_rows == 0) continue;
        HIPCHK(hipSetDevice(a->device));
        if (b->n_rows == 0) b->first = a->first;
        const uint64_t have = full ? 0 : b->n_rows;
        std::vector<uint32_t> list;  // overwritten rows of this shard that already had a sketch
        if (!full)
            for (uint64_t r : ix->sk_dirty_rows)
                if (r >= a->first && r < a->first + have) list.push_back((uint32_t)(r - a->first));
        if (have == a->n_rows && list.empty()) continue;
        if (ix->force_sketch_nomem) return fail(SZG_E_NOMEM, "hipMalloc(sketch): refused (force_sketch_nomem)");
        int rc = shard_reserve(sk, b, a->n_rows);
        if (rc) return rc;
        // rewritten rows: their resident norms (the shared bfloat16 sweep's) are stale from the first of them on
        for (uint32_t r : list) b->norm_valid = std::min<uint64_t>(b->norm_valid, r);
        DevBuf<unsigned long long> d_ang;
        DevBuf<uint32_t> d_exc, d_list;
        rc = d_ang.ensure(2);
        if (rc == SZG_OK) rc = d_exc.ensure(exc_cap + 1);
        if (rc == SZG_OK && !list.empty()) rc = d_list.ensure(list.size());
        if (rc) return rc;
        HIPCHK(hipMemset(d_ang, 0, 16));
        HIPCHK(hipMemset(d_exc, 0, (exc_cap + 1) * sizeof(uint32_t)));
        hipError_t e = hipSuccess;
        if (a->n_rows > have)
            e = szg::launch_sketch_build(a->rows, ix->layout, ix->bits, ix->dim, b->rows, sk->layout, have, a->n_rows - have,
                                         nullptr, d_ang, d_exc + 1, d_exc, exc_cap, ix->sk_gscale, 0, nullptr);
        if (e == hipSuccess && !list.empty()) {
            e = hipMemcpy(d_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
            if (e == hipSuccess)
                e = szg::launch_sketch_build(a->rows, ix->layout, ix->bits, ix->dim, b->rows, sk->layout, 0, list.size(),
                                             d_list, d_ang, d_exc + 1, d_exc, exc_cap, ix->sk_gscale, 0, nullptr);
        }
        unsigned long long ang_bits = 0;
        std::vector<uint32_t> exc(exc_cap + 1, 0);
        if (e == hipSuccess) e = hipMemcpy(&ang_bits, d_ang, sizeof(ang_bits), hipMemcpyDeviceToHost);  // (synchronises)
        if (e == hipSuccess) e = hipMemcpy(exc.data(), d_exc, exc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, "sketch build", e);
        double ang;
        memcpy(&ang, &ang_bits, sizeof(ang));
        ix->sk_max_ang = std::max(ix->sk_max_ang, ang);
        if (exc[0] > exc_cap || ix->sk_exc.size() + exc[0] > exc_cap) {
            // a collection of zero / non-finite rows: nothing to gain -- give the second index (+25 % memory; +12.5 % of
            // float64 rows) back;
            // the next load / synth gets a fresh try
            ix->sk_disabled = true;
            szg_index_destroy(ix->sketch);
            ix->sketch = nullptr;
            ix->sk_need_full = true;
            ix->sk_dirty_rows.clear();
            return SZG_OK;
        }
        for (uint32_t i = 0; i < exc[0]; i++) {
            const uint64_t r = a->first + exc[1 + i];
            if (std::find(ix->sk_exc.begin(), ix->sk_exc.end(), r) == ix->sk_exc.end()) ix->sk_exc.push_back(r);
        }
        if (a->n_rows > b->n_rows) {
            rc = shard_set_live(b, b->n_rows, a->n_rows);
            if (rc) return rc;
            b->n_live += a->n_rows - b->n_rows;
            b->n_rows = a->n_rows;
            ix->sk_live_dirty = true;
        }
    }
    if (ix->sk_live_dirty) {  // tombstones: the sketch shards take the rows' live bits over
        for (size_t s = 0; s < n_sh; s++) {
            Shard *a = ix->shards[s], *b = sk->shards[s];
            if (a->n_rows == 0) continue;
            HIPCHK(hipSetDevice(a->device));
            const uint64_t words = (a->n_rows + 63) / 64;
            for (uint64_t w = 0; w < words; w++) b->live_host[w] = a->live_host[w];
            HIPCHK(hipMemcpy(b->live_bits, b->live_host.data(), words * sizeof(uint64_t), hipMemcpyHostToDevice));
            b->has_dead = a->has_dead;
            b->n_live = a->n_live;
        }
        ix->sk_live_dirty = false;
    }
    std::sort(ix->sk_exc.begin(), ix->sk_exc.end());
    ix->sk_dirty_rows.clear();
    ix->sk_need_full = false;
    ix->sk_gen = ix->gen;
    return SZG_OK;
}

// ---- test hooks: the sketch state as it stands ----------------------------------------------------------------------

int sketch_debug_info(szg_index *ix, szg_sketch_info *out, uint64_t *out_exc_rows, uint64_t exc_capacity)
{
    std::lock_guard<std::mutex> lk(ix->sk_mu);
    const szg_index *sk = ix->sketch;
    memset(out, 0, sizeof(*out));
    out->exists = sk ? 1 : 0;
    out->in_sync = sk && ix->sk_gen == ix->gen ? 1 : 0;
    out->disabled = ix->sk_disabled ? 1 : 0;
    out->n_shards = sk ? (int32_t)sk->shards.size() : 0;
    if (sk)
        for (const Shard *sh : sk->shards) out->rows += sh->n_rows;
    out->max_ang = ix->sk_max_ang;
    out->gscale = ix->sk_gscale;
    out->n_exc = ix->sk_exc.size();
    if (!out_exc_rows) return SZG_OK;
    if (exc_capacity < ix->sk_exc.size()) return fail(SZG_E_TRUNCATED, "sketch info: exception buffer too small");
    if (!ix->sk_exc.empty()) memcpy(out_exc_rows, ix->sk_exc.data(), ix->sk_exc.size() * sizeof(uint64_t));
    return SZG_OK;
}

int sketch_debug_rows(szg_index *ix, uint64_t first_row, uint64_t n_rows, uint8_t *out, uint64_t *out_live_words,
                      uint64_t live_capacity)
{
    std::lock_guard<std::mutex> lk(ix->sk_mu);
    szg_index *sk = ix->sketch;
    if (!sk) return fail(SZG_E_RANGE, "sketch rows: the handle has no sketch index");
    if (out_live_words) {
        const size_t words = index_words(szg_index_rows(sk));
        if (live_capacity < words) return fail(SZG_E_TRUNCATED, "sketch rows: live word buffer too small");
        for (const Shard *sh : sk->shards) {  // the words the sweeps read (shard starts are multiples of 64)
            if (sh->n_rows == 0) continue;
            HIPCHK(hipSetDevice(sh->device));
            HIPCHK(hipMemcpy(out_live_words + sh->first / 64, sh->live_bits, index_words(sh->n_rows) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost));
        }
    }
    return szg_index_read_rows(sk, first_row, n_rows, out);
}

// ---- what every call through the sketch fixes before its first batch ------------------------------------------------

SketchPlan sketch_call_plan(const szg_index *ix, int n_queries, int kp)
{
    const szg_index *sk = ix->sketch;
    SketchPlan p;
    p.gs = ix->sk_gscale;
    p.slack = sketch_slack(ix->sk_max_ang, p.gs, ix->dim);
    // wide and shared batches (sketch_plan.h: the options are read from the sketch index): only where every non-empty
    // shard's launch of 32 (33 .. 64) qualifies for the form, and there is one
    auto every_shard = [&](bool (*serves)(const szg_index *, const Shard *, int, int)) {
        bool any = false;
        for (const Shard *sh : sk->shards) {
            if (sh->n_rows == 0) continue;
            any = true;
            if (!serves(sk, sh, kp, ix->sketch_list)) return false;
        }
        return any;
    };
    const SketchShape s = sketch_shape(ix, sk);
    p.wide = sketch_call_wide(s, n_queries, true);
    if (p.wide && !every_shard(sketch_wide_serves)) p.wide = 0;
    p.share = sketch_call_share(s, n_queries, kp, p.wide, true);
    if (p.share && !every_shard(sketch_share_serves)) p.share = 0;
    return p;
}

void sketch_plan_batch(const szg_index *ix, int n_queries, int q0, int wide, Batch *b, int share)
{
    plan_batch(ix->sketch, n_queries, q0, 0, sketch_batch_rules(n_queries, wide, share, ix->query_batch), b);
}

int sketch_stage_forms(szg_index *sk, double gs, Batch &b, const double *q, const uint8_t *handed, std::vector<double> *scratch,
                       const std::function<void(int, QMeta &)> &adjust)
{
    const size_t dim = (size_t)sk->dim;
    if (handed || gs > 0.0) {  // (cosine, every query served: the queries as they are)
        scratch->resize((size_t)b.nq * dim);
        for (int j = 0; j < b.nq; j++) {
            double *o = scratch->data() + (size_t)j * dim;
            if (handed && handed[j]) std::fill(o, o + dim, 0.0);  // (sweeps as zeros, collects nothing)
            else sketch_scale_query(q + (size_t)j * dim, (int)dim, gs, o);
        }
        q = scratch->data();
    }
    return stage_query_forms(sk, b, q, false, adjust);
}

// ---- one search call through the sketch ---------------------------------------------------------------------------
//
// The batch pipeline (run_batches, scan_internal.h) on the sketch index's contexts: stage() uploads a batch's queries
// and extra rows and enqueues, per shard, the sketch sweeps, the merges and one float32-row rerank; finish() settles
// the batch's queries on the host -- a short call's first queries while its last sweeps still run -- and collects
// the ones the certificate does not settle for the full sweep.
struct SketchCall {
    szg_index *ix;  // the float32 (sketch_f64: float64) handle (rows, masks, results)
    szg_index *sk;  // its sketch index (contexts, sweeps)
    const double *queries;
    int n_queries, k;
    QueryMasks mask_of;
    uint64_t *out_rows;
    double *out_dist;
    int32_t *out_count;
    std::vector<int> redo;  // queries handed over to the full sweep, ascending

    size_t n_sh = 0;
    int kp = 0;
    SketchPlan p;  // gs, slack, and whether the call takes wide batches
    std::vector<int> extra;                     // per shard: entries behind each list (the drop bound's slot, k first
                                                // rows, remembered rows)
    std::vector<uint64_t> firstk_open, firstk;  // first k eligible rows of an unfiltered / of the current query
    std::vector<double> q_scaled;
    std::vector<Cand> cands;
    std::vector<HeapItem> res;
    std::vector<double> dd;
    bool tracing = false;  // the handle's certificate trace is on

    int run();
    Batch plan(int q0);
    int stage(Batch &b);
    void settle(Batch &b, int j);
    int finish(Batch &b);
};

int SketchCall::run()
{
    n_sh = ix->shards.size();
    tracing = cert_tracing(ix);
    const int kk = k + ix->sketch_extra;
    kp = kk + std::max(ix->slack_min, kk / 2);
    p = sketch_call_plan(ix, n_queries, kp);
    sk->timing = ix->timing;
    extra.assign(n_sh, 0);
    for (size_t s = 0; s < n_sh; s++) {
        const Shard *a = ix->shards[s];
        size_t exc = 0;
        for (uint64_t r : ix->sk_exc) exc += (r >= a->first && r < a->first + a->n_rows) ? 1 : 0;
        extra[s] = 1 + k + (int)exc;
    }
    first_eligible_rows(ix, nullptr, k, &firstk_open);
    redo.reserve(n_queries);
    cands.reserve((size_t)n_sh * kp + ix->sk_exc.size() + (size_t)k);
    dd.reserve(cands.capacity());
    // A wide call's device step (7.6-8 us per query at 1M x 768) is close above the host's 7.3 us per query on one
    // thread: a second thread settles the finished batches (option finish_thread), as in long shared-sweep calls, and
    // leaves the caller 4-4.5 us.
    Finisher<Batch> fin;
    bool threaded = p.wide != 0 && ix->finish_thread && n_queries > 2 * szg::kMatrixWideQueries;
    if (threaded) threaded = fin.start([this](Batch &b) { return finish(b); });
    int rc = run_batches<Batch>(*this, threaded ? fin.hand_over() : nullptr);
    if (threaded) rc = fin.join(rc);
    return rc;
}

Batch SketchCall::plan(int q0)
{
    Batch b;
    sketch_plan_batch(ix, n_queries, q0, p.wide, &b, p.share);
    return b;
}

int SketchCall::stage(Batch &b)
{
    const double t_prep0 = now_us();
    const int dim = ix->dim;
    const double *q = queries + (size_t)b.first * dim;
    const std::vector<const uint64_t *> masks = b.masks(mask_of);
    const uint64_t *const *mptr = b.any_mask ? masks.data() : nullptr;
    const std::vector<const szg_mask *> handles = b.handles(mask_of);
    // option query_prep: the card prepares the batch from the float64 queries that go up for the rerank anyway (the
    // division by gs, the image, the constants: query_prep.h) -- no host loop here, no image upload below.  The sweeps
    // read the constants on the card (ScanArgs::qmeta); the host gets them in finish(), before the first settle.
    // Nothing between here and there reads the contexts' h_qsw or meta[] for such a batch: fill_scan_args, the one
    // reader there was, hands the kernels the card's table instead.
    const bool on_card = query_prep_serves(ix->query_prep, b.nq);
    int rc = SZG_OK;
    if (!on_card) rc = sketch_stage_forms(sk, p.gs, b, q, nullptr, &q_scaled, [](int, QMeta &) {});
    // behind each query's list: the drop bound's slot (the short-list merge writes it), its first k eligible rows of
    // the shard (kInvalidCand-padded to k), then the shard's eligible rows without a usable sketch
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        Ctx *c = b.ctx[s];
        if (!c) continue;
        const Shard *a = ix->shards[s];
        const size_t stride = (size_t)kp + extra[s];
        rc = c->h_sent.ensure((size_t)b.nq * stride);
        if (rc == SZG_OK) rc = c->d_sent.ensure((size_t)b.nq * stride);
        if (rc) break;
        for (int j = 0; j < b.nq; j++) {
            const uint64_t *m = masks[j];
            if (m) first_eligible_rows(ix, m, k, &firstk);
            const std::vector<uint64_t> &fk = m ? firstk : firstk_open;
            uint64_t *o = c->h_sent + (size_t)j * stride + kp;
            *o++ = szg::kInvalidCand;  // (no drop bound: the full lists' merge leaves it)
            size_t n = rows_in_shard(a, fk, o);
            for (; n < (size_t)k; n++) o[n] = szg::kInvalidCand;
            sketchless_rows(ix, a, m, [&](uint64_t l, bool ok) { o[n++] = ok ? l : szg::kInvalidCand; });
        }
    }
    const double t_enq0 = now_us();
    uint64_t n_prep_launches = 0;
    for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
        Ctx *c = b.ctx[s];
        if (!c) continue;
        Shard *h = sk->shards[s];
        const size_t stride = (size_t)kp + extra[s];
        hipError_t e = hipSetDevice(h->device);
        // (ahead of the queries' upload: the sweeps wait for that, and the merges and rerank come after the sweeps)
        if (e == hipSuccess)
            e = hipMemcpyAsync(c->d_sent, c->h_sent, sizeof(uint64_t) * b.nq * stride, hipMemcpyHostToDevice, c->pass.work);
        if (e != hipSuccess) {
            rc = fail(SZG_E_DEVICE, "sketch candidates upload", e);
            break;
        }
        // (the float64 queries unscaled: the rerank is on the rows; a resident mask's shard words serve the sketch
        // shard too: same rows, same device)
        rc = enqueue_queries(sk, h, c, q, b.nq, mptr, !on_card, handles.empty() ? nullptr : handles.data(), s,
                             on_card ? &p.gs : nullptr);
        if (rc == SZG_OK && on_card) n_prep_launches++;
        const RerankOn on{ix, ix->shards[s], extra[s], ix->sketch_list, p.wide != 0 || p.share != 0, p.share != 0};
        if (rc == SZG_OK) rc = enqueue_topk(sk, h, c, kp, b.nq, b.any_mask, &on);
    }
    note_stage_times(ix, t_prep0, t_enq0);
    if (rc == SZG_OK) {
        std::lock_guard<std::mutex> lk(ix->stats_mu);
        (on_card ? ix->qp.queries_dev : ix->qp.queries_host) += (uint64_t)b.nq;
        ix->qp.launches += n_prep_launches;
    }
    return rc;
}

// one query of a finished batch: its answer, or a hand-over to the full sweep
void SketchCall::settle(Batch &b, int j)
{
    const int qi = b.first + j;
    cands.clear();
    double lb = INFINITY;  // lower bound of the real-number sketch key of every eligible row outside the lists
    bool nan_first = false;
    bool zero_query = false;
    std::vector<szg_cert_entry> traced;  // certificate trace: each shard's list entries (sketch keys), then the rows beside them
    for (size_t s = 0; s < n_sh; s++) {
        const Ctx *c = b.ctx[s];
        if (!c) continue;
        double l;
        const size_t n0 = cands.size();
        gather_topk(sk, sk->shards[s], c, c->meta[j], j, &cands, &l);
        for (size_t i = n0; tracing && i < cands.size(); i++)
            traced.push_back(szg_cert_entry{cands[i].row, cands[i].dist, cands[i].ub, cands[i].key, 0u});
        // short lists: a row the sweep's blocks did not output has a key at or above the drop bound (entry kp)
        const szg::RerankOut &drop = c->drop_bound(j);
        if (drop.row != 0xFFFFFFFFu) {
            const float key = szg::key_from_ordered(drop.ukey);
            l = std::min(l, (double)key - key_eps(sk, key, c->meta[j]));
        }
        lb = std::min(lb, l);
        zero_query |= ix->metric == SZG_COSINE && c->meta[j].m1 == 0;
        const uint64_t first = ix->shards[s]->first;
        for (int i = kp + 1; i < c->pass.out_stride; i++) {
            const szg::RerankOut &r = c->out(j, i);
            if (r.row == 0xFFFFFFFFu) continue;
            // outside the first k rows a NaN never enters the heap; among them it decides everything
            if (std::isnan(r.dist) && i < kp + 1 + k) nan_first = true;
            cands.push_back(Cand{first + r.row, r.dist, 0.0f, 0.0});
            if (tracing) traced.push_back(szg_cert_entry{first + r.row, r.dist, 0.0, 0.0f, SZG_CERT_ENTRY_NO_KEY});
        }
    }
    cands.erase(std::remove_if(cands.begin(), cands.end(), [](const Cand &c) { return std::isnan(c.dist); }), cands.end());
    unique_rows(cands);
    replay_topk(cands, k, &res);
    bool ok = (!nan_first || ix->tie_mode != 0) && !zero_query;
    double D_used = NAN;
    if (ok && lb < INFINITY) {
        // D_lb: the sketch distance the key bound lb implies, rounded down (sketch_bound.h)
        D_used = sketch_dist_below(p.gs, lb);
        ok = (int)res.size() == k && sketch_settles(res.back().priority, D_used, p.slack);
    }
    if (ok && ix->tie_mode == 0) {
        dd.clear();
        for (const Cand &c : cands) dd.push_back(c.dist);
        if (history_dependent(dd.data(), dd.size(), k)) ok = false;  // the float32 path replays every row
    }
    if (tracing) {
        szg_cert_record rec = cert_record(ix, qi, SZG_CERT_SKETCH);
        rec.keys = SZG_CERT_KEYS_SINGLE;
        rec.sweep = 0;
        rec.certified = ok ? 1 : 0;
        rec.k = k;
        rec.thr_min = lb;
        rec.D = D_used;
        rec.slack = p.slack;
        cert_emit(ix, rec, traced);
    }
    if (!ok) {
        redo.push_back(qi);
        return;
    }
    emit_topk(ix, res, k, qi, out_rows, out_dist, out_count);
}

int SketchCall::finish(Batch &b)
{
    if (b.failed) {
        b.drain();
        return SZG_OK;
    }
    const size_t redo0 = redo.size();
    int rc = SZG_OK;
    // a short call's first queries (Batch::early_n) are complete once the contexts' own streams are
    const int early = b.early_n;
    double t_host = 0.0;
    for (int phase = early ? 0 : 1; phase < 2 && rc == SZG_OK; phase++) {
        for (size_t s = 0; s < n_sh && rc == SZG_OK; s++) {
            Ctx *c = b.ctx[s];
            if (!c) continue;
            hipError_t e = hipSetDevice(ix->shards[s]->device);
            if (e == hipSuccess) e = hipStreamSynchronize(phase ? c->pass.work : c->stream);
            if (e == hipSuccess && phase) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = fail(SZG_E_DEVICE, "hipStreamSynchronize", e);
            if (rc == SZG_OK && phase) rc = finish_timing(sk, c);
            // (queries prepared on the card: their constants' copy was enqueued on pass.work ahead of the sweeps.  An
            // early part's stream waited for its sweeps, which are behind that copy on the scan stream)
            if (rc == SZG_OK) take_card_meta(c);
        }
        if (rc) break;
        const double t0 = now_us();
        for (int j = phase ? early : 0; j < (phase ? b.nq : early); j++) settle(b, j);
        t_host += now_us() - t0;
    }
    if (rc) b.drain();
    else b.release();
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    ix->stats.host_finish_us += t_host;
    if (rc) return rc;
    const uint64_t fb = redo.size() - redo0, settled = (uint64_t)b.nq - fb;
    ix->stats.sketch_queries += settled;
    ix->stats.sketch_fallbacks += fb;
    ix->stats.queries += settled;
    if (ix->sketch_on == 2) {  // the recent window of eligible queries (newest in bit 0)
        const uint64_t off = ix->sk_off_gen.load();
        if (off != 0 && off != ix->gen) {  // re-armed by a mutation since it stepped aside: a fresh window
            ix->sk_hist = 0;
            ix->sk_hist_n = 0;
            ix->sk_off_gen.store(0);
        }
        for (int j = b.first; j < b.first + b.nq; j++) {
            const bool handed = std::binary_search(redo.begin() + redo0, redo.end(), j);
            ix->sk_hist = (ix->sk_hist << 1) | (handed ? 1u : 0u);
            ix->sk_hist_n = std::min(ix->sk_hist_n + 1, kAutoWindow);
        }
        if (ix->sk_hist_n == kAutoWindow && __builtin_popcountll(ix->sk_hist) >= kAutoFallbacks)
            ix->sk_off_gen.store(ix->gen);
    }
    return SZG_OK;
}

int sketch_sync_for_search(szg_index *ix)
{
    // (mutations come under the caller's write lock: after the sync, searches run side by side)
    std::lock_guard<std::mutex> lk(ix->sk_mu);
    int rc = sketch_sync(ix);
    if (rc && ix->sketch_on == 2) {
        // auto mode never turns a working handle into an error: give back what was built, step aside until the
        // next load
        if (ix->sketch) szg_index_destroy(ix->sketch);
        ix->sketch = nullptr;
        ix->sk_need_full = true;
        ix->sk_dirty_rows.clear();
        ix->sk_nomem = true;
        for (Shard *sh : ix->shards)
            if (hipSetDevice(sh->device) == hipSuccess) (void)hipGetLastError();
        rc = SZG_OK;
    }
    return rc;
}

int search_topk_sketch(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                       uint64_t *out_rows, double *out_dist, int32_t *out_count, const uint64_t *const *allow_ptrs,
                       const szg_mask *const *handles)
{
    SketchCall call{ix, nullptr, queries, n_queries, k, QueryMasks(ix, allow_bits, allow_ptrs, handles), out_rows, out_dist,
                    out_count};
    return sketch_served_call(
        ix, call, [] { return true; },
        [&] { return search_topk_impl(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles); },
        [&](const HandedOver &h, const std::vector<int> &redo) {
            return search_topk_handed(ix, h, redo, k, out_rows, out_dist, out_count);
        });
}

int search_topk_handed(szg_index *ix, const HandedOver &h, const std::vector<int> &redo, int k, uint64_t *out_rows,
                       double *out_dist, int32_t *out_count)
{
    const int m = (int)redo.size();
    std::vector<uint64_t> r2((size_t)m * k);
    std::vector<double> d2((size_t)m * k);
    std::vector<int32_t> c2(m);
    const int rc = search_topk_impl(ix, h.q.data(), m, k, nullptr, r2.data(), d2.data(), c2.data(), h.mask_ptrs(),
                                    h.handle_ptrs(), redo.data());
    if (rc) return rc;
    for (int i = 0; i < m; i++) {
        memcpy(out_rows + (size_t)redo[i] * k, &r2[(size_t)i * k], sizeof(uint64_t) * k);
        memcpy(out_dist + (size_t)redo[i] * k, &d2[(size_t)i * k], sizeof(double) * k);
        if (out_count) out_count[redo[i]] = c2[i];
    }
    return SZG_OK;
}

int search_topk_any(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                    uint64_t *out_rows, double *out_dist, int32_t *out_count, const uint64_t *const *allow_ptrs,
                    const szg_mask *const *handles)
{
    // (a batch that shares one sweep on the matrix cores is cheaper per query than any pre-pass)
    const bool shared = ix->multi_query && n_queries >= ix->mq_min;
    if (!shared && sketch_applies(ix, k))
        return search_topk_sketch(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles);
    // a k beyond the pre-pass's lists: a sample pass and a collect sweep of the sketch (scan_sketch_topk.cpp), where the option
    // is on and the sample plan serves the handle -- else the path the call takes without the option
    if (ix->sketch_topk_collect && !shared && n_queries >= 1 && k >= 1 && sketch_applies_rows(ix))
        return search_topk_collect(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles);
    return search_topk_impl(ix, queries, n_queries, k, allow_bits, out_rows, out_dist, out_count, allow_ptrs, handles);
}

}  // namespace szgi

using szgi::fail;

extern "C" {

int szg_index_query_prep_stats(szg_index *ix, szg_query_prep_stats *out)
{
    if (!ix || !out) return fail(SZG_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(ix->stats_mu);
    *out = ix->qp;
    return SZG_OK;
}

// host only: the batch rule of option query_prep (sketch_plan.h)
int szg_debug_query_prep_serves(int option, int batch_queries, int *out_min)
{
    if (out_min) *out_min = szgi::kQueryPrepMin;
    return szgi::query_prep_serves(option, batch_queries) ? 1 : 0;
}

// what a sweep of the handle's sketch would be given for these queries: by prep_query (on_card = 0) or by the kernel (1),
// scaled as SketchCall::stage scales them and launched through enqueue_query_prep as a served batch's are
int szg_debug_query_prep(szg_index *ix, const double *queries, int n_queries, int on_card, uint8_t *out_image, double *out_meta)
{
    SZG_TRY
    using namespace szgi;
    if (!ix || !queries || !out_image || !out_meta) return fail(SZG_E_INVALID, "null argument");
    if (n_queries < 0 || (on_card != 0 && on_card != 1)) return fail(SZG_E_INVALID, "n_queries >= 0, on_card is 0 or 1");
    if (!sketch_applies_rows(ix)) return fail(SZG_E_UNSUPPORTED, "query_prep: the handle keeps no sketch");
    int rc = sketch_sync_for_search(ix);
    if (rc) return rc;
    szg_index *sk = ix->sketch;
    if (!sk || ix->sk_disabled || ix->sk_nomem) return fail(SZG_E_UNSUPPORTED, "query_prep: the handle keeps no sketch");
    const double gs = ix->sk_gscale;  // (sketch_call_plan's p.gs)
    const int dim = ix->dim;
    const size_t qb = sk->qsw_bytes;
    if (!on_card) {
        std::vector<double> scaled(dim);
        for (int j = 0; j < n_queries; j++) {
            const double *q = queries + (size_t)j * dim;
            if (gs > 0.0) {
                sketch_scale_query(q, dim, gs, scaled.data());
                q = scaled.data();
            }
            QMeta m;
            prep_query(sk, q, out_image + (size_t)j * qb, &m);
            double *o = out_meta + (size_t)j * szg::kQueryPrepMeta;
            o[szg::kQpQnorm] = m.qnorm;
            o[szg::kQpM1] = m.m1;
            o[szg::kQpQscale] = m.qscale;
            o[szg::kQpQconst] = m.qconst;
            o[szg::kQpQnorm2] = m.qnorm2;
        }
        return SZG_OK;
    }
    Shard *sh = nullptr;
    for (Shard *s : sk->shards)
        if (s->n_rows) {
            sh = s;
            break;
        }
    if (!sh) return fail(SZG_E_UNSUPPORTED, "query_prep: the sketch has no rows");
    CtxGuard g{sh, ctx_acquire(sh)};
    Ctx *c = g.c;
    HIPCHK(hipSetDevice(sh->device));
    for (int j0 = 0; j0 < n_queries; j0 += kMaxBatch) {
        const int nq = std::min(kMaxBatch, n_queries - j0);
        memcpy(c->h_q64, queries + (size_t)j0 * dim, sizeof(double) * dim * nq);
        HIPCHK(hipMemcpyAsync(c->d_q64, c->h_q64, sizeof(double) * dim * nq, hipMemcpyHostToDevice, c->pass.work));
        rc = enqueue_query_prep(sk, c, nq, gs);
        if (rc == SZG_OK) rc = enqueue_card_meta_copy(c);
        if (rc) return rc;
        // (d_qsw has no pinned twin on this path: h_qsw is the host form's)
        HIPCHK(hipMemcpyAsync(out_image + (size_t)j0 * qb, c->d_qsw, qb * nq, hipMemcpyDeviceToHost, c->pass.work));
        HIPCHK(hipStreamSynchronize(c->pass.work));
        memcpy(out_meta + (size_t)j0 * szg::kQueryPrepMeta, c->h_meta, sizeof(double) * szg::kQueryPrepMeta * nq);
    }
    return SZG_OK;
    SZG_CATCH
}

}  // extern "C"
