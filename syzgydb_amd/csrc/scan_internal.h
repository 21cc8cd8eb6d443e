// scan_internal.h -- types and helpers shared by the translation units that implement
// include/syzgy_scan.h (the C ABI).  Not installed; nothing here crosses the boundary.
//
//   api_common.cpp    error text, container/heap replay, cross-shard merge (host only)
//   scan_query.cpp    query preparation (swizzle / digit planes) and the key error bounds
//   scan_handle.cpp   handle lifetime, contexts, mutations, options, statistics
//   options.cpp       the option table: names, ranges, refusal texts, stores, sketch forwarding (options.h: the rows'
//                     type and szgi::Options, the members szg_set_option writes; plain C++)
//   scan_topk.cpp     the batch pipeline of search calls (plan_batch, stage_query_forms; run_batches is below);
//                     one-sweep-per-query top-k, certification, escalation, exact replay
//   scan_mq.cpp       shared (multi-query) sweeps on the matrix cores
//   scan_sketch.cpp   8-bit sketch pre-pass (option query_prep: its top-k batches' queries prepared on the card --
//                     query_prep.h: the rule, shared with scan_query.cpp; kernels_query_prep.hip: the kernel) and what
//                     every call through the sketch shares: its plan, its batches' query forms (sketch_bound.h: the
//                     arithmetic of its certificates)
//   scan_radius.cpp   radius search (single, batch, coalesced; through the sketch: sketch_radius) and the collect core
//                     (scan_collect.h; collect_plan.h: its buffers)
//   scan_sketch_topk.cpp  top-k of large k through the sketch as a sample pass + that collect core (sketch_topk_collect;
//                     sample_plan.h: its arithmetic; kernels_sample_mx.hip: its kernels)
//   scan_comm.cpp     one-process-per-GPU exchange (RCCL all-gather + merge)
//   scan_mask.cpp     device-resident filter masks (szg_mask) and the searches that take them
//   scan_column.cpp   resident metadata columns (szg_column): comparisons against constants that write masks
//                     (column_str.h: the text columns' predicate and heap sizes; column_dfa.h: the byte automaton of
//                     szg_mask_where_dfa -- its walk, the validation of a caller's tables, the staged table)
//   scan_column_carry.cpp  columns carried across a compaction / reorder (column_carry.h: its index arithmetic)
//   scan_reorder.cpp  compaction and reorder of the resident rows on the device (reorder_plan.h: its host-only checks)
//   scan_bulk.cpp     bulk mutations: lists of rows overwritten, tombstoned or given column values in one call
//                     (bulk_plan.h: its host-only checks; kernels_bulk.hip: its scatters), and appends / overwrites from
//                     vectors in device memory (szg_dev_vectors; kernels_exact.hip: ingest_kernel), stored vectors out
//                     to device memory (fetch_kernel) and searches whose queries lie there (widen_rows_kernel)
//   scan_api.cpp      remaining C entry points (top-k with caller coalescing, distances)
//
// Who owns device memory: dev_mem.h.  Every block is held by a DevBuf / PinnedBuf (scratch of the device that is
// current) or a DevMem (bound to its device: a shard's rows, live bits, norms and staging, a column's parts, a mask's
// words) that frees itself; only scan_comm.cpp keeps its exchange staging by hand.
//
// What a batch borrows per shard is a Ctx: a stream, events and scratch that persist between batches -- every buffer
// a DevBuf / PinnedBuf -- and one Pass, the record of the batch in flight.  The Pass is reset as a
// whole where the context is handed out (ctx_acquire), written by the function that enqueues the work and read by
// the one that finishes it; results in the pinned output buffer are reached through Ctx::out / sentinel / drop_bound.
#pragma once
#include "../../include/syzgy_scan.h"
#include "dev_mem.h"
#include "kernels.h"
#include "options.h"
#include "query_prep.h"
#include "reorder_plan.h"
#include "sketch_bound.h"
#include "sketch_plan.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace szgi {
static_assert(kShortCall <= kMaxBatch, "a short call is one batch");

extern thread_local std::string g_last_error;
int fail(int code, const char *what, hipError_t e = hipSuccess);

#define HIPCHK(expr)                                                    \
    do {                                                                \
        hipError_t e__ = (expr);                                        \
        if (e__ != hipSuccess) return fail(SZG_E_DEVICE, #expr, e__);   \
    } while (0)

// No exception crosses the C boundary: std::vector / std::string growth inside an entry point
// becomes SZG_E_NOMEM.
#define SZG_TRY try {
#define SZG_CATCH                                                          \
    }                                                                      \
    catch (const std::bad_alloc &) { return fail(SZG_E_NOMEM, "out of memory (host)"); } \
    catch (...) { return fail(SZG_E_DEVICE, "unexpected exception"); }

// SZG_DEBUG_TIMERS=1: host time per call site of the enqueue path, printed when a handle is
// destroyed (development aid: which HIP call blocks)
struct SiteTimers {
    static constexpr int N = 12;
    double us[N] = {0};
    uint64_t n[N] = {0};
    const char *name[N] = {"h2d queries", "ev_up+wait", "ev_scan0", "scan launches", "ev_scan1", "ev_done+wait",
                           "merges", "rerank", "d2h", "sentinels", "ev_all", "other"};
    bool on = getenv("SZG_DEBUG_TIMERS") != nullptr;
};
extern SiteTimers g_sites;
struct SiteScope {
    int i;
    std::chrono::steady_clock::time_point t0;
    explicit SiteScope(int i_) : i(i_) { if (g_sites.on) t0 = std::chrono::steady_clock::now(); }
    ~SiteScope()
    {
        if (!g_sites.on) return;
        g_sites.us[i] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        g_sites.n[i]++;
    }
};

int64_t row_bytes_of(int bits, int dim);  // getVectorSize, collection.go:796-811

// ---- container/heap replay (Go stdlib heap.Push / heap.Pop over the
// resultPriorityQueue of collection.go:536-564: max-heap on distance) ---------
struct HeapItem {
    uint64_t row;
    double priority;
};
struct GoHeap {
    std::vector<HeapItem> a;
    bool less(size_t i, size_t j) const { return a[i].priority > a[j].priority; }
    void up(size_t j)
    {
        for (;;) {
            const size_t i = j == 0 ? 0 : (j - 1) / 2;
            if (i == j || !less(j, i)) break;
            std::swap(a[i], a[j]);
            j = i;
        }
    }
    void down(size_t i0, size_t n)
    {
        size_t i = i0;
        for (;;) {
            const size_t j1 = 2 * i + 1;
            if (j1 >= n) break;
            size_t j = j1;
            const size_t j2 = j1 + 1;
            if (j2 < n && less(j2, j1)) j = j2;
            if (!less(j, i)) break;
            std::swap(a[i], a[j]);
            i = j;
        }
    }
    void push(const HeapItem &it)
    {
        a.push_back(it);
        up(a.size() - 1);
    }
    HeapItem pop()
    {
        const size_t n = a.size() - 1;
        std::swap(a[0], a[n]);
        down(0, n);
        HeapItem it = a[n];
        a.pop_back();
        return it;
    }
    // consider()'s top-k branch for one visited record (collection.go:606-619)
    void consider_topk(uint64_t row, double dist, int k)
    {
        if ((int)a.size() <= k) {
            if ((int)a.size() < k || a[0].priority > dist) {
                push(HeapItem{row, dist});
                if ((int)a.size() > k) pop();
            }
        }
    }
    // the pop loop of collection.go:694-697: results in ascending order
    void drain(std::vector<HeapItem> *out)
    {
        out->assign(a.size(), HeapItem{});
        for (size_t i = out->size(); i-- > 0;) (*out)[i] = pop();
    }
};

// per-query constants of the prepared query
struct QMeta {
    double qnorm = 0;   // norm of the prepared (normalised / scaled) query, float paths' error bound
    double m1 = 0;      // sum q_i^2 of the caller's query (zero-query detection)
    double qscale = 0;  // integer paths: prepared query ~ qscale * Q
    double qconst = 0;  // integer paths: sum Q_i
    double qnorm2 = 0;  // euclid: sum g_i^2 of the prepared query g
    bool mq = false;    // answered by the shared float32 MFMA sweep (its own error bound)
    // the int8 shared sweep (8- and 4-bit rows): the query as kMqPlanes int8 digit planes of
    // Q_i = round(v_i / mq_qscale), |Q| <= kMqQmax (the single-query path's own planes stay
    // in qscale / qconst for the escalation sweep)
    bool mq_int = false;
    double mq_qscale = 0, mq_qconst = 0;
    bool mq_bf16 = false;  // (with mq) the shared sweep multiplied bfloat16 roundings of rows and query
};

// The certificate trace of a handle (szg_debug_trace_certificates): what each pass handed to certification, kept for a
// test to check against float64.  Off by default: the search path then pays one relaxed load per settled query.
struct CertTrace {
    std::atomic<bool> on{false};
    std::mutex mu;  // (finisher thread, coalesced callers)
    std::vector<szg_cert_record> recs;
    std::vector<szg_cert_entry> entries;
    uint64_t dropped = 0;  // records that did not fit the caps
};
constexpr size_t kCertMaxRecords = 1u << 18;
constexpr size_t kCertMaxEntries = 1u << 23;  // 32 bytes each: 256 MiB at most

struct Cand {
    uint64_t row;  // index-level row
    double dist;   // reference float64 distance
    float key;     // the scan's ranking key for this row
    double ub;     // key + the error bound of the arithmetic that produced it: the real-number key is <= ub
};

// ---- one in-flight batch of queries on one shard --------------------------------

// the arithmetic that produced the list keys of a finished top-k pass: which error bound certifies them (gather_topk)
enum class ListKeys : uint8_t {
    Single,        // one sweep per query (the single-query kernels; the sketch sweep): the bound of the row width
    SharedInt8,    // int8 shared sweep: exact integers, the integer bound with the sweep's own quantization step
    SharedBf16,    // bfloat16 shared sweep whose keys are the list keys themselves (score-matrix form)
    Bf16Rescored,  // bfloat16 sweep -> float32 re-score of its candidates -> selection: float32 list keys, and every row
                   // the sweep did not collect has a bfloat16 key above h_thr[q], the prefix threshold
    Bf16Band,      // ... re-scored only inside a band (the refine launch): h_thr[128 + q] = the band's edge as well
};
inline bool from_bf16_sweep(ListKeys k) { return k >= ListKeys::SharedBf16; }

// the sentinel rows of the staged queries -- the first k eligible rows of each in visit order (those consider() pushes
// whatever their distance, collection.go:608) -- and where their float64 distances are: a NaN there poisons the
// reference's heap, so the query takes the exact replay
enum class Sentinels : uint8_t {
    None,    // none staged
    Staged,  // the rows are up (d_sent), their distances not yet enqueued
    Own,     // distances in h_sent_out (a rerank launch of their own)
    InOut,   // distances are entries [kp, out_stride) of each query in h_out (they rode in the batch's one rerank)
};

// What was enqueued for the batch that has borrowed the context: reset as a whole when the context is handed out
// (ctx_acquire), written by the enqueue function that stages the work, read when the batch is finished.  Nothing in
// here outlives the batch.
struct Pass {
    hipStream_t work = nullptr;    // where this batch's uploads and post-processing go: `stream`, or the shard's scan
                                   // stream for a call that is a single batch (Batch::acquire)
    int early_n = 0;               // a short call (one batch on the scan stream): the merges, re-rank and copy-back of its
                                   // first early_n queries go onto `stream` behind one event and run -- like the host's
                                   // assembly of those queries -- beside the call's last sweeps (0 = one tail for all)
    int kp = 0;                    // candidates per query in h_out
    int out_stride = 0;            // entries per query in h_out: kp, + what rides behind each list (the sentinels; the
                                   // sketch pre-pass's drop bound and extra rows)
    ListKeys keys = ListKeys::Single;
    Sentinels sent = Sentinels::None;
    bool sent_own_stream = false;  // their re-rank runs on `stream` while the batch runs on the scan stream (`work`)
    int sent_n = 0;                // sentinel entries per query
    // fused selection of a shared sweep: what the rerun of an overflowed candidate buffer needs
    uint32_t cand_cap = 0;         // > 0: the selection was the fused one, with this many entries per query's buffer
    int nb = 0;
    bool has_allow = false;
    // the filter masks of the batch on the device (enqueue_queries): query j's words are allow_base + j * allow_stride
    // -- the context's d_allow slots, or ONE resident mask read in place by every query (stride 0)
    const uint64_t *allow_base = nullptr;
    uint32_t allow_stride = 0;
    // HIP-event timing: scan launches between ev_scan0 and ev_scan1 / ev_p0 and ev_p1 (0 = that pair was not recorded)
    int timed_n = 0, timed_part_n = 0;
    // option query_prep: the batch's prep_n staged queries were prepared on the card (enqueue_query_prep).  Their images
    // are in d_qsw and nowhere else; their constants are in d_meta, where the sweeps read them (ScanArgs::qmeta), on
    // their way to h_meta behind the kernel on `work` -- take_card_meta moves them into meta[] once that stream has
    // been waited for (prep_taken), and until then meta[0 .. prep_n) is NOT the batch's
    int prep_n = 0;
    bool prep_taken = false;
};

// A context is what a batch borrows per shard: a stream, events and scratch buffers that persist between batches,
// and the record of the batch in flight (pass).
struct Ctx {
    hipStream_t stream = nullptr;
    int no = 0;                          // position among its shard's contexts, in the order their streams were created
    hipEvent_t ev_p0 = nullptr, ev_p1 = nullptr;  // HIP-event timing of the early part's sweeps
    hipEvent_t ev_scan0 = nullptr, ev_scan1 = nullptr, ev_all0 = nullptr, ev_all1 = nullptr;
    hipEvent_t ev_scan_done = nullptr;   // this batch's scans have finished (scan stream)
    hipEvent_t ev_up = nullptr;          // this batch's uploads have finished (ctx stream)
    Pass pass;
    // overwritten by staging (not part of the per-acquire reset: 8 KB)
    QMeta meta[kMaxBatch];               // constants of the staged queries
    float mq_qsum[128] = {};             // bfloat16 sweep of 8-bit rows: the sum of each staged query's rounded image values
    int64_t mask_count[kMaxBatch];       // rows of the shard each staged query's resident mask allows, exact (-1: the
                                         // query's words came from the host, mask_pass_rate samples h_allow)
    size_t radius_cap = 0;         // radius batches: entries per sweep the next batch's buffers get (follows the hit counts seen)
    // pinned host staging, kMaxBatch queries
    PinnedBuf<uint8_t> h_qsw;      // swizzled queries for the scan
    PinnedBuf<double> h_q64;       // float64 queries for the rerank
    PinnedBuf<szg::RerankOut> h_out;
    PinnedBuf<uint64_t> h_allow;   // words
    PinnedBuf<uint32_t> h_count;
    // device scratch
    DevBuf<uint8_t> d_qsw;
    DevBuf<double> d_q64;
    DevBuf<uint64_t> d_lists_a, d_lists_b;  // merge ping-pong (ensure_lists)
    DevBuf<szg::RerankOut> d_out;
    DevBuf<uint64_t> d_allow;      // words
    DevBuf<uint64_t> d_collect;    // entries
    DevBuf<uint32_t> d_count;      // hit counters of collect sweeps, one 128-byte line per sweep of a launch
    // multi-query sweep: LDS image of the batch, score matrix
    PinnedBuf<uint8_t> h_mq;
    DevBuf<uint8_t> d_mq;
    std::vector<int32_t> h_mqQ;    // 4-bit int8 sweep: the queries as integers (kMaxBatch x dim)
    DevBuf<float> d_keys;
    // fused selection of the shared sweep: thresholds, candidate buffers, hit counts
    DevBuf<float> d_thr;           // [256] thresholds | band edges
    PinnedBuf<float> h_thr;        // the prefix thresholds of a two-stage batch, for certification
    PinnedBuf<double> h_qscale;    // [256] float32-query scale per staged query (re-score) | |g|^2
    DevBuf<double> d_qscale;
    DevBuf<uint64_t> d_cand;
    DevBuf<uint32_t> d_cand_count;
    PinnedBuf<uint32_t> h_cand_count;
    // the sentinel rows (Sentinels) and their distances; the sketch pre-pass keeps each query's candidates -- its
    // merged list, the drop bound's slot, the extra rows -- in h_sent / d_sent instead
    PinnedBuf<uint64_t> h_sent;
    DevBuf<uint64_t> d_sent;
    PinnedBuf<szg::RerankOut> h_sent_out;
    DevBuf<szg::RerankOut> d_sent_out;
    // option query_prep: the constants of queries prepared on the card, szg::kQueryPrepMeta doubles each (allocated by
    // the first such batch: a handle that leaves the option at 0 holds neither)
    PinnedBuf<double> h_meta;
    DevBuf<double> d_meta;

    // both ping-pong buffers grow together, and both are freed before either comes back
    int ensure_lists(size_t need)
    {
        if (d_lists_b.capacity() >= need) return SZG_OK;  // (allocated last: it has the room only if d_lists_a has)
        int rc = d_lists_a.reset();
        if (rc == SZG_OK) rc = d_lists_b.reset();
        if (rc == SZG_OK) rc = d_lists_a.ensure(need);
        return rc ? rc : d_lists_b.ensure(need);
    }
    // entry i of staged query j in h_out: i < pass.kp its list, then what rides behind it
    const szg::RerankOut &out(int j, int i) const { return h_out[(size_t)j * pass.out_stride + i]; }
    const szg::RerankOut &sentinel(int j, int i) const  // i < pass.sent_n
    {
        return pass.sent == Sentinels::InOut ? out(j, pass.kp + i) : h_sent_out[(size_t)j * pass.sent_n + i];
    }
    // sketch pre-pass with short lists: every row the sweep's blocks did not output has a key at or above this one
    const szg::RerankOut &drop_bound(int j) const { return out(j, pass.kp); }
};

// The resident rows of a shard and their live bits: what rows_reserve grows, and what a compaction / reorder builds
// afresh beside the shard's and then moves into it as a whole.
struct ShardRows {
    explicit ShardRows(int device) : rows(device), live_bits(device) {}
    ShardRows(ShardRows &&) = default;
    ShardRows &operator=(ShardRows &&) = default;  // (what the target held is released)
    uint64_t n_rows = 0;
    uint64_t cap_rows = 0;
    DevMem<uint8_t> rows;      // layout_bytes(cap_rows) + 64 bytes
    DevMem<uint64_t> live_bits;
    uint64_t bits_cap = 0;     // words
};

struct Shard : ShardRows {
    explicit Shard(int device_) : ShardRows(device_), device(device_), zero16(device_), row_norm(device_), stage(device_) {}
    const int device;
    uint64_t first = 0;        // index-level row of this shard's row 0
    uint64_t n_live = 0;
    std::vector<uint64_t> live_host;  // host copy of live_bits (tombstone / append bookkeeping, first-k rows)
    bool has_dead = false;
    int cu_count = 256;
    std::vector<Ctx *> free_ctx;
    std::vector<Ctx *> parked_ctx;   // contexts taken out of rotation ("contexts" option)
    std::vector<Ctx *> all_ctx;
    std::mutex mu;
    std::condition_variable cv;
    // All scan launches of a shard go back to back onto ONE stream: each sweep
    // gets the whole HBM bandwidth and the blocks of a launch stay in lockstep
    // (that is what keeps DRAM pages hot); uploads and the small merge/rerank/
    // copy work of other batches overlap them on the contexts' own streams.
    std::mutex chain_mu;
    hipStream_t scan_stream = nullptr;
    DevMem<uint8_t> zero16;      // 16 zero bytes idle lanes of the multi-query sweep read
    // resident float32 row norms (16-bit rows, shared bfloat16 sweep): rows [0, norm_valid) are up to date; load /
    // synth reset it, appended rows are caught up before the next shared sweep, an overwritten row at once
    DevMem<float> row_norm;
    uint64_t norm_cap = 0, norm_valid = 0;
    std::mutex norm_mu;
    // device staging of the mutation entry points (load / append / overwrite / read-back): kept
    // between calls, so AddDocument in a loop pays no hipMalloc / hipFree per row
    DevMem<uint8_t> stage;
    size_t stage_cap = 0;
    std::mutex stage_mu;         // szg_index_read_rows may run beside other readers (szg_pair_distances)
};

}  // namespace szgi

// One caller of szg_search_topk(n_queries == 1) or szg_search_radius waiting to be answered as part of a batch.
struct PendingSearch {
    const double *query;
    const uint64_t *allow;  // the caller's filter mask, or nullptr
    const szg_mask *handle = nullptr;  // ... or its resident mask (szg_search_topk_masked); never both
    int k;                  // top-k search (radius == 0)
    double radius = 0;      // > 0: radius search (k ignored, collection.go:598-605)
    uint64_t *out_rows;
    double *out_dist;
    int32_t *out_count = nullptr;   // top-k
    uint64_t capacity = 0;          // radius: room in out_rows / out_dist
    uint64_t *out_total = nullptr;  // radius: the full hit count
    int rc = 0;
    bool done = false;
    bool lead = false;  // told to take over as the batch leader
    std::condition_variable cv;
};

struct szg_index : szgi::Options {   // (the run-time options: options.h)
    int dim = 0, bits = 0, metric = 0;
    uint32_t row_bytes = 0, pitch = 0;
    szg::RowLayout layout{};  // of every shard's mirror (linear, or 16-row x 64-byte-step tiles)
    szg::RowMap map{};
    size_t qsw_bytes = 0;
    double norm_bias = 0;     // integer paths: sum n^2 = 4(SQ+SV) + norm_bias (padding removed)
    uint64_t row_base = 0;
    std::vector<szgi::Shard *> shards;
    // 8-bit sketch pre-pass for float32 collections -- float64 ones under sketch_f64 = 1 -- ("sketch" option, sketch_sync /
    // search_topk_sketch)
    szg_index *sketch = nullptr;         // an internal 8-bit index over the same rows, same shard ranges
    std::mutex sk_mu;                    // the sync
    uint64_t gen = 1, sk_gen = 0;        // mutation counter / the value the sketch was synced at
    bool sk_need_full = true;            // load / synth / reset since the last sync
    bool sk_live_dirty = true;           // tombstones since the last sync
    std::vector<uint64_t> sk_dirty_rows; // rows overwritten since the last sync (index-level)
    double sk_max_ang = 0.0;             // max over the rows of d(row, its sketch), the reference's angular distance
    double sk_gscale = 0.0;              // Euclidean collections: the sketch of a row is sk_gscale * n / 255 (0: cosine)
    std::vector<uint64_t> sk_exc;        // rows without a usable sketch (zero rows, non-finite elements): always re-ranked
    bool sk_disabled = false;            // too many such rows
    // auto mode (sketch_on == 2) steps aside -- until the next load -- when the sketch does not fit the memory rule or
    // an allocation of it fails; and -- until the next mutation or load -- when too many recent queries fell back
    bool sk_nomem = false;
    std::atomic<uint64_t> sk_off_gen{0}; // == gen: stepped aside for the fallback share (gen starts at 1)
    uint64_t sk_hist = 0;                // the last sk_hist_n eligible queries, newest in bit 0: 1 = handed over
    int sk_hist_n = 0;                   // (stats_mu)
    uint64_t opt_set = 0;                // the forwarded options (options.h) set so far, bit = table row: replayed,
                                         // with the values the members hold, on the sketch index when it is created
    int n_ctx = 4;            // contexts (and streams) per shard (bfloat16 batches of 1M x 768: 3 -> 4 = 155 -> 162 k queries/s; 6: no more)
    int n_ctx_active = 4;     // of them in rotation (the rest parked): the last accepted value of option "contexts"
    szg_sketch_topk_stats sk_topk{};  // what that path served (stats_mu; szg_index_sketch_topk_stats, szg_reset_stats)
    szg_query_prep_stats qp{};  // which side prepared such calls' queries (stats_mu; szg_index_query_prep_stats, szg_reset_stats)
    bool is_sketch = false;   // this index is the internal sketch of a float32 (or float64) handle: its keys only bound
    // settled by measurement (rounds 1-3): compile-time facts since round 4, A/B through -D and `make variant`
    static constexpr int blocks_per_cu = 0;     // 0 = waves per CU chosen from the row format (scan_geometry)
    static constexpr int block_threads = 256;
    static constexpr int shape_kernels = 1;     // row-shape-specialised kernels where they exist
    static constexpr int ring = 0;              // 8 = always the deep piece ring
    static constexpr int mq_i8 = 1;             // 8- / 4-bit rows: exact integer shared sweep (v_mfma_i32_16x16x64_i8)
    static constexpr int mq_bf16 = 1;           // 64- / 32- / 16-bit rows: shared sweep on bfloat16 roundings, certified
                                                // against its own bound and re-ranked in float64 like every other path
    static constexpr int mq_overlap = 1;        // a batch's threshold pass and tail on the context's stream beside the
                                                // neighbouring batches' sweeps
    static constexpr int mq_bf16_slack = 246;   // candidates kept beyond k where the lists hold bfloat16 keys themselves
    static constexpr int mq_tail_overlap = 0;
    static constexpr int mq_blocks_max = 6;     // query blocks of 16 per shared sweep (LDS image permitting)
    int timing = 0;           // 0 off, 1 HIP events around the scan launches, 2 + around the whole per-batch pipeline
    std::mutex stats_mu;
    // device-resident filter masks (scan_mask.cpp)
    std::atomic<uint64_t> mask_epoch{1};  // moves whenever the row count may (load, synth, appends): older masks are stale
    std::atomic<uint64_t> col_epoch{1};   // moves whenever rows are renumbered or replaced (load, synth, a reorder or
                                          // compaction that moves rows) -- NOT by appends: older columns are stale
    std::atomic<uint64_t> mask_live{0}, mask_dev_bytes{0};
    std::atomic<uint64_t> mask_h2d{0}, mask_d2d{0}, mask_shared{0};  // szg_mask_stats (with the sketch index's own)
    // szg_debug_sketch_masked (counted on the index whose shards were swept: the sketch index): launches that took a masked
    // form of the matrix sweep, those of them whose eligibility was wave-uniform (the tile skip), and their queries
    std::atomic<uint64_t> mx_masked_launches{0}, mx_masked_skip{0}, mx_masked_queries{0};
    // coalescing of concurrent single-query searches (szg_search_topk, n_queries == 1)
    std::mutex comb_mu;
    std::deque<struct PendingSearch *> comb_waiting;
    bool comb_leader = false;
    szg_stats stats{};
    szgi::CertTrace cert;        // certificate trace (test hook)
    szg_comm *comm = nullptr;    // one process per GPU: the attached communicator (borrowed; scan_comm.cpp)
    // queries from device memory (szg_search_*_dev, scan_bulk.cpp): the float64 batch on the source's device (and the
    // list of source rows behind it) and its pinned host copy, kept between calls; dq_mu is held for the length of one
    std::mutex dq_mu;
    szgi::DevMem<double> dq_dev;
    szgi::PinnedBuf<double> dq_host;
};

// A device-resident filter mask (scan_mask.cpp).  Words and counts never change after creation -- except that a
// compaction / reorder of the handle rewrites the masks it is asked to carry (scan_reorder.cpp), under the exclusive
// access every mutation has.
struct szg_mask {
    szg_index *owner = nullptr;
    uint64_t epoch = 0;     // the owner's mask_epoch this mask was made at
    uint64_t rows = 0;      // row count of the handle then
    struct Part {
        explicit Part(int device_ = 0) : device(device_), words(device_) {}
        int device;
        uint64_t first = 0, n_rows = 0;
        size_t pairs = 0;             // 16-byte pairs of words
        szgi::DevMem<uint64_t> words; // 2 * pairs words, then the popcount counter (2 words)
        uint64_t count = 0;           // rows of the shard the mask allows
    };
    std::vector<Part> parts;          // one per shard of the owner
    std::vector<uint64_t> host;       // index-level words, tail bits 0
    uint64_t count = 0;
    uint64_t dev_bytes = 0;
    bool counted = false;             // in the owner's live_masks / device_bytes
};

// A resident metadata column (scan_column.cpp): one value and one present bit per row, each shard's part on the shard's
// own device.  It covers rows [0, rows) of its handle, rows <= szg_index_rows: index appends leave it short until
// szg_column_append catches up.  A text column's value is an 8-byte reference {uint32 start, uint32 len} into the
// part's byte heap (column_str.h has its size rules).
struct szg_column {
    szg_index *owner = nullptr;
    int kind = 0;           // SZG_COL_F64 / SZG_COL_U32 / SZG_COL_STR
    uint64_t epoch = 0;     // the owner's col_epoch this column was made at
    uint64_t rows = 0;
    struct Part {
        explicit Part(int device_ = 0) : device(device_), values(device_), present(device_), heap(device_) {}
        int device;
        uint64_t first = 0, n_rows = 0, cap_rows = 0;  // cap_rows: a multiple of 128
        szgi::DevMem<uint8_t> values;      // cap_rows elements of elem() bytes
        szgi::DevMem<uint64_t> present;    // cap_rows / 64 words in the masks' 16-byte-pair layout, tail bits 0
        std::vector<uint64_t> present_host;  // the same words
        szgi::DevMem<uint8_t> heap;        // text columns: heap_cap bytes, zero behind heap_used
        uint64_t heap_used = 0, heap_cap = 0;  // heap_cap: 0 or a multiple of 16, >= the used bytes rounded up to 16, + 16
        template <typename T> T *values_as() const { return reinterpret_cast<T *>(values.data()); }
    };
    std::vector<Part> parts;              // one per shard of the owner
    size_t elem() const { return kind == SZG_COL_U32 ? sizeof(uint32_t) : 8; }   // (a double, or a text reference)
};

namespace szgi {

struct LaunchGeom {
    int grid, block;
    int rows_per_block;  // rows one block covers per wave step (waves of the block x the map's rows per wave step)
};

// What a (dimension, row width) pair fixes before any device is touched: the packed row, its resident layout, the
// lane map of the one-sweep scan and the size of the prepared query.
struct RowFormat {
    uint32_t row_bytes = 0, pitch = 0;
    szg::RowLayout layout{};
    szg::RowMap map{};
    size_t qsw_bytes = 0;
};

// ---- api_common.cpp
double now_us();
// consider()'s top-k branch replayed over the candidates in visit order, then the pop loop
void replay_topk(std::vector<Cand> &cands, int k, std::vector<HeapItem> *result);
// the candidates sorted by row, one entry per row (a row that reached them twice was re-ranked to the same distance twice)
void unique_rows(std::vector<Cand> &cands);
// a NaN distance, or two exactly equal ones among the best k+1: the reference's answer depends on its heap history
bool history_dependent(const double *dist, size_t n, int k);

// ---- scan_query.cpp
szg::RowMap choose_map(int r16, bool tiled = false);
// SZG_OK; SZG_E_INVALID (dimension or row width out of range, with the error text set); SZG_E_UNSUPPORTED: the format is
// filled in, but the prepared query does not fit the scan's LDS budget (the caller reports it)
int row_format(int dim, int quant_bits, RowFormat *f);
void prep_query(const szg_index *ix, const double *q, uint8_t *out_sw, QMeta *meta);
void prep_query_meta(const szg_index *ix, const double *q, QMeta *meta);  // the constants only (shared sweeps)
double key_eps(const szg_index *ix, double key, const QMeta &m);
// int8 digit planes of a query prepared for a one-sweep scan of ix's 8-bit rows, and the largest |Q| they carry: a
// sketch index takes 2 (16000, option sketch_planes), every other handle 3 (10^6).  prep_query, key_eps and the
// launch (ScanArgs::planes) all ask here.
int scan_planes(const szg_index *ix);
inline double scan_qmax8(const szg_index *ix) { return scan_planes(ix) == 2 ? 16000.0 : 1000000.0; }
// (radius: the batch is a radius batch -- tiled 8-bit rows then stay on the exact int8 sweep: the bfloat16 sweep's
// band around every radius would collect several times the hits)
// nq: the queries of the batch in question -- 8-bit rows take the bfloat16 sweep only for MORE than 48 of them (up to 48
// fit one int8 pass, which measures 7-10 % faster than a bfloat16 pass of three query blocks)
bool mq_uses_i8(const szg_index *ix, bool radius = false, int nq = 1 << 30);
bool mq_uses_bf16(const szg_index *ix, bool radius = false, int nq = 1 << 30);
uint16_t bf16_rne(float f);
double mq_int_scale(const szg_index *ix, double m1);
void prep_mq_int(const szg_index *ix, const double *q, QMeta *meta, int32_t *Qout);
int mq_blocks(const szg_index *ix, int nq, bool radius = false);
// key threshold of a radius search: surely contains every row with distance <= radius
float radius_key_threshold(const szg_index *ix, double radius, const QMeta &meta);

// ---- scan_handle.cpp
int ctx_alloc(szg_index *ix, Shard *sh, Ctx **out);
void ctx_free(Ctx *c);
// limit > 0: only one of the shard's first `limit` contexts (Ctx::no < limit)
Ctx *ctx_acquire(Shard *sh, int limit = 0);
Ctx *ctx_try_acquire(Shard *sh, int limit = 0);
// the forwarded options set on ix so far, applied to its newly created sketch index
void options_replay(szg_index *ix, szg_index *sketch);
// Contexts a call with one sweep per query keeps in flight per shard.  Its sweeps run on the shard's scan stream and
// each batch's uploads, merge, re-rank and copy-back on its context's stream; streams take the hardware queues the
// process opens (GPU_MAX_HW_QUEUES, HIP's default 4) in turn, so the shard's fourth context shares a queue with its scan
// stream, and that batch's tail packets then wait behind sweeps and hold sweeps up (3.1 -> 1.1 ms
// of a 38 ms region outside the sweeps with three).  One stream per queue: queues - 1 contexts, at least 1.
int one_sweep_contexts(const szg_index *ix);
void ctx_release(Shard *sh, Ctx *c);
int shard_stage(Shard *sh, size_t bytes, uint8_t **out);
int upload_rows(szg_index *ix, Shard *sh, uint64_t dst_row, const uint8_t *rows, uint64_t n);
int rows_reserve(const szg::RowLayout &layout, ShardRows *h, uint64_t rows_needed);
int shard_reserve(szg_index *ix, Shard *sh, uint64_t rows_needed);
void live_host_fill(Shard *sh, uint64_t n_rows);
int shard_set_live(Shard *sh, uint64_t lo, uint64_t hi);
void split_rows(const szg_index *ix, uint64_t n_rows, std::vector<uint64_t> *counts);
Shard *shard_of(szg_index *ix, uint64_t row, uint64_t *local);
int reset_shards(szg_index *ix, const std::vector<uint64_t> &counts);
Shard *append_target(szg_index *ix);
void note_overwritten(szg_index *ix, uint64_t row);

// ---- scan_api.cpp: the certificate trace
inline bool cert_tracing(const szg_index *ix) { return ix->cert.on.load(std::memory_order_relaxed); }
// a fresh record of query `query` of its call for pass `pass`: everything that does not apply is NaN / -1
szg_cert_record cert_record(int query, int pass);
// ... of a pass over every row of the handle: row_hi is the end of its last shard
szg_cert_record cert_record(const szg_index *ix, int query, int pass);
// append the record and its entries (dropped as a whole, and counted, when a cap would be passed)
void cert_emit(szg_index *ix, szg_cert_record r, const std::vector<szg_cert_entry> &entries);
// room for a record of n entries?  Asked BEFORE the entries are gathered, so that a record that will not fit costs no
// memory; false counts the record as dropped
bool cert_room(szg_index *ix, size_t n);
// what a collect sweep run by run_collect is traced as (null: not traced)
struct CertTag {
    int query;   // index in its call
    int pass;    // SZG_CERT_ESCALATION / SZG_CERT_RADIUS_SINGLE
};

// ---- scan_topk.cpp
// grid and block of a sweep over n_rows rows (kp = 0: a collect sweep); the second form reads them off a shard
LaunchGeom scan_geometry(int bits, const szg::RowMap &map, uint32_t row_bytes, bool tiled, uint64_t n_rows, int cu_count,
                         int kp);
LaunchGeom scan_geometry(const szg_index *ix, const Shard *sh, int kp);
size_t shard_words(const Shard *sh);
// (handles: null, or the resident masks of the batch's queries -- then `masks` holds their host words -- and `shard_no`,
// the shard's position in its index, which is also the position of its words in every handle)
// (card_prep: null, or the Euclidean sketch scale (0: none) of a batch whose queries the card prepares -- option
// query_prep: enqueue_query_prep behind the float64 upload instead of the single-query forms' upload, the constants' copy
// to the host behind the event the sweeps wait for)
int enqueue_queries(szg_index *ix, Shard *sh, Ctx *c, const double *q, int nq, const uint64_t *const *masks,
                    bool with_single_form = true, const szg_mask *const *handles = nullptr, size_t shard_no = 0,
                    const double *card_prep = nullptr);
// Option query_prep: the 8-bit index's staged float64 queries [0, nq) of the context (d_q64, enqueued on pass.work) ->
// their one-sweep images in d_qsw and constants in d_meta, on pass.work (szg::launch_query_prep; gs: the Euclidean
// sketch's scale, 0 = none).  The search path and the hook szg_debug_query_prep both launch through here.
int enqueue_query_prep(szg_index *ix, Ctx *c, int nq, double gs);
// ... the copy of those constants to h_meta, on pass.work; and, once that stream has been waited for, their move into
// meta[] (flags false, as prep_query leaves them).  Once per batch: further calls do nothing.
int enqueue_card_meta_copy(Ctx *c);
void take_card_meta(Ctx *c);
void fill_scan_args(const szg_index *ix, const Shard *sh, const Ctx *c, bool has_allow, int slot, int nq,
                    szg::ScanArgs *a);
// ... of a collect launch: query slot + j's key threshold thr[j], its buffer buf + j * cap and its counter
// count[j * szg::kCandCountStride].  dense_vote: masked launches take the dense phase where most rows pass every mask
// (false: never -- run_collect)
void fill_collect_args(const szg_index *ix, const Shard *sh, const Ctx *c, bool has_allow, int slot, int nq, const float *thr,
                       uint64_t *buf, size_t cap, uint32_t *count, bool dense_vote, szg::ScanArgs *a);
// (after: the stream that goes on once the sweeps are done -- default the work stream; part 1: the early part of a short
// call, timed with its own event pair)
// (hi: null, or one entry per launch -- a launch of more than szg::kMatrixWideQueries queries is then a shared launch of
// the matrix sweep, on the grid g names: szg::launch_scan_share)
int launch_scans_chained(szg_index *ix, Shard *sh, Ctx *c, const std::vector<szg::ScanArgs> &a, const LaunchGeom &g,
                         hipStream_t after = nullptr, int part = 0, const std::vector<szg::ScanShareHi> *hi = nullptr);
// does launch `a` (8-bit rows, `block` threads) take a masked form of the matrix sweep under the index's options?
bool scan_takes_masked_form(const szg_index *ix, const szg::ScanArgs &a, int block);
// the sketch pre-pass: the sweep runs over a sketch shard, its merged lists are re-ranked on the float32 rows of the
// shard it stands for, together with `extra` more rows per query that the caller has uploaded behind each list in
// c->d_sent (kp + extra entries per query)
struct RerankOn {
    const szg_index *ix;
    const Shard *sh;
    int extra;  // entries behind each list: the drop bound's slot, then the staged rows
    int list;   // option sketch_list: the sweep's per-wave / per-block list length (0 = automatic, >= kp = kp)
    bool wide;  // the call takes wide batches: launches hold up to szg::kMatrixWideQueries queries where the matrix
                // sweep's two-block form serves them (sketch_wide_serves), up to queries_per_launch elsewhere
    bool share = false;  // ... and shared batches: a batch of 33 .. szg::kMatrixShareQueries queries is ONE launch of the
                         // shared form where it serves (sketch_share_serves)
};
// the index as sketch_plan.h sees it: sk's rows and options, ix's sketch_list and query_batch (ix: the handle whose
// sketch index sk is; a plain handle's one-sweep batches: ix = sk)
SketchShape sketch_shape(const szg_index *ix, const szg_index *sk);
// sketch_plan.h's questions of the same names on shard `sh` of sketch index `sk`, at the geometry of its plain sweep
// (kp = 0: the collect form, list_opt is not read)
bool sketch_wide_serves(const szg_index *sk, const Shard *sh, int kp, int list_opt);
bool sketch_share_serves(const szg_index *sk, const Shard *sh, int kp, int list_opt);
int enqueue_topk(szg_index *ix, Shard *sh, Ctx *c, int kp, int nq, bool has_allow, const RerankOn *on = nullptr);
// candidates of staged query `slot` from a finished top-k pass and *lb, the lower bound of the real-number key of every
// eligible row of the shard that is not among them
void gather_topk(const szg_index *ix, const Shard *sh, const Ctx *c, const QMeta &m, int slot, std::vector<Cand> *cands,
                 double *lb);
// float64 distances of the staged sentinel rows (Sentinels::Staged, d_sent) on `stream`, results to h_sent_out
int launch_sentinel_rerank(szg_index *ix, Shard *sh, Ctx *c, int nq, hipStream_t stream);
int finish_timing(szg_index *ix, Ctx *c);
// the rows of `rows` (index-level) that fall into the shard: how many, and shard-local to out[] (null: only counted)
size_t rows_in_shard(const Shard *sh, const std::vector<uint64_t> &rows, uint64_t *out);
// the k result slots of query qi of a call (rows + row_base; unused slots UINT64_MAX / 0.0)
void emit_topk(const szg_index *ix, const std::vector<HeapItem> &res, int k, int qi, uint64_t *out_rows, double *out_dist,
               int32_t *out_count);
// the end of a call's stage(): host time of the preparation [t_prep0, t_enq0) and of the enqueueing [t_enq0, now)
void note_stage_times(szg_index *ix, double t_prep0, double t_enq0);
int run_collect(szg_index *ix, Shard *sh, Ctx *c, int slot, float thr_key, bool has_allow, std::vector<Cand> *cands,
                const CertTag *tag = nullptr);
// fraction of the shard's rows that staged query `slot` may visit (tombstones, and its filter mask: the exact count of
// a resident mask, a sample of the words of one that came from the host)
double mask_pass_rate(const Shard *sh, const Ctx *c, bool has_allow, int slot);
void first_eligible_rows(const szg_index *ix, const uint64_t *allow, int k, std::vector<uint64_t> *rows_out);
int search_topk_impl(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                     uint64_t *out_rows, double *out_dist, int32_t *out_count,
                     const uint64_t *const *allow_ptrs = nullptr, const szg_mask *const *handles = nullptr,
                     const int *trace_index = nullptr);
// (trace_index: the queries' indexes in the caller's call, for the certificate trace of a call made on its behalf)
// consider()'s top-k branch over every row of the handle in visit order, continuing the heap *h (rows + row_base)
int replay_rows_into_heap(szg_index *ix, const double *query, const uint64_t *allow, int k, GoHeap *h);

// ---- scan_radius.cpp
// radius searches for a batch of queries (own radius and filter mask each): results[i] = the hits of query i, ascending
// (trace_index: the queries' indexes in the caller's call, for the certificate trace of a call made on its behalf)
int search_radius_impl(szg_index *ix, const double *queries, int n_queries, const double *radii,
                       const uint64_t *const *masks, std::vector<std::vector<HeapItem>> *results,
                       const szg_mask *const *handles = nullptr, const int *trace_index = nullptr);
// the one entry of every radius search: through the sketch (option sketch_radius) where the queries would each take a
// sweep of their own and the sketch applies to the handle, else search_radius_impl
int search_radius_any(szg_index *ix, const double *queries, int n_queries, const double *radii,
                      const uint64_t *const *masks, std::vector<std::vector<HeapItem>> *results,
                      const szg_mask *const *handles = nullptr);

// ---- scan_sketch_topk.cpp
// Top-k of large k through the sketch (option sketch_topk_collect): does the sample plan serve every shard of the
// handle's sketch index for k (sample_plan.h)?  Called with the sketch in sync.
bool sketch_topk_collect_serves(const szg_index *ix, int k);
// ... and the call itself: a sample pass, the radius it implies, the collect core at that radius, the reference's heap
// replayed over what was collected; the queries it does not settle go to search_topk_impl as ONE call
int search_topk_collect(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                        uint64_t *out_rows, double *out_dist, int32_t *out_count, const uint64_t *const *allow_ptrs,
                        const szg_mask *const *handles);

#ifndef SZG_BF16_8BIT_DEFAULT
#define SZG_BF16_8BIT_DEFAULT 1  // tiled 8-bit rows take the bfloat16 sweep for top-k batches (SZG_BF16_8BIT=0: the int8 sweep)
#endif
// ---- scan_mq.cpp
// the shard's resident row norms are complete (16-bit rows; no-op otherwise): called before a shared sweep is enqueued
int ensure_row_norms(szg_index *ix, Shard *sh);
// ... and the grouped one-sweep launches (8-bit rows): the shard's complete norm array, or null -- norms switched off
// (scan_norms = 1, SZG_NO_ROW_NORMS), no array (its allocation failed: no error, the sweep sums the norms itself).
// *err: any other failure of ensure_row_norms (a launch, a stream), which the caller returns
const float *scan_row_norms(szg_index *ix, Shard *sh, int *err);
// (rerun: the fused selection of this batch overflowed on this context -- again, through the score matrix)
int enqueue_topk_mq(szg_index *ix, Shard *sh, Ctx *c, int kp, int kp_wide, int nq, int nb, bool has_allow,
                    bool rerun = false);

// the batch's tail will compute the sentinel rows' distances itself (stage them, do not launch their own rerank)
bool mq_tail_takes_sentinels(const szg_index *ix, const Shard *sh, int kp, int kp_wide, int nq, int nb);
// radius batches: ONE shared sweep collects every (query, row) pair at or below the query's key threshold
// (thr[q], host) into c->d_collect (cap entries per query, counts in c->d_count)
int enqueue_collect_mq(szg_index *ix, Shard *sh, Ctx *c, int nq, int nb, bool has_allow, const float *thr, size_t cap);

// ---- scan_sketch.cpp
bool sketch_applies(const szg_index *ix, int k);
// ... without the clause on k: float32 rows (float64 under sketch_f64 = 1), the row count rule, the steps aside (radius
// searches: sketch_radius)
bool sketch_applies_rows(const szg_index *ix);
// the sketch index brought up to date under sk_mu, as a search needs it.  Auto mode never turns a working handle into
// an error: a failed sync gives back what was built and sets sk_nomem (the caller looks at sk_disabled / sk_nomem)
int sketch_sync_for_search(szg_index *ix);
// a load / synth: auto mode may try the sketch again (mutations are never concurrent with searches)
void sketch_rearm(szg_index *ix);
// test hooks (szg_debug_sketch_info / szg_debug_sketch_rows): the sketch state as it stands, under sk_mu, never a sync
int sketch_debug_info(szg_index *ix, szg_sketch_info *out, uint64_t *out_exc_rows, uint64_t exc_capacity);
int sketch_debug_rows(szg_index *ix, uint64_t first_row, uint64_t n_rows, uint8_t *out, uint64_t *out_live_words,
                      uint64_t live_capacity);
int search_topk_any(szg_index *ix, const double *queries, int n_queries, int k, const uint64_t *allow_bits,
                    uint64_t *out_rows, double *out_dist, int32_t *out_count,
                    const uint64_t *const *allow_ptrs = nullptr, const szg_mask *const *handles = nullptr);

// ---- scan_mask.cpp
// an empty mask shaped after the handle's shards, its device words allocated (not yet written); *out is set even on
// failure (mask_free it)
int mask_alloc(szg_index *ix, szg_mask **out);
void mask_free(szg_mask *m);  // null is fine
struct MaskGuard {  // frees a mask under construction on every exit path but the successful one
    szg_mask *m = nullptr;
    ~MaskGuard() { mask_free(m); }
    szg_mask *release()
    {
        szg_mask *r = m;
        m = nullptr;
        return r;
    }
};
// SZG_OK, or SZG_E_INVALID when the mask belongs to another handle or was made before the row count last changed
int mask_check(const szg_index *ix, const szg_mask *m);
const uint64_t *mask_host_words(const szg_mask *m);                 // index-level, ceil(rows / 64) words
const uint64_t *mask_shard_words(const szg_mask *m, size_t shard);  // device, shard-local (an even number of words)
uint64_t mask_shard_count(const szg_mask *m, size_t shard);         // rows of the shard the mask allows, exact
// szg_search_topk_masked up to the combiner (scan_api.cpp): the checks, and the search itself unless the call is a lone
// query that may be coalesced -- then *lone is its mask and nothing has been searched yet
int search_topk_masked_prepare(szg_index *ix, const double *queries, int n_queries, int k, const szg_mask *const *masks,
                               int n_masks, uint64_t *out_rows, double *out_dist, int32_t *out_count, const szg_mask **lone);
// words per slot of a batch's d_allow when resident masks are gathered into it (16-byte pairs)
inline size_t mask_slot_words(uint64_t n_rows) { return (size_t)(((n_rows + 63) / 64 + 1) & ~1ull); }
inline size_t mask_slot_words(const Shard *sh) { return mask_slot_words(sh->n_rows); }
// words of a mask with one bit per row (no padding): the host copy of a mask, a shard's slice of it
inline size_t index_words(uint64_t rows) { return (size_t)((rows + 63) / 64); }

// ---- scan_column.cpp
int stale_column();  // SZG_E_INVALID, "stale column: ..."
// the checks every call on a column but rows / read / destroy makes first: made at the handle's column epoch, one part
// per shard (stale_column otherwise); and SZG_E_INVALID, "the column's kind does not match the call"
int column_check(const szg_column *c);
int kind_mismatch();
// a valid, complete column of ix (SZG_E_INVALID otherwise: another handle's, stale, or short of the handle's rows)
int column_complete_check(const szg_index *ix, const szg_column *c);
// room for `need` rows in a part / for `used` bytes in its text heap: a bigger allocation with the old contents carried
// over, or -- a part that starts empty -- what a freshly created column has (column_str.h has the sizes).  zeroed ==
// false: the caller writes every byte of a new heap itself
int part_reserve(const szg_column *c, szg_column::Part &p, uint64_t need);
int heap_reserve(szg_column::Part &p, uint64_t used, bool zeroed = true);

// ---- scan_column_carry.cpp: the columns a compaction / reorder carries (scan_reorder.cpp calls these in this order)
// the new parts of the carried columns until the switch; what has not been handed to its column goes with this
struct CarriedColumns {
    std::vector<szg_column *> cols;
    std::vector<std::vector<szg_column::Part>> parts;  // [column][shard]
};
// every entry is a valid, complete column of ix; *out takes each once
int column_carry_check(szg_index *ix, szg_column *const *columns, int n_columns, std::vector<szg_column *> *out);
// new row first[d] + i of shard d (counts[d] rows) = old row src[first[d] + i] (index-level): every allocation, launch
// and check; the columns and the handle are untouched.  d_src: the whole list where the rows' move left it resident on
// the device of a handle of one shard (it is not uploaded again), else null
int column_carry_build(szg_index *ix, const std::vector<uint64_t> &src, const uint64_t *d_src, const std::vector<uint64_t> &counts,
                       const std::vector<uint64_t> &first, const std::vector<szg_column *> &cols, CarriedColumns *out);
// the old parts are freed, the new ones handed over, the columns valid at `epoch` with `rows` rows: nothing here fails
void column_carry_switch(CarriedColumns *cc, uint64_t rows, uint64_t epoch);

// One link of the shard's scan chain: under chain_mu, launch(st) puts the sweeps onto the shard's scan stream behind the
// batch's uploads (ev_up, recorded on the work stream by the caller), and `after` goes on once they are done.  With
// timing on the sweeps sit between an event pair (part 1: the early part's own) and count as n launches.  `what`
// names the launch in the error text.
template <class Launch>
int chain_sweeps(szg_index *ix, Shard *sh, Ctx *c, hipStream_t after, int part, int n, const char *what, Launch &&launch)
{
    std::lock_guard<std::mutex> lk(sh->chain_mu);
    hipStream_t st = ix->serialize_scans ? sh->scan_stream : c->pass.work;
    if (st != c->pass.work) {
        SiteScope t_(1);
        HIPCHK(hipStreamWaitEvent(st, c->ev_up, 0));
    }
    if (ix->timing) {
        SiteScope t_(2);
        HIPCHK(hipEventRecord(part ? c->ev_p0 : c->ev_scan0, st));
    }
    {
        SiteScope t_(3);
        const hipError_t e = launch(st);
        if (e != hipSuccess) return fail(SZG_E_DEVICE, what, e);
    }
    if (ix->timing) {
        SiteScope t_(4);
        HIPCHK(hipEventRecord(part ? c->ev_p1 : c->ev_scan1, st));
        (part ? c->pass.timed_part_n : c->pass.timed_n) = n;
    }
    if (st != after) {
        SiteScope t_(5);
        // (with timing on, the event just recorded behind the sweeps marks the same point of the stream: one packet
        // less between two batches' sweeps)
        hipEvent_t done = ix->timing ? (part ? c->ev_p1 : c->ev_scan1) : c->ev_scan_done;
        if (!ix->timing) HIPCHK(hipEventRecord(done, st));
        HIPCHK(hipStreamWaitEvent(after, done, 0));
    }
    return SZG_OK;
}

struct CtxGuard {  // returns a borrowed context on every exit path
    Shard *sh;
    Ctx *c;
    ~CtxGuard() { ctx_release(sh, c); }
};

// ---- the batch pipeline of a search call (top-k and radius; scan_topk.cpp) ----------------------------------------
//
// A call's queries travel in batches (up to 16 with one sweep each, or up to 96 sharing one sweep), as many in flight
// as the shards have free contexts: a batch is planned (plan_batch), borrows one context per shard, is staged (its
// queries prepared once, uploaded and its sweeps enqueued on every shard) and finished in order (run_batches).

// the filter masks of a call's queries: one pointer per query (null = unfiltered), or masks back to back with one
// bit per row of the index, or resident masks (one handle per query, null = unfiltered), or none.  operator() gives
// the host words in every case (a handle keeps a host copy of its words)
struct QueryMasks {
    const uint64_t *bits;
    const uint64_t *const *ptrs;
    const szg_mask *const *handles;
    size_t stride = 0;  // words per mask of `bits`
    QueryMasks(const szg_index *ix, const uint64_t *bits_, const uint64_t *const *ptrs_,
               const szg_mask *const *handles_ = nullptr)
        : bits(bits_), ptrs(ptrs_), handles(handles_)
    {
        uint64_t total_rows = 0;
        for (const Shard *sh : ix->shards) total_rows += sh->n_rows;
        stride = (total_rows + 63) / 64;
    }
    const szg_mask *handle(int qi) const { return handles ? handles[qi] : nullptr; }
    const uint64_t *operator()(int qi) const
    {
        if (handles) return handles[qi] ? mask_host_words(handles[qi]) : nullptr;
        if (ptrs) return ptrs[qi];
        return bits ? bits + (size_t)qi * stride : nullptr;
    }
};

// one batch of a call: queries [first, first+nq) and the contexts it has borrowed
struct Batch {
    szg_index *ix = nullptr;     // owner of the contexts
    int first = 0, nq = 0;
    int nb = 0;                  // > 0: the batch shares one sweep (query blocks of 16)
    bool single = false;         // the whole call is this one batch (a short call)
    int ctx_limit = 0;           // > 0: contexts come from the shards' first ctx_limit (one_sweep_contexts)
    int early_n = 0;             // ... whose first early_n queries' tail runs beside its last sweeps (Pass::early_n;
                                 // settled by acquire: 0 unless the batch runs on the scan stream)
    bool any_mask = false;       // some query of the batch carries a filter mask
    bool failed = false;         // enqueueing failed part-way: drain and release only
    std::vector<Ctx *> ctx;      // one per shard (null: the shard is empty)
    Batch() = default;
    Batch(Batch &&) = default;
    Batch(const Batch &) = delete;
    Batch &operator=(const Batch &) = delete;
    // a batch dropped with contexts still attached (a failure, an exception unwinding the call) drains and returns
    // them, so later calls do not wait for contexts that never come back
    ~Batch() { drain(); }
    bool acquire(bool may_block);  // one context per non-empty shard; false (holding none) if one is not free
    void release();
    void drain();                  // wait for the contexts' streams, then release
    // the filter masks of the batch's queries (sets any_mask)
    std::vector<const uint64_t *> masks(const QueryMasks &mask_of);
    // ... and their resident masks (empty when the call carries none)
    std::vector<const szg_mask *> handles(const QueryMasks &mask_of) const;
};

// the next batch of a call of n_queries, from query q0; nb = the query blocks of a shared sweep (0: one sweep per query)
// (sketch_plan.h: the rules, a one-sweep batch's size and a short call's early tail)
void plan_batch(szg_index *ix, int n_queries, int q0, int nb, const BatchRules &r, Batch *b);

// Prepare the batch's queries q[0, nq) ONCE on its first context -- the single-query form (swizzled floats / digit
// planes) for a batch of one sweep per query, the integer queries of the int8 shared sweep when int_planes -- and copy
// the forms and constants to the other shards' contexts.  adjust(j, meta): the caller's touches on query j's constants
// before they are copied.
int stage_query_forms(szg_index *ix, Batch &b, const double *q, bool int_planes,
                      const std::function<void(int, QMeta &)> &adjust);
// query j of a shared-sweep batch in the single-query kernels' form, built only when it is needed (an escalation, a
// radius query that overflows the batch's buffers): prepared once, uploaded on every shard's `work` stream;
// *meta = its constants
int stage_single_form(szg_index *ix, Batch &b, const double *q, int j, QMeta *meta);

// ---- scan_sketch.cpp: what a call through ix's sketch index -- the top-k pre-pass, a radius search -- fixes up front
struct SketchPlan {
    double gs = 0.0;     // Euclidean: sketch distances are in units of gs (the sketch sweeps see q / gs); 0: cosine
    double slack = 0.0;  // sketch_slack (sketch_bound.h) of the largest d(row, its sketch) the build measured
    int wide = 0;        // the call takes wide batches (32 queries, one launch of the two-block matrix sweep each):
                         // 1 = under the automatic rule, 2 = forced (option sketch_wide = 2)
    int share = 0;       // the call takes shared batches (up to 64 queries, one shared launch each; top-k calls only):
                         // 1 = under the automatic rule, 2 = forced (option sketch_share = 2)
};
// (kp: what sketch_wide_serves is asked with -- 0: a collect call)
SketchPlan sketch_call_plan(const szg_index *ix, int n_queries, int kp);
// the next batch of such a call, from query q0, on the sketch index's contexts
void sketch_plan_batch(const szg_index *ix, int n_queries, int q0, int wide, Batch *b, int share = 0);
// ... and its queries q[0, nq) in the forms the sketch sweeps take: scaled as sketch_scale_query scales them -- zeros in
// the slots marked handed (null: none is) -- into *scratch, which the call keeps between its batches, then
// stage_query_forms on sketch index sk with the caller's adjust
int sketch_stage_forms(szg_index *sk, double gs, Batch &b, const double *q, const uint8_t *handed, std::vector<double> *scratch,
                       const std::function<void(int, QMeta &)> &adjust);
// float32 shard a's rows without a usable sketch (sk_exc): f(shard-local row, eligible: live and allowed by mask words m)
template <class F>
void sketchless_rows(const szg_index *ix, const Shard *a, const uint64_t *m, F &&f)
{
    for (uint64_t r : ix->sk_exc) {
        if (r < a->first || r >= a->first + a->n_rows) continue;
        const uint64_t l = r - a->first;
        f(l, ((a->live_host[l >> 6] >> (l & 63)) & 1) && (!m || ((m[r >> 6] >> (r & 63)) & 1)));
    }
}
// the queries such a call hands over (redo, ascending), gathered for ONE call of the full-precision path: their
// vectors, and their masks in the form the caller's came in (pointers or resident handles; null: none is filtered)
struct HandedOver {
    std::vector<double> q;
    std::vector<const uint64_t *> masks;
    std::vector<const szg_mask *> handles;
    bool any = false;
    HandedOver(const szg_index *ix, const double *queries, const QueryMasks &mask_of, const std::vector<int> &redo)
        : q(redo.size() * (size_t)ix->dim), masks(redo.size()), handles(mask_of.handles ? redo.size() : 0)
    {
        for (size_t i = 0; i < redo.size(); i++) {
            memcpy(&q[i * ix->dim], queries + (size_t)redo[i] * ix->dim, sizeof(double) * ix->dim);
            masks[i] = mask_of(redo[i]);
            if (!handles.empty()) handles[i] = mask_of.handles[redo[i]];
            any |= masks[i] != nullptr;
        }
    }
    const uint64_t *const *mask_ptrs() const { return handles.empty() && any ? masks.data() : nullptr; }
    const szg_mask *const *handle_ptrs() const { return !handles.empty() && any ? handles.data() : nullptr; }
};
// ... for a top-k call: search_topk_impl on them, traced under their indexes in the caller's call, and their answers
// into the caller's arrays
int search_topk_handed(szg_index *ix, const HandedOver &h, const std::vector<int> &redo, int k, uint64_t *out_rows,
                       double *out_dist, int32_t *out_count);

// The entry frame of every search through the sketch (the top-k pre-pass, top-k of large k, radius searches).  call: the
// pipeline -- run() answers what it settles and leaves the rest in redo; its sk is set here, once the sketch is in sync.
// serves(): the caller's further condition on the synced sketch.  whole(): the full-precision path on the whole call --
// where the sketch has stepped aside or does not serve (the path the call takes without it: not a fallback, not
// counted), and in auto mode after a failure inside the pipeline (an allocation of a sketch context, say): the sketch
// index then stays until the next load and steps aside (sk_nomem).  handed(h, redo): ONE call of the full-precision path
// on the queries handed over, redo as its trace index, and their answers scattered back.  (Only the pre-pass's
// hand-overs enter the automatic window sk_hist: SketchCall::finish counts them.)
template <class Call, class Serves, class Whole, class Handed>
int sketch_served_call(szg_index *ix, Call &call, Serves &&serves, Whole &&whole, Handed &&handed)
{
    int rc = sketch_sync_for_search(ix);
    if (rc) return rc;
    if (ix->sk_disabled || ix->sk_nomem || !serves()) return whole();
    call.sk = ix->sketch;
    rc = call.run();
    if (rc && ix->sketch_on == 2) {
        ix->sk_nomem = true;
        return whole();
    }
    if (rc || call.redo.empty()) return rc;
    std::sort(call.redo.begin(), call.redo.end());
    return handed(HandedOver(ix, call.queries, call.mask_of, call.redo), call.redo);
}

// The in-flight loop of a call: plan a batch, borrow its contexts (none free: finish the oldest batch in flight
// first), stage it, and in the end finish the rest in order.  hand_over (optional): takes every staged batch instead
// (a finisher thread: acquire then blocks until it gives contexts back); false once that thread has failed.
template <class B, class Call>
int run_batches(Call &call, const std::function<bool(B &&)> &hand_over = nullptr)
{
    std::deque<B> inflight;
    int rc = SZG_OK;
    for (int q0 = 0; q0 < call.n_queries && rc == SZG_OK;) {
        B b = call.plan(q0);
        if (!b.acquire(hand_over || inflight.empty())) {  // no free context: finish the oldest batch first
            rc = call.finish(inflight.front());
            inflight.pop_front();
            continue;
        }
        rc = call.stage(b);
        b.failed = rc != SZG_OK;  // nothing to gather: finish() only drains and releases
        q0 += b.nq;
        if (!hand_over) inflight.push_back(std::move(b));
        else if (!hand_over(std::move(b))) break;
    }
    while (!inflight.empty()) {
        const int r2 = call.finish(inflight.front());
        if (rc == SZG_OK) rc = r2;
        inflight.pop_front();
    }
    return rc;
}

// The second host thread of a long call: it takes the staged batches in order and finishes them -- waits, candidate
// assembly, certification, output, release of the contexts -- while the calling thread prepares and enqueues.  The
// hand-over is the batch queue; contexts are the flow control (acquire blocks until the finisher has released one).
template <class B>
struct Finisher {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<B> q;
    bool done = false;
    int rc = SZG_OK;
    std::string err;
    std::atomic<bool> failed{false};
    std::thread th;
    // start the thread; finish(B &) settles one batch.  false: no thread to be had, the caller does both
    bool start(std::function<int(B &)> finish)
    {
        try {
            th = std::thread([this, finish] {
                for (;;) {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return !q.empty() || done; });
                    if (q.empty()) return;
                    B t(std::move(q.front()));
                    q.pop_front();
                    lk.unlock();
                    int r;
                    try {
                        r = finish(t);
                    } catch (const std::bad_alloc &) {
                        r = fail(SZG_E_NOMEM, "out of host memory");
                    } catch (...) {
                        r = fail(SZG_E_DEVICE, "unexpected exception");
                    }
                    if (r != SZG_OK && !failed.load()) {  // (every batch is still finished: its contexts go back)
                        rc = r;
                        err = szg_last_error();
                        failed.store(true);
                    }
                }
            });
        } catch (...) {
            return false;
        }
        return true;
    }
    // run_batches' hand_over
    std::function<bool(B &&)> hand_over()
    {
        return [this](B &&t) {
            {
                std::lock_guard<std::mutex> lk(mu);
                q.push_back(std::move(t));
            }
            cv.notify_one();
            return !failed.load();
        };
    }
    void stop()
    {
        if (!th.joinable()) return;
        {
            std::lock_guard<std::mutex> lk(mu);
            done = true;
        }
        cv.notify_one();
        th.join();
    }
    // join, and the call's result: the caller's own rc, else the finisher's first failure (in this thread's last-error slot)
    int join(int rc_caller)
    {
        stop();
        if (rc_caller == SZG_OK && failed.load()) return fail(rc, err.c_str());
        return rc_caller;
    }
    ~Finisher() { stop(); }  // (an exception unwinding the call: the queued batches are still finished first)
};

}  // namespace szgi
