// options.h -- the run-time options of a handle (szg_set_option; include/syzgy_scan.h documents them): the members
// that hold them, with their defaults, and ONE table with a row per option -- its name, the values it accepts, how an
// accepted value is stored, the text of a refusal, whether szg_debug_option_check knows it and whether the internal
// sketch index follows it.  Plain C++, no HIP (tests/cpp/test_options.cpp); the rows are options.cpp's, out of line,
// and evaluated there alone: scan_group_ring's depends on SZG_GROUP_RING_ALT, and a variant build rebuilds only the
// objects it names.
#pragma once
#include <cstddef>
#include <cstdint>

namespace szgi {

constexpr int kMaxBatch = 96;  // queries one batch may stage (szg::kMqMaxQueries: a bfloat16 shared sweep)
constexpr uint64_t kCarryStageMax = 64ull << 20;  // the largest carry_stage_bytes: column_carry.h's kCarryStageBytes, a
                                                  // header of HIP's qualifiers (scan_handle.cpp holds the two equal)

// What szg_set_option writes.  szg_index derives from it: every read is ix->name, as before.
struct Options {
    int sketch_on = 2;                   // ("sketch") 0 off, 1 forced on, 2 auto (sketch_applies)
    int sketch_extra = 30;               // sketch neighbours asked for beyond k: k = 10 -> 40, which keeps the sketch
                                         // sweep's lists in registers (kp <= 64); the pre-pass serves k <= 34
    int sketch_min_rows = 4096;          // smaller collections are not worth a second index
    int sketch_list = 0;                 // the sketch sweep's per-wave / per-block list length (0 = automatic, >= kp:
                                         // kp, the full lists and the two-level merge)
    int slack_min = 16;       // ("slack")
    int query_batch = 16;     // queries per scan launch
    int radius_mq = 1;        // radius batches of 2+ queries share one sweep of the corpus (the shared sweeps' collect form)
    int finish_thread = 1;    // shared-sweep calls of 3+ batches: a second host thread assembles the finished batches
                              // while the caller's prepares and enqueues the next ones (0 = one thread does both)
    int queries_per_launch = 16;  // sweeps one scan launch walks back to back (query-major)
    int scan_group = 0;       // queries of a launch the one-sweep kernel scores per row read, where the launch qualifies
                              // (8-bit rows, top-k, no masks, lists in registers): 0 = automatic, 1, 2 or 4
    int scan_group_ring = 0;  // ring depth of the grouped row-shape kernels that exist at two: 0 = automatic, or one of the
                              // depths the library carries (szg::scan_group_ring_known)
    int scan_norms = 0;       // grouped one-sweep launches take the rows' norms from the resident array (ensure_row_norms):
                              // 0 = automatic, 1 = always sum them in the sweep
    int sketch_planes = 0;    // digit planes of a query prepared for a sketch sweep: 0 = automatic (2, |Q| <= 16000),
                              // 3 = the plain 8-bit handles' (|Q| <= 10^6).  Only is_sketch indexes read it (scan_planes):
                              // only queries are prepared differently, nothing resident depends on it.
    int sketch_matrix = 0;    // the matrix sweep (kernels_scan_mx.hip) for one-sweep launches that qualify -- tiled 8-bit rows,
                              // two-plane queries, resident norms, no masks, scan_group = 0: 0 = automatic (launches of
                              // szg::kMatrixMinQueries queries or more), 1 = never, 2 = every such launch
    int sketch_select = 0;    // the matrix sweep's selection: 0 = automatic (row lists where the lists hold at most
                              // szg::kRowListMax entries), 1 = the serial inserts everywhere
    int sketch_wide = 0;      // the matrix sweep's two-block form (32 queries per row read): 0 = automatic (calls of
                              // kWideCallMin one-sweep queries on, under the default query_batch and queries_per_launch),
                              // 1 = never, 2 = every call of more than 16 queries where the shape allows
    int sketch_share = 0;     // the matrix sweep's shared form (64 queries per launch, paired blocks walk the same rows):
                              // 0 = automatic (calls of kShareCallMin one-sweep queries on, under the default query_batch
                              // and queries_per_launch), 1 = never, 2 = every sketch call of more than 32 queries, in
                              // batches of up to 64 from its first query on
    int sketch_bulk = 0;      // the row lists' whole-tile merge: 0 = automatic (tiles with szg::kBulkMin passing pairs or more),
                              // 1 = never (rounds only), n >= 2 = tiles with n passing pairs or more
    int sketch_radius = 0;    // radius queries that would each take a sweep of their own (a lone query, radius_mq = 0) go
                              // through the sketch where it applies to the handle: 0 = never (the default: the option
                              // soaks, as the top-k pre-pass did, before a later change makes it automatic), 1 = always
    int sketch_masked = 0;    // top-k launches of the sketch pre-pass with tombstones or filter masks take the matrix sweep's
                              // masked forms wherever the same launch without masks would take the matrix sweep: 0 = never
                              // (the default while the option soaks: masked launches keep the one-query kernel), 1 = always
    int sketch_f64 = 0;       // float64 handles (the reference's default quantization) keep an 8-bit sketch too, an eighth of
                              // their rows' bytes, under every rule of float32 handles: 0 = never (the default while the
                              // option soaks: such a handle keeps no sketch and allocates nothing more), 1 = always.  Read on
                              // the handle whose rows are float64 (sketch_applies_rows); the sketch index carries it unread.
    int sketch_topk_collect = 0;  // top-k calls that take a sweep per query with a k the pre-pass does not serve go through
                              // the sketch as a sample pass and a collect sweep (scan_sketch_topk.cpp, SketchTopkCall): 0 = never
                              // (the default while the option soaks), 1 = wherever the sample plan serves every shard.  Read
                              // on the handle the call is made on (search_topk_any); the sketch index carries it unread.
    int query_prep = 0;       // the batches of a top-k call through the sketch have their queries prepared on the card
                              // (kernels_query_prep.hip) instead of by prep_query: 0 = never (the default while the option
                              // soaks), 1 = batches of kQueryPrepMin queries or more, 2 = every batch (query_prep_serves).
                              // Read on the handle the call is made on (SketchCall::stage); the sketch index carries it unread.
    int tie_mode = 0;         // 0: exact full replay on ties/NaN, 1: keep the fast answer
    int serialize_scans = 1;  // scan launches of a shard never overlap each other
    int multi_query = 1;      // share one sweep between the queries of a batch (MFMA path)
    int mask_dense = 1;       // masked sweeps whose masks pass most rows use the dense phase
    int coalesce = 1;         // concurrent single-query calls share sweeps (see Combiner)
    int mq_min = 2;           // smallest batch worth a shared sweep (measured: 2 queries already break even)
    int mq_hits = 1024;       // fused selection: candidates per query the full sweep is expected to collect
                              // (sets the prefix: n_rows * kp / mq_hits rows)
    // test hooks: paths that occur by themselves only on particular data
    int force_escalate = 0;   // treat every first pass as uncertified
    int force_matrix = 0;     // shared sweeps: the score-matrix form (what an overflowing candidate buffer falls back to)
    int force_no_refine = 0;  // shared sweeps: the batch's tail as separate re-score / select / rerank launches (kp > 256)
    int force_sketch_nomem = 0;  // the sketch's device allocation is refused (auto mode steps aside)
    uint64_t carry_stage_bytes = 0;  // a carried column's staging window between two parts; 0 = kCarryStageBytes
                              // (pieces of 16 bytes travel, so a window is a multiple of 16)
};

// How a row stores an accepted value: as it is; value != 0 (these rows accept every value); min(value, 2^30);
// carry_stage_bytes, the one 64-bit member; and "contexts", which is no member but the contexts in rotation per shard:
// the handle applies it (scan_handle.cpp) and holds it against its n_ctx -- a constant, so no row's acceptance
// depends on another row's value.
enum class OptionStore { kInt, kBool, kClamp30, kBytes, kContexts };

struct OptionRow {
    const char *name;
    int Options::*member;        // null: kBytes, kContexts
    bool (*accepts)(int64_t);
    const char *refusal;         // the text of SZG_E_INVALID for a value that is not accepted
    OptionStore store;
    bool scan_check;             // szg_debug_option_check answers for it (the one-sweep kernel's options)
    bool forwarded;              // the internal sketch index follows it: set there too, replayed when that index is created
};

const OptionRow *option_rows(int *n);  // the table; at most 64 rows: the handle marks its forwarded rows that were set in one word
const OptionRow *option_find(const char *name);         // null: no such option
const OptionRow *option_of(int Options::*member);       // the row that stores into `member` (the plan hooks' arguments)
const char *option_refusal(const OptionRow *row, int64_t value);  // null: accepted
void option_store(const OptionRow *row, Options *o, int64_t value);  // an accepted value (kContexts: nothing)
int64_t option_load(const OptionRow *row, const Options &o);         // what is stored (kContexts: 0)

}  // namespace szgi
