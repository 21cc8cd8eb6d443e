// sketch_plan.h -- the plan of a search call whose queries take one sweep each, and of a call through the sketch above
// all: how the call splits into batches, a batch into parts and launches on one shard, which launches take the matrix
// sweep's wide or shared form, and how many passes over the rows that makes.  The launch path (scan_sketch.cpp,
// scan_topk.cpp, scan_radius.cpp, scan_sketch_topk.cpp) and the plan hooks (scan_api.cpp) both compute from here.  Plain C++, no HIP, header
// only -- what depends on the build's variants (scan_variant, scan_lds_bytes, merge_short_fits) is scan_plan.cpp's:
// tests/cpp/test_sketch_plan.cpp compiles the two on their own under the address and undefined-behaviour sanitizers.
#pragma once
#include <algorithm>
#include <vector>

#include "scan_plan.h"

namespace szgi {

// ---- the call's batches ---------------------------------------------------------------------------------------------

constexpr int kFirstBatch = 4;     // queries of a call's first (and last) one-sweep batch: the card starts sweeping sooner
constexpr int kShortCall = 32;     // calls of up to this many one-sweep queries are ONE batch on the scan stream
constexpr int kShortCallLast = 4;  // ... queries of which the tail is left for after the final sweep
// Wide batches of the sketch pre-pass (option sketch_wide = 0): a call takes batches of szg::kMatrixWideQueries queries,
// one launch each, from two of them between its first and last batch of kFirstBatch on -- below that a pipeline of
// 32-query batches has nothing to overlap with
constexpr int kWideCallMin = 2 * szg::kMatrixWideQueries + 2 * kFirstBatch;
// Shared batches (option sketch_share = 0): batches of szg::kMatrixShareQueries queries, one shared launch each, by the
// same rule -- from two of them between the first and last batch of kFirstBatch on.  Shorter calls keep their plan.
constexpr int kShareCallMin = 2 * szg::kMatrixShareQueries + 2 * kFirstBatch;

// Option query_prep = 1: batches of a sketch top-k call of at least this many queries have their queries prepared on the
// card.  Below it a launch and a copy of constants sit in front of the batch's few sweeps and buy back less host time
// than they cost: a lone search and the kFirstBatch-query edges of a long call stay on the host ("queries
// prepared on the card", has the measurement the value is from)
constexpr int kQueryPrepMin = 8;
// does the card prepare a batch of batch_queries queries under the option's value?  0 never, 1 from kQueryPrepMin on, 2 every
// batch (the tests' setting)
inline bool query_prep_serves(int option, int batch_queries)
{
    if (batch_queries < 1) return false;
    return option == 2 || (option == 1 && batch_queries >= kQueryPrepMin);
}

// How a call splits into batches: the caller's parameters
struct BatchRules {
    int batch;        // queries of a one-sweep-per-query batch
    int edge;         // ... of the call's first and last such batch
    int short_max;    // a call of up to this many one-sweep queries is ONE batch on the scan stream
    bool early_tail;  // ... whose first queries' tail runs beside its last sweeps
    bool radius;      // radius batches (mq_uses_i8)
};
// Queries of the batch that starts at query q0 of a call of n_queries with one sweep each.  A short call is one batch;
// a longer call's FIRST batch is small, so that the card starts sweeping after a few microseconds of preparation
// instead of a whole batch's (the next batch is prepared while it sweeps) ... and its LAST one too: what is left
// to do once the last sweep has ended is that batch's merges, re-rank, copy-back and result assembly
inline int one_sweep_batch_size(int n_queries, int q0, const BatchRules &r)
{
    const int left = n_queries - q0;
    if (q0 == 0 && n_queries <= r.short_max) return n_queries;
    int nq = std::min(r.batch, left);
    if (left > r.edge) {
        if (q0 == 0) nq = std::min(nq, r.edge);
        else if (left <= r.batch + r.edge) nq = left - r.edge;
    }
    return nq;
}
// The early tail of a short call (one batch on the scan stream: launches of <= 16 sweeps back to back, uploads ahead of
// them, no event on the critical path).  From 8 queries on, the merges, re-rank, copy-back and host assembly of its
// first early_n queries run on the context's own stream and the calling thread WHILE the last sweeps run; only the last
// few queries' tail is left after the final sweep.  0: the call runs in one part.
inline int short_call_early(int n_queries, const BatchRules &r, bool serialize_scans)
{
    if (!r.early_tail || !serialize_scans || n_queries > r.short_max || n_queries < 8) return 0;
    return n_queries - std::min(kShortCallLast, n_queries / 2);
}

// ---- the sketch index as the plan sees it ---------------------------------------------------------------------------

struct SketchShape {
    int bits;
    szg::RowMap map;
    bool tiled;
    int ring;
    bool no_shape_kernels;
    int scan_group, planes, scan_group_ring;
    int sketch_matrix, sketch_select, sketch_wide, sketch_share, sketch_masked;
    int sketch_list;         // option sketch_list: entries per wave and block list (0 = automatic, >= kp = kp)
    int query_batch;         // 1 .. kMaxBatch (the option's range)
    int queries_per_launch;
    bool norms = true;       // the rows' norms are resident (the library's sketch shards: always)
};

// what scan_variant decides from for one launch of a sweep over such rows: n_queries queries at `block` threads that
// keep lists of list_len entries (collect: none), with tombstones or filter masks (masked) or without
inline szg::ScanPlanIn sketch_plan_in(const SketchShape &s, int list_len, bool collect, bool masked, int n_queries, int block)
{
    szg::ScanPlanIn in{s.bits, s.map, s.tiled, list_len, collect, masked, s.ring, s.no_shape_kernels};
    in.group = s.scan_group;
    in.n_queries = n_queries;
    in.block = block;
    in.planes = s.planes;
    in.group_ring = s.scan_group_ring;
    in.matrix_opt = s.sketch_matrix;
    in.norms = s.norms;
    in.select_opt = s.sketch_select;
    in.wide_opt = s.sketch_wide;
    in.share_opt = s.sketch_share;
    in.masked_opt = s.sketch_masked;
    return in;
}
// passes over the rows that the launch makes: one per group of its queries (one per query where the launch does not
// qualify for groups); a shared launch counts one per column group, as requested -- what its second reader finds on the
// die is not taken off; a masked form counts as the unmasked launch of the form it takes
inline int launch_passes(const szg::ScanPlanIn &in)
{
    const int group = szg::scan_variant(in).group;
    return (in.n_queries + group - 1) / group;
}

// ---- one shard: a plain sweep over it takes `grid` blocks of `block` threads ----------------------------------------

// List length m of a sketch sweep over `grid` blocks (option sketch_list).  The query's kp best rows
// fall about kp / grid to a block; automatic lists hold twice that plus 8 (8 at 512 blocks), so a block rarely has
// more of them than its list keeps -- and when it has, the drop bound says so and the query falls back.  m >= kp (or
// lists the one-launch merge cannot hold): the full lists and the two-level merge.
inline int sketch_list_len(int want, int kp, int grid)
{
    const int m = want > 0 ? want : std::max(8, 2 * kp / std::max(grid, 1) + 8);
    if (m >= kp || !szg::merge_short_fits(grid, m, kp)) return kp;
    return m;
}
// The geometry of a shared launch on a shard whose plain sweep takes `grid` blocks: grid 2 S and S lists of m entries
// per query.  Everything that sizes or walks the lists of a shared launch reads S from here (szg::share_slices, as the
// kernel does).
struct ShareGeom {
    int grid, slices, m;
};
inline ShareGeom share_geometry(int grid, int list_opt, int kp)
{
    const int G = szg::share_grid(grid);
    const int S = szg::share_slices(G);
    return ShareGeom{G, S, sketch_list_len(list_opt, kp, S)};
}
// Does the matrix sweep's two-block form serve a launch of szg::kMatrixWideQueries queries on the shard, for calls that
// keep kp candidates per query (scan_variant's answer for that launch)?  kp = 0: the collect form (radius searches
// through the sketch; no lists).  has_dead: a top-k launch takes the masked form of the same shape under
// sketch_masked = 1 and is served exactly where the unmasked one is; a collect launch with masks never is.
inline bool sketch_wide_serves(const SketchShape &s, int grid, int block, bool has_dead, int kp)
{
    const bool collect = kp == 0;
    if (kp > 64) return false;
    const int m = collect ? 0 : sketch_list_len(s.sketch_list, kp, grid);
    return szg::scan_variant(sketch_plan_in(s, m, collect, has_dead, szg::kMatrixWideQueries, block)).wide != 0;
}
// ... and its shared form a top-k launch of 33 .. szg::kMatrixShareQueries queries: where the wide form serves the shard
// (asked with the plain launch's list length; the shared launch's S lists may be longer)
inline bool sketch_share_serves(const SketchShape &s, int grid, int block, bool has_dead, int kp)
{
    if (kp < 1 || !sketch_wide_serves(s, grid, block, has_dead, kp)) return false;
    const int m = share_geometry(grid, s.sketch_list, kp).m;
    return szg::scan_variant(sketch_plan_in(s, m, false, has_dead, szg::kMatrixShareQueries, block)).share != 0;
}

// ---- the call rule: which batches a call through the sketch takes --------------------------------------------------

// Wide batches (option sketch_wide): 32 queries, one launch of the two-block matrix sweep each.  served: every non-empty
// shard's launch of 32 qualifies (sketch_wide_serves), and there is one.  1 = automatic: long calls under the default
// batch and launch sizes; 2 = forced (sketch_wide = 2): every call of more than 16 queries.
inline int sketch_call_wide(const SketchShape &s, int n_queries, bool served)
{
    if (!served || s.sketch_wide == 1 || n_queries <= szg::kMatrixQueries) return 0;
    if (s.sketch_wide == 2) return 2;
    return n_queries >= kWideCallMin && s.query_batch == 16 && s.queries_per_launch == 16 ? 1 : 0;
}
// Shared batches (option sketch_share; top-k calls: kp >= 1): up to 64 queries, one shared launch each.  served: every
// non-empty shard's launch of 33 .. 64 qualifies (sketch_share_serves).  1 = automatic: long calls that take wide batches
// under the automatic rule (a rest of 17 .. 32 queries is a wide launch); 2 = forced: every call of more than 32 queries.
inline int sketch_call_share(const SketchShape &s, int n_queries, int kp, int wide, bool served)
{
    if (!served || kp < 1 || s.sketch_share == 1 || n_queries <= szg::kMatrixWideQueries) return 0;
    if (s.sketch_share == 2) return 2;
    return wide == 1 && n_queries >= kShareCallMin ? 1 : 0;
}
// the rules such a call splits by
inline BatchRules sketch_batch_rules(int n_queries, int wide, int share, int query_batch)
{
    // (a wide call is longer than kShortCall: first and last batch of kFirstBatch, 32 between them -- 64 in a shared call)
    BatchRules r{share ? szg::kMatrixShareQueries : (wide ? szg::kMatrixWideQueries : query_batch), kFirstBatch, kShortCall, true,
                 false};
    // forced: batches of up to 32 (64) from the call's first query on, no small edges, no early tail
    if (wide == 2) r = BatchRules{szg::kMatrixWideQueries, n_queries, szg::kMatrixWideQueries, false, false};
    if (share == 2) r = BatchRules{szg::kMatrixShareQueries, n_queries, szg::kMatrixShareQueries, false, false};
    return r;
}
// the batch sizes of a call of n_queries through the sketch (host arithmetic: the plan hooks and tests)
inline std::vector<int> sketch_batch_sizes(int n_queries, int wide, int share, int query_batch)
{
    std::vector<int> out;
    const BatchRules r = sketch_batch_rules(n_queries, wide, share, query_batch);
    for (int q0 = 0; q0 < n_queries;) {
        const int nq = std::max(1, one_sweep_batch_size(n_queries, q0, r));
        out.push_back(nq);
        q0 += nq;
    }
    return out;
}

// ---- one batch's top-k launches on one shard ------------------------------------------------------------------------

// The batch's nq queries go in one part -- or, for a short call (early > 0), two: the sweeps of queries [0, early), whose
// merges, re-rank and copy-back leave the scan stream for the context's own, and the last few queries, whose tail is all
// that is left to do after the call's final sweep.  Part 1 is that early part and launches first; part 0 the rest.
struct SketchLaunches {
    bool masks;   // the launches carry tombstones or filter masks ...
    bool masked;  // ... AND keep the one-query kernel; under sketch_masked = 1 they split and launch as the unmasked call
                  // of the same size does, and every launch that qualifies takes the matrix sweep's masked form
    bool share;   // 33 .. 64 queries in ONE launch of the shared form, on a grid of 2 S blocks that leaves S lists per query
    bool wide;    // launches of up to 32 queries where the two-block form serves them
    int matrix;   // the launches' sketch_matrix: a call with wide batches takes the matrix sweep whatever a launch's count
                  // -- a rest of one or two queries too -- so that a query's keys do not depend on where the batches'
                  // edges fall; a call that keeps more than 64 candidates per query -- lists that would not fit registers
                  // at full length -- stays with the grouped kernels even where its short lists would fit
    int qpl;      // queries per launch
    int grid, block;
    int lists0;   // block lists per query the sweeps leave
    int m;        // entries per wave and block list
    int nq, early;
    int first_part() const { return early ? 1 : 0; }
    int q0(int part) const { return part ? 0 : early; }
    int q1(int part) const { return part ? early : nq; }
    int n_launches(int part) const { return (q1(part) - q0(part) + qpl - 1) / qpl; }
    int count(int part, int start) const { return std::min(qpl, q1(part) - start); }  // of the launch that starts at query `start`
    // f(part, start, count) for every launch, in launch order
    template <class F>
    void each(F &&f) const
    {
        for (int part = first_part(); part >= 0; part--)
            for (int j = q0(part); j < q1(part); j += qpl) f(part, j, count(part, j));
    }
};
// sketch: the sweeps run over a sketch index (lists of m < kp entries where they can; wide and share: the call's,
// sketch_call_wide / sketch_call_share); false: a plain handle's one-sweep batch, full lists.
inline SketchLaunches sketch_batch_launches(const SketchShape &s, bool sketch, int grid, int block, int kp, int nq, int early,
                                            bool masks, int wide, int share)
{
    SketchLaunches l{};
    l.masks = masks;
    l.masked = masks && !(sketch && s.sketch_masked == 1);
    l.nq = nq;
    l.early = early > 0 && early < nq ? early : 0;
    l.grid = grid;
    l.block = block;
    l.lists0 = grid;
    l.m = sketch ? sketch_list_len(s.sketch_list, kp, grid) : kp;
    l.share = sketch && share && !l.masked && !l.early && nq > szg::kMatrixWideQueries && nq <= szg::kMatrixShareQueries &&
              sketch_share_serves(s, grid, block, masks, kp);
    if (l.share) {
        const ShareGeom sg = share_geometry(grid, s.sketch_list, kp);
        l.grid = sg.grid;
        l.lists0 = sg.slices;
        l.m = sg.m;
    }
    // (the same question the call asked before it planned wide batches)
    l.wide = sketch && (wide || share) && !l.masked && nq > szg::kMatrixQueries && sketch_wide_serves(s, grid, block, masks, kp);
    l.qpl = l.share ? szg::kMatrixShareQueries : (l.wide ? szg::kMatrixWideQueries : std::max(1, s.queries_per_launch));
    l.matrix = sketch && (wide || share) && s.sketch_matrix == 0 ? 2 : s.sketch_matrix;
    if (kp > 64) l.matrix = 1;
    return l;
}
// passes of the batch's launch of n queries
inline int sketch_launch_passes(const SketchShape &s, const SketchLaunches &l, int n)
{
    szg::ScanPlanIn in = sketch_plan_in(s, l.m, false, l.masks, n, l.block);
    in.matrix_opt = l.matrix;
    return launch_passes(in);
}

// A whole top-k call of n_queries through the sketch on one shard: its wide / share, its batches, launches and passes, as
// the functions above split it (what the plan hooks answer and the tests check; the library's walk is its pipeline)
struct SketchCallWalk {
    int wide, share, launches, passes;
    std::vector<int> batches;
};
inline SketchCallWalk sketch_call_walk(const SketchShape &s, int grid, int block, int kp, int n_queries, bool masks,
                                       bool serialize_scans)
{
    SketchCallWalk w{};
    // (a top-k call: kp = 0 would ask for the collect form)
    w.wide = sketch_call_wide(s, n_queries, kp >= 1 && sketch_wide_serves(s, grid, block, masks, kp));
    w.share = sketch_call_share(s, n_queries, kp, w.wide, sketch_share_serves(s, grid, block, masks, kp));
    const BatchRules r = sketch_batch_rules(n_queries, w.wide, w.share, s.query_batch);
    w.batches = sketch_batch_sizes(n_queries, w.wide, w.share, s.query_batch);
    int q0 = 0;
    for (const int nq : w.batches) {
        const int early = q0 == 0 ? short_call_early(n_queries, r, serialize_scans) : 0;
        const SketchLaunches l = sketch_batch_launches(s, true, grid, block, kp, nq, early, masks, w.wide, w.share);
        l.each([&](int, int, int n) {
            w.launches += 1;
            w.passes += sketch_launch_passes(s, l, n);
        });
        q0 += nq;
    }
    return w;
}

// ---- a batch's collect launches on one shard (radius searches through the sketch; the sample pass of a large-k top-k) --

// launches of 32 queries where the call takes wide batches, the batch may (ok: unmasked launches with resident norms;
// the sample pass: its two-block image fits LDS as well) and the collect form's two blocks serve the shard; else of
// per_launch
struct CollectLaunches {
    bool wide32;
    int qpl;
};
inline CollectLaunches sketch_collect_launches(const SketchShape &s, int grid, int block, bool has_dead, int wide, bool ok, int nq,
                                               int per_launch)
{
    const bool wide32 = wide && ok && nq > szg::kMatrixQueries && sketch_wide_serves(s, grid, block, has_dead, 0);
    return CollectLaunches{wide32, wide32 ? szg::kMatrixWideQueries : per_launch};
}

}  // namespace szgi
