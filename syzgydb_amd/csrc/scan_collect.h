// scan_collect.h -- the collect core: one batch of collect sweeps on the device and back (defined in scan_radius.cpp).
// Per shard a batch holds nq buffers of cap entries in d_collect (the sweeps append row and key), the same in d_out (the
// re-rank's float64 distances, sorted per query) and one counter per query in d_count.  The callers -- RadiusCall and
// SketchRadiusCall (scan_radius.cpp), SketchTopkCall (scan_sketch_topk.cpp) -- differ in which index is swept, how the
// counters start and which launches make the sweeps; everything else is here.  Internal to those two files.
#pragma once
#include "collect_plan.h"
#include "scan_internal.h"

namespace szgi {

constexpr uint32_t kNoKeyUkey = 0xFFFFFFFFu;  // "ordered key" of the entries staged ahead of the sweep: a sweep's keys
                                              // are clamped to 3e38, so none of them orders that high

struct CollectBatch : Batch {
    std::vector<float> thr;       // key threshold per query, of the sweep that runs
    std::vector<size_t> cap;      // per shard: entries per query of this batch's buffers
    std::vector<uint8_t> copied;  // per shard: the block of re-ranked hits was copied back at enqueue time
    std::vector<QMeta> meta;      // each query's constants with the flags of the sweep that runs (float32 path: traced calls only)
    void size() { thr.assign(nq, 0.0f), cap.assign(ctx.size(), 0), copied.assign(ctx.size(), 0); }  // (once planned)
};

// consider()'s radius branch over the hits cs (distance <= radius already applied; presorted: already ascending by
// distance -- the device's sort), then the pop loop: the hits ascending, ties in the order the reference's heap leaves
void radius_assemble(std::vector<HeapItem> &cs, bool presorted, std::vector<HeapItem> *out);

// the buffers of batch t on shard s: cap follows the largest hit count the context has seen (collect_cap has the rules)
// (floor: entries per query the caller's plan asks for from the first batch on -- the sample plan's; 0: none)
int collect_buffers(CollectBatch &t, size_t s, bool limited, size_t head_max, size_t floor = 0);

// collect launches of up to qpl sweeps for queries [q0, q1) of the batch, back to back on the shard's scan chain; `after`
// goes on once they are done.  wide: the call takes wide batches -- its launches take the matrix sweep whatever their
// count, as top-k's; norms: the shard's resident row norms for the launches that read them (null: none does)
int collect_sweeps(szg_index *ix, Shard *sh, Ctx *c, const CollectBatch &t, size_t cap, int q0, int q1, int qpl,
                   hipStream_t after, int part, bool wide = false, const float *norms = nullptr);

// the device tail of queries [q0, q1) on stream tl: the float64 distances of what was collected -- on the rows of shard
// `rows` of index `on`: the sweep's own, or the float32 shard a sketch shard stands for --, the counts staying on the
// device; each query's hits sorted by distance there too (lists of up to kSortHitsMax: the host only filters); the
// counters and, where the block is small, the hits on their way back
int collect_tail(const szg_index *on, const Shard *rows, Ctx *c, const CollectBatch &t, size_t s, int q0, int q1, hipStream_t tl);

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
                   const std::vector<uint64_t> *exc, Collected *out);

// the certificate record of query j of batch t: what was collected for it on every shard, under its sweep's threshold
void collect_record(szg_index *ix, const szg_index *swept, const CollectBatch &t, int j, int traced_as, int pass, int keys,
                    int sweep, double D, double slack, const std::vector<szg_cert_entry> &entries);

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

// float32 shard a's eligible rows without a usable sketch (sketchless_rows under mask words m), appended to *head as the
// entries a collect batch through the sketch stages ahead of the sweep: kNoKeyUkey << 32 | shard-local row
void sketchless_head(const szg_index *ix, const Shard *a, const uint64_t *m, std::vector<uint64_t> *head);

// One shard's part of a collect batch through the sketch, behind its uploads: head[j] -- the entries staged ahead of the
// sweep in query j's buffer -- and the counters that start at their counts, the collect sweeps over sketch shard s of sk
// under t.thr, and the tail on the rows of shard s of ix.  p: the call's plan; floor: collect_buffers'.
int sketch_collect_enqueue(szg_index *ix, szg_index *sk, const SketchPlan &p, CollectBatch &t, size_t s,
                           const std::vector<std::vector<uint64_t>> &head, size_t floor);

}  // namespace szgi
