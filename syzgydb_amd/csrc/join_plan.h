// join_plan.h -- the plan of the sketch-on-sketch join (szg_index_neighbors; kernels_join.hip, scan_join.cpp; DESIGN.md
// 4.5 item 20): does the kernel serve a call, and with which query block, slices, lists and LDS.  The launcher, the
// kernel's last check (launch_join) and the hook szg_debug_join_plan all compute from here.  Plain C++, header only; the
// launch-side declarations at the end need the HIP runtime.
#pragma once
#include <cstddef>
#include <cstdint>

#include "scan_plan.h"

namespace szg {

constexpr int kJoinMaxDim = 4096;     // tiled sketch rows of up to 64 whole 64-byte steps
constexpr int kJoinStageSteps = 16;   // 1 KiB step lines of one row tile per stage of the double buffer
constexpr int kJoinMaxKp = 96;        // the pre-pass's list rule (sketch_applies)
constexpr int kJoinMaxSlices = 256;   // lists per query that launch_merge_short merges in one launch
constexpr int kJoinBatch = 1024;      // queries of one launch: 16 query blocks of 64
// Calls of fewer queries take the parent's route (decode on the card, the masked search).  Measured at 1M x 768 cosine,
// k = 10 ("neighbours of stored rows"): the join is SLOWER than that route at every count -- 64: 1.26 against
// 0.94 ms, 1 024: 9.8 against 6.7 ms, 16 384: 150 against 102 ms -- so by default no call takes it: the threshold is where
// those numbers put it.  The kernel stays reachable through the hook szg_debug_join_min_queries (tests, measurements), whose
// least value is one launch's worth of a single query.
constexpr int kJoinMinQueries = 0x7FFFFFFF;

// per sketch row: S1 = sum v', S2 = sum v'^2 over its bytes v' = v - 128, and 1 / |n| of n = 2 v' + 1 in float32
struct JoinRowStat {
    int32_t s1, s2;
    float rinv;
    int32_t pad;
};

// LDS of a block of qb query rows over rows of `dim` bytes: two stages, and -- where the A operand does not stay in
// registers (more than 16 steps, or a query block below 64) -- the block's query rows
constexpr bool join_areg(int dim, int qb) { return qb == 64 && dim <= 64 * kJoinStageSteps; }
constexpr size_t join_lds_bytes(int dim, int qb)
{
    const int steps = dim / 64, sc = steps < kJoinStageSteps ? steps : kJoinStageSteps;
    return (size_t)2 * sc * 1024 + (join_areg(dim, qb) ? 0 : (size_t)qb * dim);
}

struct JoinPlan {
    int served;        // the kernel serves the launch
    int qb;            // query rows per block: 64, 32 or 16 (one wave per 16)
    int areg;          // the A operand stays in registers
    int masked;        // the masked form
    int query_blocks, slices, tiles_per_slice;
    int m;             // entries per (query, slice) list
    size_t lds_bytes;
};
// dim: the rows' bytes; n_queries: of the launch (<= kJoinBatch); kp: candidates merged per query; shard_rows: the rows
// swept.  QB is the largest of 64, 32, 16 whose LDS stays below a CU's 160 KiB (a block never takes all of it).  Slices:
// enough blocks for four per CU, at least kp / 4 where the shard has the tiles (lists of 16 then hold twice a slice's
// share of the kp best and 8 more, the pre-pass's rule), at most kJoinMaxSlices and never an empty one.
inline JoinPlan join_plan(int dim, int n_queries, int kp, int masked, int cu_count, uint64_t shard_rows)
{
    JoinPlan p{};
    if (dim < 64 || dim % 64 != 0 || dim > kJoinMaxDim || n_queries < 1 || n_queries > kJoinBatch || kp < 2 || kp > kJoinMaxKp ||
        shard_rows < 1 || shard_rows > 0xFFFFFFF0ull || cu_count < 1)
        return p;
    p.qb = 64;
    while (p.qb > 16 && join_lds_bytes(dim, p.qb) >= kLongLdsCu) p.qb /= 2;
    if (join_lds_bytes(dim, p.qb) >= kLongLdsCu) return p;
    p.areg = join_areg(dim, p.qb) ? 1 : 0;
    p.masked = masked ? 1 : 0;
    p.lds_bytes = join_lds_bytes(dim, p.qb);
    p.query_blocks = (n_queries + p.qb - 1) / p.qb;
    const uint64_t tiles = (shard_rows + 15) / 16;
    uint64_t s = ((uint64_t)4 * cu_count + p.query_blocks - 1) / p.query_blocks;
    const uint64_t least = (uint64_t)(kp + 3) / 4;
    if (s < least) s = least;
    if (s > (uint64_t)kJoinMaxSlices) s = kJoinMaxSlices;
    if (s > tiles) s = tiles;
    p.tiles_per_slice = (int)((tiles + s - 1) / s);
    p.slices = (int)((tiles + p.tiles_per_slice - 1) / p.tiles_per_slice);
    int m = 2 * kp / p.slices + 8;
    if (m > kRowListMax) m = kRowListMax;
    if (m > kp - 1) m = kp - 1;
    p.m = m;
    p.served = merge_short_fits(p.slices, p.m, kp) ? 1 : 0;
    return p;
}

struct JoinArgs {
    const uint8_t *rows;     // the shard's sketch rows, tiled
    uint32_t n_rows, steps;
    int dim;
    const uint8_t *qtiles;   // the launch's query sketch rows, packed dense in the same tiled layout
    uint32_t n_queries;
    const JoinRowStat *row_stat, *q_stat;
    const uint64_t *live, *allow;  // the masked form: null = all ones
    uint32_t query_blocks, slices, tiles_per_slice;
    int m;
    uint64_t *lists;         // [n_queries][slices][m]
};

}  // namespace szg

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace szg {
hipError_t launch_join_row_stats(const uint8_t *rows, uint32_t n_rows, uint32_t steps, int dim, JoinRowStat *out, hipStream_t stream);
// metric: kCosine / kEuclidean.  A launch that is not exactly one join_plan made for (a, p) is hipErrorInvalidValue.
hipError_t launch_join(int metric, const JoinArgs &a, const JoinPlan &p, hipStream_t stream);
}  // namespace szg
#endif
