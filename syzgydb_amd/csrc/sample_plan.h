// sample_plan.h -- the arithmetic of the sample pass of a top-k search of large k through the sketch (option
// sketch_topk_collect; scan_sketch_topk.cpp, kernels_sample_mx.hip): which tiles of a sketch shard are
// scored, where each (query, sampled row) pair's key goes, how large the key buffer is, and how many entries per query the
// collect buffers of the sweep that follows start with.  Plain C++, no HIP, like collect_plan.h:
// tests/cpp/test_sample_plan.cpp compiles it on its own under the address and undefined-behaviour sanitizers.
//
// The sample is every stride-th tile of 16 rows: tiles 0, stride, 2 stride, ... below ceil(rows / 16).  Sample tile j is
// tile j * stride of the shard; its row t has slot 16 j + t of its query's keys, whether or not the row exists (the
// shard's last tile may be partial and may be in the sample: the slots of its missing rows hold "no key").
#pragma once
#include <cstddef>
#include <cstdint>

namespace szgi {

constexpr int kSampleStrideMax = 16;       // the strides tried, largest first: 16, 8, 4, 2
constexpr int kSampleRowsPerK = 4;         // a shard is served where its sample holds at least this many rows per result
constexpr int kSampleCapFactor = 8;        // the collect buffers start at this many entries per k * stride, rounded up to
                                           // a power of two (DESIGN.md 4.5 item 16 has the simulation behind it)
// The largest k served: at the largest stride the starting buffers of a 32-query batch are 32 x 8 x 2048 x 16 = 8M
// entries, the limit every batch through the sketch keeps (collect_plan.h, kRadiusBatchEntries).
constexpr int kSampleTopkMax = 2048;
constexpr uint32_t kSampleNoKey = 0xFFFFFFFFu;  // the slot of a row that does not exist or is not eligible for the query

struct SamplePlanIn {
    uint64_t rows = 0;     // of the sketch shard
    int k = 0;
    int n_queries = 0;     // of the launch (1 .. 32)
    int bits = 0;          // of the swept index: the sketch is 8
    int planes = 0;        // digit planes of its queries: the matrix cores take 2
    bool tiled = false;    // its layout: 16-row tiles of whole 64-byte steps
    uint32_t steps = 0;    // 64-byte steps per row
    uint32_t r16 = 0;      // 16-byte pieces per row of the lane map (whole steps: 4 * steps)
};

struct SamplePlan {
    bool serves = false;
    uint32_t stride = 0;        // in tiles
    uint64_t tiles = 0;         // sample tiles
    uint64_t sample_rows = 0;   // rows of the shard in them
    uint64_t slots = 0;         // key slots per query: 16 * tiles
    uint64_t key_bytes = 0;     // of the launch's key buffer: n_queries * slots * 4
    size_t cap = 0;             // entries per query the collect buffers start with
};

// tiles and rows of the sample of a shard of `rows` rows at `stride`
inline uint64_t sample_tiles(uint64_t rows, uint32_t stride)
{
    const uint64_t n_tiles = (rows + 15) / 16;
    return (n_tiles + stride - 1) / stride;
}
inline uint64_t sample_row_count(uint64_t rows, uint32_t stride)
{
    const uint64_t t = sample_tiles(rows, stride);
    if (t == 0) return 0;
    const uint64_t last_first = (t - 1) * (uint64_t)stride * 16;  // first row of the last sample tile (< rows)
    const uint64_t in_last = rows - last_first < 16 ? rows - last_first : 16;
    return (t - 1) * 16 + in_last;
}
// the tile of sample tile j, the slot of row t of it in a query's keys, and where query q's keys start
inline uint64_t sample_tile_of(uint64_t j, uint32_t stride) { return j * (uint64_t)stride; }
inline uint64_t sample_slot(uint64_t j, uint32_t t) { return j * 16 + t; }
inline uint64_t sample_key_index(int q, uint64_t slots, uint64_t slot) { return (uint64_t)q * slots + slot; }

inline size_t sample_cap(int k, uint32_t stride)
{
    const uint64_t want = (uint64_t)kSampleCapFactor * (uint64_t)k * stride;
    size_t cap = 1;
    while (cap < want) cap <<= 1;
    return cap;
}

inline SamplePlan sample_plan(const SamplePlanIn &in)
{
    SamplePlan p;
    // what the matrix forms serve: tiled 8-bit rows in whole 64-byte steps, two-plane queries, a launch of up to 32
    if (in.bits != 8 || in.planes != 2 || !in.tiled || in.steps == 0 || in.steps * 4u != in.r16) return p;
    if (in.k < 1 || in.k > kSampleTopkMax || in.n_queries < 1 || in.n_queries > 32 || in.rows == 0 ||
        in.rows > 0xFFFFFFFFull)
        return p;
    for (uint32_t s = kSampleStrideMax; s >= 2; s >>= 1) {
        if (sample_row_count(in.rows, s) < (uint64_t)kSampleRowsPerK * (uint64_t)in.k) continue;
        p.serves = true;
        p.stride = s;
        p.tiles = sample_tiles(in.rows, s);
        p.sample_rows = sample_row_count(in.rows, s);
        p.slots = p.tiles * 16;
        p.key_bytes = (uint64_t)in.n_queries * p.slots * sizeof(uint32_t);
        p.cap = sample_cap(in.k, s);
        return p;
    }
    return p;
}

}  // namespace szgi
