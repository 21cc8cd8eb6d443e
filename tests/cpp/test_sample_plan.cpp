// Stand-alone check of the sample plan of a top-k search through the sketch (syzgydb_amd/csrc/sample_plan.h): the stride,
// the sample's tiles and rows, the key slots and the starting capacity.  Plain C++, no HIP, its own main;
// tests/test_sketch_topk_collect_cpu.py builds it with -fsanitize=address,undefined and runs it: the key buffer is a heap
// block of exactly key_bytes, every slot of every query is written the way the sample kernel writes it (sample tile j,
// row t -> slot 16 j + t) and every row read is checked against the shard's rows, so an index past either end aborts the
// run.  The expected numbers are written out by hand from the rules (the largest of 16, 8, 4, 2 that leaves 4 k sample
// rows; 8 k stride rounded up to a power of two; k <= 2048).
#include "../../syzgydb_amd/csrc/sample_plan.h"

#include <cstdio>
#include <memory>
#include <vector>

static int g_failures = 0;

#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_failures++;                                                       \
        }                                                                       \
    } while (0)

static szgi::SamplePlanIn shard(uint64_t rows, int k, int nq, uint32_t steps = 12)
{
    szgi::SamplePlanIn in;
    in.rows = rows, in.k = k, in.n_queries = nq;
    in.bits = 8, in.planes = 2, in.tiled = true, in.steps = steps, in.r16 = 4 * steps;
    return in;
}

// the sample pass as the kernel walks it: every slot of a buffer of exactly the planned size, once
static void walk(uint64_t rows, int k, int nq)
{
    const szgi::SamplePlan p = szgi::sample_plan(shard(rows, k, nq));
    if (!p.serves) return;
    EXPECT(p.key_bytes == (uint64_t)nq * p.slots * 4 && p.slots == 16 * p.tiles);
    std::unique_ptr<uint32_t[]> keys(new uint32_t[p.key_bytes / 4]);
    std::vector<uint8_t> seen(rows, 0);
    const uint64_t n_tiles = (rows + 15) / 16;
    uint64_t scored = 0;
    for (uint64_t j = 0; j < p.tiles; j++) {
        const uint64_t tile = szgi::sample_tile_of(j, p.stride);
        EXPECT(tile < n_tiles);
        for (uint32_t t = 0; t < 16; t++) {
            const uint64_t row = tile * 16 + t;
            const bool ok = row < rows;
            if (ok) {
                EXPECT(!seen[row]);
                seen[row] = 1;  // (past the rows: aborts under the sanitizer)
                scored++;
            }
            for (int q = 0; q < nq; q++)
                keys[szgi::sample_key_index(q, p.slots, szgi::sample_slot(j, t))] = ok ? (uint32_t)row : szgi::kSampleNoKey;
        }
    }
    EXPECT(scored == p.sample_rows);
    // every slot was written, with the row the slot stands for
    for (int q = 0; q < nq; q++)
        for (uint64_t s = 0; s < p.slots; s++) {
            const uint64_t row = (s / 16) * p.stride * 16 + s % 16;
            EXPECT(keys[(uint64_t)q * p.slots + s] == (row < rows ? (uint32_t)row : szgi::kSampleNoKey));
        }
    // the next tile of the walk is past the shard
    EXPECT(szgi::sample_tile_of(p.tiles, p.stride) >= n_tiles);
}

int main()
{
    using namespace szgi;
    // the stride steps at exactly 4 k sample rows: 6400 rows at stride 16 are 25 tiles = 400 rows
    SamplePlan p = sample_plan(shard(6400, 100, 1));
    EXPECT(p.serves && p.stride == 16 && p.tiles == 25 && p.sample_rows == 400 && p.slots == 400 && p.cap == 16384);
    p = sample_plan(shard(6400, 101, 1));
    EXPECT(p.serves && p.stride == 8 && p.tiles == 50 && p.sample_rows == 800 && p.cap == 8192);
    p = sample_plan(shard(6400, 201, 1));
    EXPECT(p.serves && p.stride == 4 && p.sample_rows == 1600 && p.cap == 8192);
    p = sample_plan(shard(6400, 401, 1));
    EXPECT(p.serves && p.stride == 2 && p.sample_rows == 3200 && p.cap == 8192);
    p = sample_plan(shard(6400, 800, 1));
    EXPECT(p.serves && p.stride == 2 && p.cap == 16384);
    EXPECT(!sample_plan(shard(6400, 801, 1)).serves);  // 3200 sample rows at stride 2 < 3204
    // a partial last tile outside the sample (6399: tile 399 of 400) and inside it (6401: tile 400, one row)
    p = sample_plan(shard(6399, 99, 1));
    EXPECT(p.serves && p.stride == 16 && p.tiles == 25 && p.sample_rows == 400 && p.slots == 400);
    p = sample_plan(shard(6401, 100, 1));
    EXPECT(p.serves && p.stride == 16 && p.tiles == 26 && p.sample_rows == 401 && p.slots == 416);
    p = sample_plan(shard(6385, 100, 1));  // 400 tiles, the last with one row, not in the sample: still 400 rows
    EXPECT(p.serves && p.stride == 16 && p.sample_rows == 400);
    // the cap on k, and the batch limit it keeps: 32 queries x 8 x 2048 x 16 entries
    p = sample_plan(shard(1u << 20, 2048, 32));
    EXPECT(p.serves && p.stride == 16 && p.cap == (1u << 18) && p.cap * 32 == (8u << 20));
    EXPECT(p.key_bytes == 32ull * 65536 * 4);
    EXPECT(!sample_plan(shard(1u << 20, 2049, 32)).serves);
    EXPECT(!sample_plan(shard(1u << 20, 0, 1)).serves && !sample_plan(shard(0, 35, 1)).serves);
    EXPECT(!sample_plan(shard(20000, 35, 33)).serves && !sample_plan(shard(20000, 35, 0)).serves);
    // what the matrix forms do not serve
    SamplePlanIn in = shard(20000, 35, 1);
    in.tiled = false;
    EXPECT(!sample_plan(in).serves);
    in = shard(20000, 35, 1);
    in.planes = 3;
    EXPECT(!sample_plan(in).serves);
    in = shard(20000, 35, 1);
    in.bits = 4;
    EXPECT(!sample_plan(in).serves);
    in = shard(20000, 35, 1);
    in.r16 = 4 * in.steps + 1;  // rows that are no whole 64-byte steps
    EXPECT(!sample_plan(in).serves);
    // buffers of exactly the planned sizes, every slot written
    for (uint64_t rows : {6399ull, 6400ull, 6401ull, 19967ull, 19968ull, 19969ull, 20000ull, 561ull, 17ull})
        for (int k : {1, 35, 100, 1000})
            for (int nq : {1, 3, 17, 32}) walk(rows, k, nq);
    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("sample plan ok\n");
    return 0;
}
