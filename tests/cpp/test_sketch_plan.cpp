// Stand-alone check of the plan of a call through the sketch as sketch_plan.h states it: the batches of a call, the call
// rule's thresholds, the early tail of a short call, and the launches of every batch -- the functions the launch path and
// the plan hooks both compute from.  Plain C++, no HIP, its own main; tests/test_sketch_plan_cpu.py builds it from
// sketch_plan.h, scan_plan.h and scan_plan.cpp alone with -fsanitize=address,undefined and runs it.
#include "../../syzgydb_amd/csrc/sketch_plan.h"

#include <cstdio>
#include <vector>

using namespace szgi;

static int g_failures = 0;

#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_failures++;                                                       \
        }                                                                       \
    } while (0)

// the sketch of 768-dimensional rows, 4M of them on 256 CUs: a plain sweep takes 512 blocks of 256 threads; lists of 8
static const szg::RowMap kSketch768{48, 4, 12, 16, 1, 1};
static const int kGrid = 512, kBlock = 256, kKp = 8;

static SketchShape shape(int wide_opt = 0, int share_opt = 0, int masked_opt = 0)
{
    return SketchShape{8, kSketch768, true, 0, false, 0, 2, 0, 0, 0, wide_opt, share_opt, masked_opt, kKp, 16, 16, true};
}

static std::vector<int> chunks(int n, int size)
{
    std::vector<int> out;
    for (; n > 0; n -= size) out.push_back(n < size ? n : size);
    return out;
}
static std::vector<int> edged(int n, int size)  // 4, batches of `size`, a rest that leaves 4, 4
{
    std::vector<int> out{4};
    for (n -= 8; n > 0; n -= size) out.push_back(n < size ? n : size);
    out.push_back(4);
    return out;
}

int main()
{
    // the shape qualifies for both forms -- and not with lists of 16 entries, whose two blocks do not fit 64 KiB
    EXPECT(sketch_wide_serves(shape(), kGrid, kBlock, false, kKp) && sketch_share_serves(shape(), kGrid, kBlock, false, kKp));
    EXPECT(!sketch_wide_serves(shape(1), kGrid, kBlock, false, kKp) && !sketch_share_serves(shape(0, 1), kGrid, kBlock, false, kKp));
    EXPECT(!sketch_wide_serves(shape(), kGrid, kBlock, true, kKp) && sketch_wide_serves(shape(0, 0, 1), kGrid, kBlock, true, kKp));
    EXPECT(sketch_wide_serves(shape(), kGrid, kBlock, false, 0) && !sketch_wide_serves(shape(0, 0, 1), kGrid, kBlock, true, 0));
    {
        SketchShape s = shape();
        s.sketch_list = 16;
        EXPECT(!sketch_wide_serves(s, kGrid, kBlock, false, 16));
    }
    EXPECT(share_geometry(kGrid, kKp, kKp).grid == 512 && share_geometry(kGrid, kKp, kKp).slices == 256);
    EXPECT(share_geometry(1, kKp, kKp).grid == 2 && share_geometry(1, kKp, kKp).slices == 1);

    // the batches of the automatic rule and of the forced plans
    for (const int n : {71, 100, 135, 136, 200, 1024}) {
        const SketchCallWalk w = sketch_call_walk(shape(), kGrid, kBlock, kKp, n, false, true);
        EXPECT(w.wide == (n >= 72 ? 1 : 0) && w.share == (n >= 136 ? 1 : 0));
        EXPECT(w.batches == edged(n, n >= 136 ? 64 : (n >= 72 ? 32 : 16)));
        EXPECT(sketch_call_walk(shape(0, 1), kGrid, kBlock, kKp, n, false, true).batches == edged(n, n >= 72 ? 32 : 16));
        EXPECT(sketch_call_walk(shape(1, 0), kGrid, kBlock, kKp, n, false, true).batches == edged(n, 16));
        EXPECT(sketch_call_walk(shape(0, 2), kGrid, kBlock, kKp, n, false, true).batches == chunks(n, 64));
        EXPECT(sketch_call_walk(shape(2, 1), kGrid, kBlock, kKp, n, false, true).batches == chunks(n, 32));
        EXPECT(sketch_batch_sizes(n, 0, 2, 16) == chunks(n, 64) && sketch_batch_sizes(n, 2, 0, 16) == chunks(n, 32));
    }
    EXPECT((sketch_batch_sizes(71, 0, 0, 16) == std::vector<int>{4, 16, 16, 16, 15, 4}));
    EXPECT((sketch_batch_sizes(100, 1, 0, 16) == std::vector<int>{4, 32, 32, 28, 4}));
    EXPECT((sketch_batch_sizes(135, 1, 0, 16) == std::vector<int>{4, 32, 32, 32, 31, 4}));
    EXPECT((sketch_batch_sizes(136, 1, 1, 16) == std::vector<int>{4, 64, 64, 4}));
    EXPECT((sketch_batch_sizes(200, 1, 1, 16) == std::vector<int>{4, 64, 64, 64, 4}));
    EXPECT((sketch_batch_sizes(97, 0, 2, 16) == std::vector<int>{64, 33}) && (sketch_batch_sizes(136, 0, 2, 16) == std::vector<int>{64, 64, 8}));
    {
        const SketchCallWalk w = sketch_call_walk(shape(), kGrid, kBlock, kKp, 1024, false, true);
        EXPECT(w.batches.size() == 18 && w.batches[16] == 56 && w.launches == 18 && w.passes == 34);
    }

    // the call rule's thresholds: 2 x 32 + 2 x 4 and 2 x 64 + 2 x 4 queries, under the default batch and launch sizes only
    EXPECT(kWideCallMin == 72 && kShareCallMin == 136);
    EXPECT(sketch_call_wide(shape(), 71, true) == 0 && sketch_call_wide(shape(), 72, true) == 1);
    EXPECT(sketch_call_share(shape(), 135, kKp, 1, true) == 0 && sketch_call_share(shape(), 136, kKp, 1, true) == 1);
    EXPECT(sketch_call_wide(shape(), 1024, false) == 0 && sketch_call_share(shape(), 1024, kKp, 1, false) == 0);
    EXPECT(sketch_call_share(shape(), 1024, kKp, 0, true) == 0 && sketch_call_share(shape(), 1024, 0, 1, true) == 0);
    EXPECT(sketch_call_wide(shape(2), 16, true) == 0 && sketch_call_wide(shape(2), 17, true) == 2);
    EXPECT(sketch_call_share(shape(0, 2), 32, kKp, 0, true) == 0 && sketch_call_share(shape(0, 2), 33, kKp, 0, true) == 2);
    for (int which = 0; which < 2; which++) {
        SketchShape s = shape();
        (which ? s.query_batch : s.queries_per_launch) = 8;
        EXPECT(sketch_call_wide(s, 1024, true) == 0);
        const SketchCallWalk w = sketch_call_walk(s, kGrid, kBlock, kKp, 1024, false, true);
        EXPECT(w.wide == 0 && w.share == 0);
        s.sketch_wide = s.sketch_share = 2;  // (forced: whatever the sizes)
        EXPECT(sketch_call_wide(s, 1024, true) == 2 && sketch_call_share(s, 1024, kKp, 2, true) == 2);
    }

    // the early tail: none below 8 queries, all but the last min(4, n / 2) from 8 to 32, none above, none without
    // serialize_scans, none when forced
    for (int n = 1; n <= 100; n++) {
        const BatchRules r = sketch_batch_rules(n, 0, 0, 16);
        const int last = n / 2 < 4 ? n / 2 : 4;
        EXPECT(short_call_early(n, r, true) == (n >= 8 && n <= 32 ? n - last : 0));
        EXPECT(short_call_early(n, r, false) == 0);
        EXPECT(short_call_early(n, sketch_batch_rules(n, 2, 0, 16), true) == 0);
        EXPECT(short_call_early(n, sketch_batch_rules(n, 0, 2, 16), true) == 0);
        EXPECT(short_call_early(n, sketch_batch_rules(n, 1, 1, 16), true) == (n >= 8 && n <= 32 ? n - last : 0));
    }

    // every call of 1 .. 200 queries under every wide / share: its launches partition [0, nq) in order, none holds more
    // queries than its form allows, and the passes are one per group of 16 (32 in the wide and shared forms) per launch
    for (int masks = 0; masks < 3; masks++)  // no masks; masks under sketch_masked = 0; under sketch_masked = 1
        for (int wide = 0; wide <= 2; wide++)
            for (int share = 0; share <= 2; share++)
                for (int nq = 1; nq <= 200; nq++) {
                    const SketchShape s = shape(0, 0, masks == 2 ? 1 : 0);
                    const BatchRules r = sketch_batch_rules(nq, wide, share, s.query_batch);
                    int q0 = 0, next = 0, passes = 0, want = 0;
                    bool ok = true;
                    for (const int b : sketch_batch_sizes(nq, wide, share, s.query_batch)) {
                        const int early = q0 == 0 ? short_call_early(nq, r, true) : 0;
                        const SketchLaunches l = sketch_batch_launches(s, true, kGrid, kBlock, kKp, b, early, masks != 0, wide, share);
                        ok = ok && l.masked == (masks == 1) && !(l.masked && (l.wide || l.share)) && !(l.share && l.early);
                        ok = ok && l.m == kKp && l.lists0 == (l.share ? 256 : 512) && l.grid == 512;
                        int launches = 0;
                        l.each([&](int part, int start, int n) {
                            ok = ok && q0 + start == next && n >= 1 && (part == 0 || l.early);
                            ok = ok && n <= (l.share ? 64 : (l.wide ? 32 : 16)) && (!l.share || n > 32);
                            next += n;
                            launches++;
                            passes += sketch_launch_passes(s, l, n);
                            // (one pass per query: a masked launch that keeps the one-query kernel, and a masked launch
                            // of one or two queries of a call without wide batches -- the matrix sweep starts at three)
                            const bool single = l.masked || (masks && l.matrix == 0 && n < szg::kMatrixMinQueries);
                            const int group = single ? 1 : (l.share || l.wide ? 32 : 16);
                            want += (n + group - 1) / group;
                        });
                        ok = ok && launches == l.n_launches(0) + (l.early ? l.n_launches(1) : 0);
                        q0 += b;
                        ok = ok && next == q0;
                    }
                    ok = ok && next == nq && passes == want;
                    if (!ok) std::fprintf(stderr, "masks %d wide %d share %d nq %d: passes %d, want %d\n", masks, wide, share, nq, passes, want);
                    EXPECT(ok);
                }
    // the short calls the GPU tests pin (tests/test_gpu_sketch_matrix.py, launch_sizes)
    for (const int nq : {7, 8, 17, 32, 40}) {
        const SketchCallWalk w = sketch_call_walk(shape(), kGrid, kBlock, kKp, nq, false, true);
        EXPECT(w.launches == (nq == 7 ? 1 : (nq == 32 ? 3 : (nq == 40 ? 4 : 2))) && w.passes == w.launches);
    }
    // launches of collect batches: 32 where the call is wide, the batch may and the form serves
    EXPECT(sketch_collect_launches(shape(), kGrid, kBlock, false, 1, true, 17, 16).qpl == 32);
    EXPECT(sketch_collect_launches(shape(), kGrid, kBlock, false, 1, true, 16, 16).qpl == 16);
    EXPECT(sketch_collect_launches(shape(), kGrid, kBlock, false, 0, true, 32, 16).qpl == 16);
    EXPECT(sketch_collect_launches(shape(), kGrid, kBlock, false, 1, false, 32, 16).qpl == 16);
    EXPECT(!sketch_collect_launches(shape(), kGrid, kBlock, true, 2, true, 32, 7).wide32);

    if (g_failures) {
        std::fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    std::printf("sketch plan ok\n");
    return 0;
}
