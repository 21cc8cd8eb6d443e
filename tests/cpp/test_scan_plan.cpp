// Stand-alone check of the one-sweep scan's plan (syzgydb_amd/csrc/scan_plan.h + scan_plan.cpp): which kernel a launch
// takes, the LDS it needs and the shapes of the list merges.  Plain C++, no HIP, its own main;
// tests/test_scan_plan_standalone_cpu.py builds it from the two files alone with -fsanitize=address,undefined and runs
// it.  Every expected number below is written out by hand from the rules the project states: the sketch's rows are
// 8-bit, 768 dimensions, tiled -- 48 pieces of 16 bytes, 4 lanes per row, 12 pieces per lane, 16 rows per wave step, 12
// steps of 64 bytes; a block of 256 threads is 4 waves; a two-plane image is 32 bytes per piece and query, a candidate 8.
#include "../../syzgydb_amd/csrc/scan_plan.h"

#include <cstdio>

using namespace szg;

static int g_failures = 0;

#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_failures++;                                                       \
        }                                                                       \
    } while (0)

static const RowMap kSketch768{48, 4, 12, 16, 1, 1};

// a top-k launch of the sketch pre-pass: two digit planes, resident norms, every option automatic
static ScanPlanIn sketch_launch(int n_queries, int kp)
{
    ScanPlanIn in{8, kSketch768, true, kp, false, false, 0, false};
    in.group = 0;
    in.n_queries = n_queries;
    in.block = 256;
    in.planes = 2;
    in.matrix_opt = 0;
    in.norms = true;
    in.wide_opt = 0;
    return in;
}

int main()
{
    // the record's defaults are the defaults the positional parameters had
    {
        const ScanPlanIn d{};
        EXPECT(d.group == 1 && d.n_queries == 1 && d.block == 256 && d.planes == 3 && d.group_ring == 0 && d.matrix_opt == 1 &&
               !d.norms && d.select_opt == 0 && d.wide_opt == 1);
    }
    // 16 queries, lists of 8: the matrix sweep in its 12-step form at ring 6, 16 queries per row read, row lists;
    // 16 x (48 x 32 image + 12 constants + 4 waves x 8 x 8 lists) = 16 x 1804 bytes of LDS
    {
        const ScanVariant v = scan_variant(sketch_launch(16, 8));
        EXPECT(v.matrix == 1 && v.matrix_steps == 12 && v.ring_depth == 6 && v.group == 16 && v.row_lists == 1 && v.wide == 0);
        EXPECT(v.shaped == 0 && v.deep == 0 && v.nontemporal == 1 && v.matrix_blocks() == 1);
        EXPECT(scan_lds_bytes(8, kSketch768, 8, 256, v.group, 2, v.matrix_blocks()) == 28864);
    }
    // 32 queries: the wide form, two blocks of 1804 x 16 = 57 728 bytes
    {
        const ScanVariant v = scan_variant(sketch_launch(32, 8));
        EXPECT(v.matrix == 1 && v.wide == 1 && v.group == 32 && v.row_lists == 1 && v.matrix_blocks() == 2);
        EXPECT(scan_lds_bytes(8, kSketch768, 8, 256, v.group, 2, v.matrix_blocks()) == 57728);
        // 17 is wide already, 33 is more than a launch of the form holds
        EXPECT(scan_variant(sketch_launch(17, 8)).wide == 1);
        EXPECT(scan_variant(sketch_launch(33, 8)).wide == 0);
    }
    // ... with lists of 16: 32 x (1536 + 12 + 512) = 65 920, 384 bytes over 64 KiB -- one block
    {
        EXPECT(scan_lds_bytes(8, kSketch768, 16, 256, 32, 2, 2) == 64 * 1024 + 384);
        const ScanVariant v = scan_variant(sketch_launch(32, 16));
        EXPECT(v.matrix == 1 && v.wide == 0 && v.group == 16 && v.row_lists == 1 && v.matrix_blocks() == 1);
        EXPECT(scan_variant(sketch_launch(32, 15)).wide == 1);  // 32 x 2028 = 64 896
        // lists of 17: the serial inserts, which the wide form does not have
        const ScanVariant s = scan_variant(sketch_launch(32, 17));
        EXPECT(s.matrix == 1 && s.row_lists == 0 && s.wide == 0);
        ScanPlanIn serial = sketch_launch(32, 8);
        serial.select_opt = 1;
        EXPECT(scan_variant(serial).row_lists == 0 && scan_variant(serial).wide == 0 && scan_variant(serial).matrix == 1);
    }
    // 2 queries: below kMatrixMinQueries; G = 2 of the (4, 12) shape at the grouped ring
    {
        const ScanVariant v = scan_variant(sketch_launch(2, 8));
        EXPECT(v.matrix == 0 && v.group == 2 && v.shaped == 412 && v.matrix_blocks() == 0);
        EXPECT(v.ring_depth == scan_group_ring_of(12, 4, 0));
        EXPECT(scan_group_ring_of(12, 4, 0) == kGroupRingAuto && scan_group_ring_of(12, 4, kGroupRingBase) == 4);
        EXPECT(scan_group_ring_of(12, 4, kGroupRingAlt) == (12 % kGroupRingAlt == 0 ? kGroupRingAlt : 4));
        ScanPlanIn base = sketch_launch(2, 8);
        base.group_ring = kGroupRingBase;
        EXPECT(scan_variant(base).ring_depth == 4);
        // two two-plane images and two lists per wave, and the step lists: 2 x (1536 + 256) + 4 x 256 x 4
        EXPECT(scan_lds_bytes(8, kSketch768, 8, 256, 2, 2) == 7680);
        // sketch_matrix = 2: the matrix sweep from one query on
        ScanPlanIn always = sketch_launch(2, 8);
        always.matrix_opt = 2;
        EXPECT(scan_variant(always).matrix == 1 && scan_variant(always).group == 16);
        EXPECT(scan_variant(sketch_launch(3, 8)).matrix == 1);
    }
    // 1 query: G = 1, the shape's own ring; the whole three-plane image 48 x 48 + lists 256 + step lists 4096
    {
        const ScanVariant v = scan_variant(sketch_launch(1, 8));
        EXPECT(v.matrix == 0 && v.group == 1 && v.shaped == 412 && v.ring_depth == SZG_SHAPE_RING(4));
        EXPECT(query_lds_bytes(8, 48) == 2304);
        EXPECT(scan_lds_bytes(8, kSketch768, 8, 256, 1, 2) == 6656);
    }
    // masked: the any-shape kernel, one query per row read
    {
        ScanPlanIn in = sketch_launch(16, 8);
        in.masked = true;
        const ScanVariant v = scan_variant(in);
        EXPECT(v.shaped == 0 && v.group == 1 && v.matrix == 0 && v.deep == 0 && v.ring_depth == kRingShort);
    }
    // lists of 65 live in LDS: the deep ring, nothing else
    {
        const ScanVariant v = scan_variant(sketch_launch(16, 65));
        EXPECT(v.deep == 1 && v.ring_depth == kRingDeep && v.shaped == 0 && v.group == 1 && v.matrix == 0);
        EXPECT(scan_variant(sketch_launch(16, 64)).matrix == 1 && scan_variant(sketch_launch(16, 64)).row_lists == 0);
        // ... and the tuning hooks: ring = 8 forces it, no_shape_kernels keeps the short ring
        ScanPlanIn forced = sketch_launch(16, 8);
        forced.ring = 8;
        EXPECT(scan_variant(forced).deep == 1 && scan_variant(forced).matrix == 0 && scan_variant(forced).group == 1);
        ScanPlanIn plain = sketch_launch(1, 8);
        plain.no_shape_kernels = true;
        EXPECT(scan_variant(plain).shaped == 0 && scan_variant(plain).ring_depth == kRingShort);
    }
    // a collect launch of 32 keeps no lists: two blocks of 16 x (1536 + 16) = 49 664 bytes, whatever kp says
    {
        ScanPlanIn in = sketch_launch(32, 0);
        in.collect = true;
        const ScanVariant v = scan_variant(in);
        EXPECT(v.matrix == 1 && v.wide == 1 && v.group == 32 && v.row_lists == 0 && v.matrix_steps == 12 && v.ring_depth == 6);
        EXPECT(scan_lds_bytes(8, kSketch768, 0, 256, v.group, 2, v.matrix_blocks()) == 49664);
        in.kp = 100;
        EXPECT(scan_variant(in).wide == 1 && scan_variant(in).deep == 0);
        in.ring = 8;
        EXPECT(scan_variant(in).matrix == 0 && scan_variant(in).deep == 1);
        in.ring = 0;
        in.wide_opt = 1;
        EXPECT(scan_variant(in).matrix == 1 && scan_variant(in).wide == 0 && scan_variant(in).group == 16);
        // a query swept again on its own keeps the one-query collect kernel
        in.matrix_opt = 1;
        EXPECT(scan_variant(in).matrix == 0 && scan_variant(in).group == 1 && scan_variant(in).shaped == 412);
    }
    // sketch_matrix = 1: the G = 4 kernel; without norms, with three planes, over linear rows or under a named group: no matrix
    {
        ScanPlanIn in = sketch_launch(16, 8);
        in.matrix_opt = 1;
        const ScanVariant v = scan_variant(in);
        EXPECT(v.matrix == 0 && v.group == 4 && v.shaped == 412 && v.ring_depth == scan_group_ring_of(12, 4, 0));
        for (int what = 0; what < 4; what++) {
            ScanPlanIn no = sketch_launch(16, 8);
            if (what == 0) no.norms = false;
            if (what == 1) no.planes = 3;
            if (what == 2) no.tiled = false;
            if (what == 3) no.group = 4;
            EXPECT(scan_variant(no).matrix == 0 && scan_variant(no).group == 4);
        }
    }
    // the first eight fields alone (what szg_debug_scan_plan sets): the row-shape kernels of each width, group 1, no matrix
    {
        struct Case {
            int qbits;
            RowMap map;
            bool tiled;
            int shaped, ring;
        };
        const Case cases[] = {
            {4, {12, 4, 3, 16, 1, 1}, true, 403, 3},   // 4-bit 384 dimensions
            {4, {24, 4, 6, 16, 1, 1}, true, 406, 6},   // 4-bit 768
            {8, {24, 4, 6, 16, 1, 1}, true, 406, 6},   // 8-bit 384
            {8, {48, 4, 12, 16, 1, 1}, true, 412, 4},  // 8-bit 768
            {32, {96, 8, 12, 8, 1, 1}, false, 812, 4}, // float32 384, linear
            {16, {48, 4, 12, 16, 1, 1}, false, 0, 4},  // no shape kernels at 16 and 64 bits
            {64, {96, 8, 12, 8, 1, 1}, false, 0, 4},
            {8, {25, 4, 7, 16, 1, 0}, false, 0, 4},    // a ragged map
        };
        for (const Case &c : cases) {
            const ScanVariant v = scan_variant(ScanPlanIn{c.qbits, c.map, c.tiled, 10, false, false, 0, false});
            EXPECT(v.shaped == c.shaped && v.ring_depth == SZG_SHAPE_RING(c.ring) && v.group == 1 && v.matrix == 0 && v.deep == 0);
            EXPECT(v.nontemporal == (c.map.L >= 8 || c.tiled ? 1 : 0));
            const ScanVariant m = scan_variant(ScanPlanIn{c.qbits, c.map, c.tiled, 10, false, true, 0, false});
            EXPECT(m.shaped == 0 && m.ring_depth == kRingShort);
            const ScanVariant col = scan_variant(ScanPlanIn{c.qbits, c.map, c.tiled, 0, true, false, 0, false});
            EXPECT(col.shaped == c.shaped && col.group == 1 && col.matrix == 0);
        }
    }
    // the staged query per width: planes of 16 bytes per piece, or 4 / 8 bytes per element
    EXPECT(query_lds_bytes(4, 24) == 24u * 16 * kPlanes4 && query_lds_bytes(16, 3) == 96 && query_lds_bytes(32, 3) == 48 &&
           query_lds_bytes(64, 3) == 48);

    // the merges: a tournament of 64 lists up to lists of 128; the rank merge's fan fits 64 KiB: 8192 / kp, at most 32, at least 2
    EXPECT(merge_fan(1) == 64 && merge_fan(128) == 64 && merge_fan(129) == 32 && merge_fan(256) == 32 && merge_fan(512) == 16 &&
           merge_fan(4095) == 2 && merge_fan(4096) == 2 && merge_fan(100000) == 2);
    // the short merge: 1024 lists of 7 + 16 groups x (kp + 1) words: 8192 words = 64 KiB at kp = 63
    EXPECT(merge_short_lds(1024, 7, 63) == 64 * 1024);
    EXPECT(merge_short_fits(1024, 7, 63) && !merge_short_fits(1024, 7, 64) && !merge_short_fits(1024, 8, 63));
    EXPECT(!merge_short_fits(1025, 1, 2) && !merge_short_fits(0, 1, 2) && !merge_short_fits(64, 0, 8));
    EXPECT(merge_short_fits(64, 7, 8) && !merge_short_fits(64, 8, 8));
    EXPECT(merge_short_cap(1024, 63) == 1006 && merge_short_sorts(1024, 63) == 512);
    EXPECT(merge_short_cap(64, 8) == 6 && merge_short_sorts(64, 8) == 4 && merge_short_sorts(64, 2) == 0);
    EXPECT(merge_short_sorts(512, 24) == 128);  // 8 groups x 24 - 2 = 190

    if (g_failures) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("scan plan ok\n");
    return 0;
}
