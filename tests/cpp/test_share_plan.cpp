// Stand-alone check of the matrix sweep's shared form as scan_plan.h plans it (share_map, share_slices, share_grid,
// scan_variant's share answer).  Plain C++, no HIP, its own main; tests/test_share_plan_cpu.py builds it from scan_plan.h
// and scan_plan.cpp alone with -fsanitize=address,undefined and runs it.  The kernel's own index arithmetic is restated
// here from its contract: block b of a grid of G = 2 S blocks is (slice, group) = share_map(b, G); wave w of the block
// walks tiles slice * nwaves + w, + S * nwaves, ...; the list of query q goes to block_lists + (q * S + slice) * m.
#include "../../syzgydb_amd/csrc/scan_plan.h"

#include <cstdio>
#include <vector>

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

static ScanPlanIn sketch_launch(int n_queries, int kp, int share_opt)
{
    ScanPlanIn in{8, kSketch768, true, kp, false, false, 0, false};
    in.group = 0;
    in.n_queries = n_queries;
    in.block = 256;
    in.planes = 2;
    in.matrix_opt = 0;
    in.norms = true;
    in.wide_opt = 0;
    in.share_opt = share_opt;
    return in;
}

int main()
{
    // the map: a bijection onto [0, S) x {0, 1} for every even G; partners b, b + 8 where 16 divides G
    for (uint32_t G = 2; G <= 1024; G += 2) {
        const uint32_t S = (uint32_t)share_slices((int)G);
        EXPECT(S == G / 2);
        std::vector<int> seen(2 * S, 0);
        bool ok = true;
        for (uint32_t b = 0; b < G; b++) {
            const ShareSlot s = share_map(b, G);
            ok = ok && s.slices == S && s.slice < S && s.group < 2;
            if (!ok) break;
            seen[s.slice * 2 + s.group]++;
        }
        EXPECT(ok);
        for (uint32_t i = 0; ok && i < 2 * S; i++) ok = seen[i] == 1;
        EXPECT(ok);
        if (G % 16 == 0)
            for (uint32_t b = 0; b < G; b++) {
                const ShareSlot s = share_map(b, G);
                if (s.group != 0) continue;
                const ShareSlot t = share_map(b + 8, G);
                EXPECT(b + 8 < G && t.slice == s.slice && t.group == 1);
            }
    }
    // the launch's grid from the plain launch's: 2 max(1, grid / 2), always even
    EXPECT(share_grid(1) == 2 && share_grid(2) == 2 && share_grid(3) == 2 && share_grid(12) == 12 && share_grid(13) == 12 &&
           share_grid(512) == 512);
    for (int g = 1; g <= 1024; g++) EXPECT(share_grid(g) % 2 == 0 && share_grid(g) >= 2 && share_grid(g) <= (g < 2 ? 2 : g));

    // list offsets of 33 .. 64 queries stay inside a buffer of exactly nq * S * m entries, and no two lists overlap
    for (int G : {2, 6, 12, 16, 48, 512})
        for (int m : {1, 8, 15})
            for (int nq = 33; nq <= kMatrixShareQueries; nq++) {
                const size_t S = (size_t)share_slices(G), total = (size_t)nq * S * m;
                std::vector<uint8_t> buf(total, 0);  // (out-of-range offsets: the address sanitizer's to find)
                for (uint32_t b = 0; b < (uint32_t)G; b++) {
                    const ShareSlot s = share_map(b, (uint32_t)G);
                    for (int x = 0; x < kMatrixWideQueries; x++) {
                        const int q = (int)s.group * kMatrixWideQueries + x;
                        if (q >= nq) continue;  // (idle columns write no list)
                        const size_t off = ((size_t)q * s.slices + s.slice) * m;
                        EXPECT(off + m <= total);
                        if (off + m <= total)
                            for (int i = 0; i < m; i++) buf[off + i]++;
                    }
                }
                bool once = true;
                for (size_t i = 0; i < total; i++) once = once && buf[i] == 1;
                EXPECT(once);
            }

    // every tile is visited exactly once per group
    const int nwaves = 4;
    for (uint64_t n_rows : {1ull, 15ull, 16ull, 17ull, 1000ull, 65537ull})
        for (int G : {2, 6, 16, 48, 512}) {
            const uint64_t n_tiles = (n_rows + 15) / 16;
            std::vector<int> seen(2 * n_tiles, 0);
            for (uint32_t b = 0; b < (uint32_t)G; b++) {
                const ShareSlot s = share_map(b, (uint32_t)G);
                const uint64_t stride = (uint64_t)s.slices * nwaves;
                for (int w = 0; w < nwaves; w++)
                    for (uint64_t t = (uint64_t)s.slice * nwaves + w; t < n_tiles; t += stride) seen[t * 2 + s.group]++;
            }
            bool once = true;
            for (int v : seen) once = once && v == 1;
            EXPECT(once);
        }

    // scan_variant: 33 .. 64 queries under sketch_share 0 / 2 take the shared form with the two-block LDS; 1 and the
    // record's default do not; neither do 32 or 65 queries, lists of 16 at 768 dimensions (65 920 bytes) or of 17
    {
        const ScanPlanIn d{};
        EXPECT(d.share_opt == 1);
        const ScanVariant z{};
        EXPECT(z.share == 0);
    }
    for (int nq : {33, 48, 64})
        for (int opt : {0, 2}) {
            const ScanVariant v = scan_variant(sketch_launch(nq, 8, opt));
            EXPECT(v.matrix == 1 && v.share == 1 && v.wide == 0 && v.group == 32 && v.row_lists == 1 && v.matrix_blocks() == 2);
            EXPECT(scan_lds_bytes(8, kSketch768, 8, 256, v.group, 2, v.matrix_blocks()) == 57728);
        }
    EXPECT(scan_variant(sketch_launch(64, 8, 1)).share == 0);
    EXPECT(scan_variant(sketch_launch(32, 8, 2)).share == 0 && scan_variant(sketch_launch(32, 8, 2)).wide == 1);
    EXPECT(scan_variant(sketch_launch(65, 8, 2)).share == 0);
    EXPECT(scan_variant(sketch_launch(64, 15, 2)).share == 1);
    EXPECT(scan_variant(sketch_launch(64, 16, 2)).share == 0);
    EXPECT(scan_variant(sketch_launch(64, 17, 2)).share == 0);
    {
        ScanPlanIn in = sketch_launch(64, 8, 2);
        in.wide_opt = 1;
        EXPECT(scan_variant(in).share == 0);
        in = sketch_launch(64, 8, 2);
        in.masked = true;
        EXPECT(scan_variant(in).share == 0);
        in = sketch_launch(64, 0, 2);
        in.collect = true;
        EXPECT(scan_variant(in).share == 0);
    }

    if (g_failures) {
        std::fprintf(stderr, "%d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("share plan ok\n");
    return 0;
}
