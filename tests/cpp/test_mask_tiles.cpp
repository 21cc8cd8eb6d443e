// Stand-alone check of the tile walk of the matrix sweep's masked form (syzgydb_amd/csrc/mask_tiles.h: mask_next_tile).
// Plain C++, no HIP, its own main; tests/test_sketch_masked_cpu.py builds it with -fsanitize=address,undefined and runs it.
// The walk is compared with a brute-force loop over the rows' bits, for random and adversarial words, strides 1, 4 and
// 1024 and every first tile below the stride.  The words live in heap blocks of exactly ceil(rows / 64) words, so a read
// past them is an address-sanitizer error; bits of the last word past the rows are set at random (the walk may report a
// tile for them -- the kernel masks rows past n_rows itself -- but only a tile below n_tiles).
#include "../../syzgydb_amd/csrc/mask_tiles.h"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
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

// exactly n words on the heap (null for "no mask")
struct Words {
    std::unique_ptr<uint64_t[]> w;
    size_t n = 0;
    explicit Words(size_t n_) : w(new uint64_t[n_]()), n(n_) {}
    bool bit(uint64_t r) const { return (w[r >> 6] >> (r & 63)) & 1u; }
    void set(uint64_t r) { w[r >> 6] |= 1ull << (r & 63); }
};

// the slice of tile t by the rows' bits, one at a time; bits past `cover` (the words' last bit) read as 0
static uint32_t brute_slice(const Words *live, const Words *allow, uint64_t t)
{
    uint32_t s = 0;
    for (uint32_t i = 0; i < 16; i++) {
        const uint64_t r = t * 16 + i;
        bool ok = true;
        if (live) ok = ok && r < live->n * 64 && live->bit(r);
        if (allow) ok = ok && r < allow->n * 64 && allow->bit(r);
        if (ok) s |= 1u << i;
    }
    return s;
}

static void check_walk(const Words *live, const Words *allow, uint64_t rows, const char *what)
{
    const uint64_t n_tiles = (rows + 15) / 16;
    const uint64_t strides[] = {1, 4, 1024};
    for (uint64_t stride : strides) {
        for (uint64_t first = 0; first < stride; first++) {
            // the whole walk of a wave: every tile it reports against the brute-force list of its eligible tiles
            std::vector<uint64_t> want;
            for (uint64_t t = first; t < n_tiles; t += stride)
                if (brute_slice(live, allow, t)) want.push_back(t);
            size_t at = 0;
            uint64_t from = first;
            bool ok = true;
            for (;;) {
                const MaskTile m = mask_next_tile(live ? live->w.get() : nullptr, allow ? allow->w.get() : nullptr, from, stride, n_tiles);
                if (m.tile >= n_tiles) {
                    ok = ok && m.tile == n_tiles && m.slice == 0;
                    break;
                }
                ok = ok && at < want.size() && m.tile == want[at] && m.slice == brute_slice(live, allow, m.tile) && m.slice != 0 &&
                     m.tile % stride == first % stride;
                if (!ok) break;
                at++;
                from = m.tile + stride;
            }
            ok = ok && at == want.size();
            if (!ok) {
                std::fprintf(stderr, "%s: rows %llu stride %llu first %llu\n", what, (unsigned long long)rows,
                             (unsigned long long)stride, (unsigned long long)first);
                g_failures++;
                return;
            }
            // a walk that starts past the end finds nothing and reads nothing
            const MaskTile e = mask_next_tile(live ? live->w.get() : nullptr, allow ? allow->w.get() : nullptr, n_tiles + first, stride, n_tiles);
            EXPECT(e.tile == n_tiles && e.slice == 0);
        }
    }
}

int main()
{
    std::mt19937_64 rng(20261020);
    // rows: below one tile, one word, tile counts that are no multiple of 4 (a last word with 1 .. 3 tiles), partial last
    // tiles, and enough tiles for stride 1024 to come round
    const uint64_t row_counts[] = {1, 15, 16, 17, 63, 64, 65, 80, 81, 127, 129, 16 * 7, 16 * 7 + 3, 4096 + 37, 16 * 1024 * 3 + 16 * 5 + 1};
    for (uint64_t rows : row_counts) {
        const size_t words = (size_t)((rows + 63) / 64);
        const uint64_t n_tiles = (rows + 15) / 16;
        // adversarial words
        Words zero(words), one(words), last_tile(words), tile0(words), last_row(words);
        for (size_t i = 0; i < words; i++) one.w[i] = ~0ull;  // (the tail bits past the rows are set too)
        for (uint64_t r = (n_tiles - 1) * 16; r < rows; r++) last_tile.set(r);
        for (uint64_t r = 0; r < 16 && r < rows; r++) tile0.set(r);
        last_row.set(rows - 1);
        check_walk(&zero, nullptr, rows, "all zero (live)");
        check_walk(nullptr, &zero, rows, "all zero (allow)");
        check_walk(&one, &zero, rows, "all zero (allow) under all one");
        check_walk(&one, nullptr, rows, "all one");
        check_walk(&one, &one, rows, "all one, both");
        check_walk(nullptr, nullptr, rows, "no mask");
        check_walk(&last_tile, nullptr, rows, "only the last tile");
        check_walk(&one, &last_tile, rows, "only the last tile (allow)");
        check_walk(&tile0, nullptr, rows, "only tile 0");
        check_walk(nullptr, &tile0, rows, "only tile 0 (allow)");
        check_walk(&last_row, nullptr, rows, "one bit in the last row");
        check_walk(&tile0, &last_row, rows, "disjoint live and allow");
        // random words at several densities, tails included; live and allow that only overlap in places
        const double dens[] = {0.5, 0.05, 0.002};
        for (double d : dens) {
            Words a(words), b(words);
            std::bernoulli_distribution coin(d);
            for (uint64_t r = 0; r < words * 64; r++) {
                if (coin(rng)) a.set(r);
                if (coin(rng) || coin(rng)) b.set(r);
            }
            check_walk(&a, nullptr, rows, "random live");
            check_walk(nullptr, &b, rows, "random allow");
            check_walk(&a, &b, rows, "random live and allow");
            // whole runs of empty tiles: clear every tile of one residue of stride 4
            Words c(words);
            for (uint64_t r = 0; r < words * 64; r++)
                if ((r / 16) % 4 != 1) c.set(r);
            check_walk(&c, &b, rows, "one residue of stride 4 empty");
        }
    }
    if (g_failures) {
        std::fprintf(stderr, "%d failure(s)\n", g_failures);
        return 1;
    }
    std::puts("mask tiles ok");
    return 0;
}
