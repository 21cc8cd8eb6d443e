// Stand-alone check of syzgydb_amd/csrc/column_bits.h (no HIP, its own main): copy_bits against a bit-by-bit
// restatement for every pair of offsets within a word and lengths across one, two and three words, with source and
// destination buffers sized EXACTLY for the bits they hold -- so a read or write one word too far is a heap overflow
// the address sanitizer reports.  Build with -fsanitize=address,undefined (tests/test_columns_cpu.py does).
#include "../../syzgydb_amd/csrc/column_bits.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bool get(const uint64_t *w, uint64_t i) { return (w[i >> 6] >> (i & 63)) & 1ull; }

int main()
{
    const uint64_t lengths[] = {0, 1, 2, 37, 63, 64, 65, 100, 127, 128, 129, 191, 200};
    long cases = 0;
    for (uint64_t dst_off = 0; dst_off < 130; dst_off += (dst_off < 66 ? 1 : 31))
        for (uint64_t src_off = 0; src_off < 70; src_off++)
            for (uint64_t n : lengths)
                for (int with_src = 0; with_src < 2; with_src++) {
                    // exactly the words that hold the bits (at least one, so data() is never null by accident)
                    uint64_t *src = nullptr;
                    const uint64_t src_words = (src_off + n + 63) / 64, dst_words = (dst_off + n + 63) / 64;
                    if (with_src) {
                        src = (uint64_t *)malloc((src_words ? src_words : 1) * sizeof(uint64_t));
                        for (uint64_t i = 0; i < src_words; i++) src[i] = next();
                    }
                    uint64_t *dst = (uint64_t *)malloc((dst_words ? dst_words : 1) * sizeof(uint64_t));
                    std::vector<uint64_t> before(dst_words);
                    for (uint64_t i = 0; i < dst_words; i++) before[i] = dst[i] = next();
                    szgi::copy_bits(dst, dst_off, src, src_off, n);
                    for (uint64_t i = 0; i < dst_words * 64; i++) {
                        bool want = get(before.data(), i);
                        if (i >= dst_off && i < dst_off + n) want = with_src ? get(src, src_off + (i - dst_off)) : true;
                        if (get(dst, i) != want) {
                            printf("copy_bits wrong: dst_off %llu src_off %llu n %llu src %d bit %llu\n",
                                   (unsigned long long)dst_off, (unsigned long long)src_off, (unsigned long long)n,
                                   with_src, (unsigned long long)i);
                            return 1;
                        }
                    }
                    free(src);
                    free(dst);
                    cases++;
                }
    printf("column bits ok: %ld cases\n", cases);
    return 0;
}
