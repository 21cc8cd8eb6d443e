// Stand-alone dumper of the spanfile pager (include/syzgy_pager.h, syzgydb_amd/csrc/spanfile_pager.cpp): the one part
// of the library that reads bytes it did not write.  Plain C++, no HIP, its own main; tests/test_pager_malformed_cpu.py
// compiles it together with spanfile_pager.cpp under -fsanitize=address,undefined and runs it over malformed and mutated
// collection files.  For every file named on the command line it opens the file with 1, 2 and 3 threads, calls every
// accessor -- the ids and the vectors into heap blocks of exactly their size, so a write past either end aborts the run --
// reads every metadata byte through the returned pointer, and prints one line per open.  It judges nothing: the Python
// side compares each line with the model of the read rules (tests/spanfile_model.py).
#include "../../include/syzgy_pager.h"

#include <cstdio>
#include <cstdlib>
#include <string>

// the pager's one outside symbol (szg_pager_load pages into a scan handle): record the call, touch every byte
static uint64_t g_loaded_rows = 0, g_loaded_sum = 0;
static int64_t g_row_bytes = 0;
extern "C" int szg_index_load(szg_index *, const uint8_t *rows, uint64_t n_rows)
{
    g_loaded_rows = n_rows;
    g_loaded_sum = 0;
    for (uint64_t i = 0; i < n_rows * (uint64_t)g_row_bytes; i++) g_loaded_sum += rows[i];
    return SZG_OK;
}

static uint32_t crc32_of(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}

static int64_t row_bytes_of(int bits, int dim) { return bits == 4 ? ((int64_t)dim + 1) / 2 : (int64_t)dim * bits / 8; }

static std::string dump(const char *path, int threads)
{
    char buf[160];
    szg_pager *p = nullptr;
    const int rc = szg_pager_open(&p, path, threads);
    if (rc != SZG_OK) {
        std::snprintf(buf, sizeof buf, "rc=%d", rc);
        return buf + std::string(p ? " handle-left-behind" : "");
    }
    int dim = 0, bits = 0, metric = 0;
    szg_pager_options(p, &dim, &bits, &metric);
    const uint64_t count = szg_pager_count(p);
    const int64_t rb = row_bytes_of(bits, dim);
    const uint64_t need = count * (uint64_t)rb;
    std::snprintf(buf, sizeof buf, "rc=0 dim=%d bits=%d metric=%d count=%llu skipped=%llu", dim, bits, metric,
                  (unsigned long long)count, (unsigned long long)szg_pager_skipped(p));
    std::string line = buf;

    uint64_t *ids = static_cast<uint64_t *>(std::malloc(count ? count * sizeof(uint64_t) : 1));
    uint8_t *vec = static_cast<uint8_t *>(std::malloc(need ? need : 1));
    if (!ids || !vec) std::abort();
    int r = szg_pager_ids(p, ids);
    if (r) line += " ids-rc=" + std::to_string(r);
    if (need) {
        r = szg_pager_vectors(p, vec, need - 1);   // one byte short: refused, nothing written
        line += " short=" + std::to_string(r);
    } else {
        line += " short=na";
    }
    r = szg_pager_vectors(p, vec, need);
    if (r) line += " vectors-rc=" + std::to_string(r);
    const uint8_t *md = nullptr;
    uint64_t ml = 0;
    line += " range=" + std::to_string(szg_pager_metadata(p, count, &md, &ml));
    line += " ids=";
    for (uint64_t i = 0; i < count; i++) line += (i ? "," : "") + std::to_string((unsigned long long)ids[i]);
    std::snprintf(buf, sizeof buf, " vec=%08x meta=", crc32_of(vec, need));
    line += buf;
    for (uint64_t i = 0; i < count; i++) {
        r = szg_pager_metadata(p, i, &md, &ml);
        if (r) {
            line += " metadata-rc=" + std::to_string(r);
            break;
        }
        std::snprintf(buf, sizeof buf, "%s%llu:%08x", i ? "," : "", (unsigned long long)ml, crc32_of(md, ml));
        line += buf;
    }
    // the load path copies through a buffer of its own: the stub must see the same bytes
    g_row_bytes = rb;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < need; i++) sum += vec[i];
    r = szg_pager_load(p, reinterpret_cast<szg_index *>(&g_row_bytes));
    if (r || g_loaded_rows != count || g_loaded_sum != sum) line += " load-differs rc=" + std::to_string(r);
    std::free(ids);
    std::free(vec);
    szg_pager_close(p);
    return line;
}

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++)
        for (int threads = 1; threads <= 3; threads++)
            std::printf("%s t=%d %s\n", argv[a], threads, dump(argv[a], threads).c_str());
    return 0;
}
