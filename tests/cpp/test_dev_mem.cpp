// test_dev_mem.cpp -- syzgydb_amd/csrc/dev_mem.h in a stand-alone program over a malloc backend, under the address /
// undefined-behaviour sanitizers (tests/test_dev_mem_cpu.py builds and runs it; LeakSanitizer makes a block that is
// never given back a non-zero exit).  The backend records the device that is current and aborts when a block is freed
// while another device is; it logs every allocation and free, so the order of the two is checked as well.
#include "../../syzgydb_amd/csrc/dev_mem.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::abort();                                                    \
        }                                                                    \
    } while (0)

namespace {

struct Event {
    char what;   // 'a' allocation, 'f' free
    void *p;
    size_t bytes;
    int device;
};
int g_current = -1;
std::map<void *, int> g_home;   // device of every live block
std::vector<Event> g_log;
int g_pinned_live = 0;
std::string g_text;

struct MallocBackend {
    static int set_device(int d)
    {
        g_current = d;
        return 0;
    }
    static int dev_alloc(void **p, size_t bytes)
    {
        *p = std::malloc(bytes);   // (exactly `bytes`: the sanitizer sees a write one element too far)
        g_home[*p] = g_current;
        g_log.push_back({'a', *p, bytes, g_current});
        return 0;
    }
    static int dev_free(void *p)
    {
        CHECK(g_home.count(p) == 1);
        CHECK(g_home[p] == g_current);   // a block goes with its own device current
        g_home.erase(p);
        g_log.push_back({'f', p, 0, g_current});
        std::free(p);
        return 0;
    }
    static int pinned_alloc(void **p, size_t bytes)
    {
        *p = std::malloc(bytes);
        g_pinned_live++;
        return 0;
    }
    static int pinned_free(void *p)
    {
        g_pinned_live--;
        std::free(p);
        return 0;
    }
    static int error(szgi::DevErr kind, const char *what, int)
    {
        g_text = what;
        return kind == szgi::kDevRefused ? -2 : -1;
    }
};
template <typename T> using Buf = szgi::BasicBuf<T, false, MallocBackend>;
template <typename T> using Pinned = szgi::BasicBuf<T, true, MallocBackend>;
template <typename T> using Mem = szgi::BasicDevMem<T, MallocBackend>;

uint64_t blocks() { return szgi::dev_alloc_state().blocks.load(); }
uint64_t bytes() { return szgi::dev_alloc_state().bytes.load(); }
void refuse(int64_t nth) { szgi::dev_alloc_state().refuse_in.store(nth); }

void test_ensure()
{
    MallocBackend::set_device(0);
    Buf<uint32_t> b;
    CHECK(b.data() == nullptr && b.capacity() == 0);
    CHECK(b.ensure(3) == 0 && b.capacity() == 64 && blocks() == 1 && bytes() == 64 * 4);   // at least 64 elements
    b[63] = 7;
    uint32_t *p = b.data();
    CHECK(b.ensure(64) == 0 && b.data() == p && g_log.size() == 1);   // fits: nothing happens
    CHECK(b.ensure(65) == 0 && b.capacity() == 65 && bytes() == 65 * 4);
    b[64] = 9;
    // free FIRST: the old block is gone before the new one comes
    CHECK(g_log.size() == 3 && g_log[1].what == 'f' && g_log[1].p == p && g_log[2].what == 'a');
    CHECK(b.reset() == 0 && b.data() == nullptr && b.capacity() == 0 && blocks() == 0 && bytes() == 0);
    Pinned<double> h;   // pinned memory is neither counted nor refused
    refuse(1);
    CHECK(h.ensure(10) == 0 && h.capacity() == 64 && blocks() == 0 && g_pinned_live == 1);
    h[63] = 1.0;
    CHECK(b.ensure(1) == -2 && g_text == "scratch allocation");   // (the countdown was still armed)
    CHECK(h.reset() == 0 && g_pinned_live == 0);
}

void test_alloc_exact()
{
    Mem<uint8_t> m(3);
    CHECK(m.alloc_exact(1, "one") == 0 && m.capacity() == 1 && bytes() == 1 && g_log.back().device == 3);
    m[0] = 1;
    CHECK(m.alloc_exact(4097, "odd") == 0 && m.capacity() == 4097 && bytes() == 4097 && blocks() == 1);
    m[4096] = 1;
    Mem<uint64_t> w(1);
    CHECK(w.alloc_exact(5, "words") == 0 && w.capacity() == 5 && bytes() == 4097 + 40 && blocks() == 2);
    w[4] = ~0ull;
    CHECK(w.alloc_exact(0, "nothing") == 0 && w.data() == nullptr && w.capacity() == 0 && blocks() == 1);
    MallocBackend::set_device(0);   // (m goes on device 3 whatever is current here)
}

void test_moves()
{
    Mem<uint32_t> a(1), b(2);
    CHECK(a.alloc_exact(10, "a") == 0 && b.alloc_exact(20, "b") == 0);
    uint32_t *pa = a.data(), *pb = b.data();
    Mem<uint32_t> c(std::move(a));   // move construction: the source is empty, nothing is freed
    CHECK(c.data() == pa && c.device() == 1 && c.capacity() == 10 && a.data() == nullptr && a.capacity() == 0);
    CHECK(blocks() == 2);
    MallocBackend::set_device(0);
    const size_t n = g_log.size();
    b = std::move(c);   // move assignment between devices: b's block goes on device 2, b is then c's on device 1
    CHECK(g_log.size() == n + 1 && g_log.back().what == 'f' && g_log.back().p == pb && g_log.back().device == 2);
    CHECK(b.data() == pa && b.device() == 1 && b.capacity() == 10 && c.data() == nullptr && blocks() == 1);
    b = std::move(b);   // (self-assignment keeps the block)
    CHECK(b.data() == pa && blocks() == 1);
    MallocBackend::set_device(0);   // b goes on device 1 at the end of the scope
}

// the one growth shape: build the new block, copy, move-assign
int grow(Mem<uint32_t> *holder, size_t have, size_t want)
{
    Mem<uint32_t> bigger(holder->device());
    if (int rc = bigger.alloc_exact(want, "growth")) return rc;
    if (have) std::memcpy(bigger.data(), holder->data(), have * sizeof(uint32_t));
    *holder = std::move(bigger);
    return 0;
}

void test_growth()
{
    Mem<uint32_t> h(4);
    CHECK(grow(&h, 0, 100) == 0);
    for (uint32_t i = 0; i < 100; i++) h[i] = i * i;
    uint32_t *old = h.data();
    const size_t n = g_log.size();
    MallocBackend::set_device(0);
    CHECK(grow(&h, 100, 150) == 0 && h.capacity() == 150 && h.data() != old);
    for (uint32_t i = 0; i < 100; i++) CHECK(h[i] == i * i);   // (read after the old block is gone: copied before)
    // allocation, then -- after the copy -- exactly one free, of the old block, on its device
    CHECK(g_log.size() == n + 2 && g_log[n].what == 'a' && g_log[n + 1].what == 'f' && g_log[n + 1].p == old);
    CHECK(g_log[n + 1].device == 4 && blocks() == 1 && bytes() == 600);
    // a refusal: the holder is what it was
    refuse(1);
    old = h.data();
    CHECK(grow(&h, 150, 300) == -2 && g_text == "growth");
    CHECK(h.data() == old && h.capacity() == 150 && h[99] == 99 * 99 && blocks() == 1 && bytes() == 600);
    CHECK(szgi::dev_alloc_state().refuse_in.load() == 0);   // disarmed itself
    CHECK(grow(&h, 150, 300) == 0 && h.capacity() == 300 && h[99] == 99 * 99);
}

struct Part {   // as a column's: its device and owning members
    explicit Part(int device_ = 0) : device(device_), values(device_), present(device_) {}
    int device;
    Mem<uint8_t> values;
    Mem<uint64_t> present;
};

void test_vector_of_parts()
{
    std::vector<Part> parts;
    std::vector<uint8_t *> where;
    for (int d = 0; d < 9; d++) {   // (reallocates several times: the parts move, no block is freed or copied)
        parts.emplace_back(d % 3);
        CHECK(parts.back().values.alloc_exact(16 + d, "values") == 0 && parts.back().present.alloc_exact(2, "present") == 0);
        parts.back().values[15 + d] = (uint8_t)d;
        where.push_back(parts.back().values.data());
    }
    CHECK(blocks() == 18);
    for (int d = 0; d < 9; d++) CHECK(parts[d].values.data() == where[d] && parts[d].values[15 + d] == d && parts[d].device == d % 3);
    for (const Event &e : g_log) CHECK(e.what == 'a');   // (nothing was freed while the vector grew)
    std::vector<Part> fresh;   // the switch of a carry: a move-assignment of the parts
    for (int d = 0; d < 2; d++) {
        fresh.emplace_back(5);
        CHECK(fresh.back().values.alloc_exact(8, "values") == 0);
    }
    MallocBackend::set_device(7);
    parts = std::move(fresh);   // the nine old parts go, each on its own device (the backend aborts otherwise)
    CHECK(parts.size() == 2 && blocks() == 2 && parts[1].values.device() == 5);
}

void test_countdown()
{
    std::vector<Mem<uint32_t>> v;
    for (int i = 0; i < 6; i++) v.emplace_back(i);
    refuse(3);   // the third allocation from now on
    int rc[6];
    for (int i = 0; i < 6; i++) rc[i] = v[i].alloc_exact(10 + i, "counted");
    CHECK(rc[0] == 0 && rc[1] == 0 && rc[2] == -2 && rc[3] == 0 && rc[4] == 0 && rc[5] == 0);
    CHECK(v[2].data() == nullptr && v[2].capacity() == 0 && blocks() == 5);
    CHECK(g_home.size() == 5);   // the backend was not asked for the refused one
    refuse(2);
    refuse(0);   // disarmed by hand: nothing is refused
    CHECK(v[2].alloc_exact(12, "counted") == 0 && blocks() == 6);
    // a refused ensure() has freed first, as a failed one has
    refuse(1);
    CHECK(v[0].ensure(1000) == -2 && v[0].data() == nullptr && blocks() == 5);
    MallocBackend::set_device(0);
}

}  // namespace

int main()
{
    void (*tests[])() = {test_ensure, test_alloc_exact, test_moves, test_growth, test_vector_of_parts, test_countdown};
    for (auto t : tests) {
        g_log.clear();
        t();
        CHECK(blocks() == 0 && bytes() == 0 && g_home.empty() && g_pinned_live == 0);   // everything is given back
        CHECK(szgi::dev_alloc_state().refuse_in.load() == 0);
    }
    std::printf("dev mem ok\n");
    return 0;
}
