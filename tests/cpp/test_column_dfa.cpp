// Stand-alone check of syzgydb_amd/csrc/column_dfa.h (no HIP, its own main): the walk of a byte automaton that the
// text-column kernel runs, against a byte-by-byte restatement, and the host-side helpers -- the validation of a caller's
// tables, the absorbing states, the staged image.
//
// The automata: "length = 0 mod 3" (no absorbing state: every byte is read), "odd number of 0xff bytes", "contains NUL"
// (an absorbing accept), "first byte is a" (an absorbing reject or accept from byte 1), one state that rejects or
// accepts everything, and random tables with and without absorbing states.  Every value is walked at each of the 16
// byte alignments of a heap that is allocated EXACTLY as the library sizes it (str_heap_capacity), through a fetch
// functor that refuses every dword holding no byte of the row, with the tables read from an image of exactly
// dfa_image_dwords() dwords as the kernel reads them -- a read past either is the address sanitizer's report.  Lengths
// 0 to 17 and a few long ones; a stop at an absorbing state in mid-row must leave the rest of the row unread.
// Build with -fsanitize=address,undefined (tests/test_regex_dfa_cpu.py does).
#include "../../syzgydb_amd/csrc/column_dfa.h"
#include "../../syzgydb_amd/csrc/column_str.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using bytes = std::basic_string<uint8_t>;

struct Automaton {
    const char *name;
    uint32_t n_states, n_classes, start;
    std::vector<uint8_t> class_of;    // 256
    std::vector<uint16_t> next;       // n_states * n_classes
    std::vector<uint64_t> accept;     // ceil(n_states / 64)
    void accepts(uint32_t s) { accept[s >> 6] |= 1ull << (s & 63); }
};

static Automaton make(const char *name, uint32_t n_states, uint32_t n_classes, uint32_t start)
{
    Automaton a{name, n_states, n_classes, start, std::vector<uint8_t>(256, 0), std::vector<uint16_t>((size_t)n_states * n_classes, 0),
                std::vector<uint64_t>((n_states + 63) / 64, 0)};
    return a;
}

// the fetch of a host heap: aligned dword i, only while it holds a byte of the row [lo, hi)
struct HostFetch {
    const uint8_t *heap;
    uint32_t lo, hi;
    mutable long fetched = 0;
    mutable uint32_t highest = 0;
    uint32_t operator()(uint32_t i) const
    {
        if (!(4ull * i < hi && 4ull * i + 4 > lo)) {
            printf("fetch of dword %u, which holds no byte of the row [%u, %u)\n", i, lo, hi);
            exit(1);
        }
        fetched++;
        if (i > highest) highest = i;
        uint32_t v;
        memcpy(&v, heap + 4ull * i, 4);   // (past the allocation: the sanitizer's report)
        return v;
    }
};

// the restatement: every byte, one transition each
static uint32_t naive(const Automaton &a, const bytes &v)
{
    uint32_t s = a.start;
    for (uint8_t b : v) s = a.next[(size_t)s * a.n_classes + a.class_of[b]];
    return s;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static long cases = 0, early = 0;

// `value` at byte `start` of a heap of its own, flanked by bytes that would change the verdict if they were fed
static int check(const Automaton &a, const bytes &value, uint32_t start, uint8_t flank)
{
    if (szgi::dfa_validate(a.n_states, a.n_classes, a.start, a.class_of.data(), a.next.data(), a.accept.data()) != szgi::kDfaOk) {
        printf("%s: the automaton does not validate\n", a.name);
        return 1;
    }
    uint32_t state0 = 0;
    // the image in an allocation of exactly its size, as the library uploads it
    const std::vector<uint32_t> staged = szgi::dfa_stage(a.n_states, a.n_classes, a.start, a.class_of.data(), a.next.data(), &state0);
    uint32_t *image = (uint32_t *)malloc(staged.size() * 4);
    memcpy(image, staged.data(), staged.size() * 4);
    const uint8_t *cls = (const uint8_t *)image;
    const uint16_t *tab = (const uint16_t *)(image + 64);

    const uint64_t used = (uint64_t)start + value.size() + 4;
    const uint64_t cap = szgi::str_heap_capacity(used);
    uint8_t *heap = (uint8_t *)calloc(cap, 1);
    memset(heap, flank, start);
    if (!value.empty()) memcpy(heap + start, value.data(), value.size());
    memset(heap + start + value.size(), flank, 4);

    HostFetch fetch{heap, start, start + (uint32_t)value.size()};
    const uint32_t got = szgi::dfa_walk(
        fetch, start, (uint32_t)value.size(), [cls](uint32_t b) -> uint32_t { return cls[b]; },
        [tab](uint32_t i) -> uint32_t { return tab[i]; }, a.n_classes, state0);
    const uint32_t want = naive(a, value);
    int bad = 0;
    if (got != want || szgi::dfa_accepts(a.accept.data(), got) != szgi::dfa_accepts(a.accept.data(), want)) {
        printf("%s: start %u len %zu: state %u, the bytewise walk says %u\n", a.name, start, value.size(), got, want);
        bad = 1;
    } else if ((value.empty() || (state0 & szgi::kDfaStop)) && fetch.fetched) {
        printf("%s: read the heap for an empty row or from an absorbing start\n", a.name);
        bad = 1;
    } else if (fetch.fetched > (long)((start + value.size() + 3) / 4 - start / 4)) {
        printf("%s: fetched a dword twice\n", a.name);
        bad = 1;
    } else if (!value.empty() && !(state0 & szgi::kDfaStop)) {
        // where the bytewise walk first stands in an absorbing state, the walk has stopped: it has asked for at most
        // the dword behind the one that holds that byte
        const std::vector<uint8_t> absorbing = szgi::dfa_absorbing(a.n_states, a.n_classes, a.next.data());
        uint32_t s = a.start;
        for (size_t i = 0; i < value.size(); i++) {
            s = a.next[(size_t)s * a.n_classes + a.class_of[value[i]]];
            if (absorbing[s]) {
                const uint32_t at = (uint32_t)((start + i) / 4);
                if (fetch.highest > at + 1) {
                    printf("%s: start %u len %zu: absorbing at byte %zu, but dword %u was read\n", a.name, start, value.size(), i,
                           fetch.highest);
                    bad = 1;
                }
                if ((start + value.size() - 1) / 4 > at + 1) early++;
                break;
            }
        }
    }
    cases++;
    free(heap);
    free(image);
    return bad;
}

static bytes random_bytes(size_t n, const uint8_t *alphabet, size_t n_alphabet)
{
    bytes b(n, 0);
    for (size_t i = 0; i < n; i++) b[i] = alphabet[next_random() % n_alphabet];
    return b;
}

#define EXPECT(cond)                                                \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                               \
        }                                                           \
    } while (0)

static std::vector<Automaton> automata()
{
    std::vector<Automaton> out;
    {   // length = 0 mod 3: one class, a cycle of three states
        Automaton a = make("length mod 3", 3, 1, 0);
        a.next = {1, 2, 0};
        a.accepts(0);
        out.push_back(a);
    }
    {   // an odd number of 0xff bytes
        Automaton a = make("odd 0xff", 2, 2, 0);
        a.class_of[0xff] = 1;
        a.next = {0, 1, 1, 0};
        a.accepts(1);
        out.push_back(a);
    }
    {   // contains NUL: state 1 is an absorbing accept
        Automaton a = make("contains NUL", 2, 2, 0);
        for (int b = 1; b < 256; b++) a.class_of[b] = 1;
        a.next = {1, 0, 1, 1};
        a.accepts(1);
        out.push_back(a);
    }
    {   // the first byte is 'a': absorbing from byte 1 either way
        Automaton a = make("first byte a", 3, 2, 0);
        a.class_of['a'] = 1;
        a.next = {2, 1, 1, 1, 2, 2};
        a.accepts(1);
        out.push_back(a);
    }
    {
        Automaton a = make("rejects all", 1, 1, 0);
        out.push_back(a);
        Automaton b = make("accepts all", 1, 1, 0);
        b.accepts(0);
        out.push_back(b);
    }
    // random tables: 70 states over 5 classes (two accept words), some states made absorbing; 256 classes, 3 states
    for (int round = 0; round < 6; round++) {
        Automaton a = make("random", round < 4 ? 70 : 3, round < 4 ? 5 : 256, 0);
        for (int b = 0; b < 256; b++) a.class_of[b] = (uint8_t)(a.n_classes == 256 ? b : next_random() % a.n_classes);
        for (uint16_t &e : a.next) e = (uint16_t)(next_random() % a.n_states);
        for (uint32_t s = 0; s < a.n_states; s++) {
            if (next_random() % 2) a.accepts(s);
            if (round % 2 && next_random() % 4 == 0)
                for (uint32_t c = 0; c < a.n_classes; c++) a.next[(size_t)s * a.n_classes + c] = (uint16_t)s;
        }
        a.start = (uint32_t)(next_random() % a.n_states);
        out.push_back(a);
    }
    return out;
}

static int check_helpers()
{
    using namespace szgi;
    Automaton a = make("helpers", 3, 2, 0);
    a.class_of['a'] = 1;
    a.next = {2, 1, 1, 1, 2, 2};
    const uint8_t *cls = a.class_of.data();
    const uint16_t *nxt = a.next.data();
    const uint64_t *acc = a.accept.data();
    EXPECT(dfa_validate(3, 2, 0, cls, nxt, acc) == kDfaOk && dfa_validate(3, 2, 2, cls, nxt, acc) == kDfaOk);
    EXPECT(dfa_validate(3, 2, 0, nullptr, nxt, acc) == kDfaNull && dfa_validate(3, 2, 0, cls, nullptr, acc) == kDfaNull);
    EXPECT(dfa_validate(3, 2, 0, cls, nxt, nullptr) == kDfaNull);
    EXPECT(dfa_validate(0, 2, 0, cls, nxt, acc) == kDfaCounts && dfa_validate(3, 0, 0, cls, nxt, acc) == kDfaCounts);
    EXPECT(dfa_validate(3, 257, 0, cls, nxt, acc) == kDfaCounts);
    // the limits are decided by the counts alone: these tables do not exist and are not read
    EXPECT(dfa_validate(kDfaStatesMax + 1, 1, 0, cls, nxt, acc) == kDfaTooLarge);
    EXPECT(dfa_validate(kDfaStatesMax, 33, 0, cls, nxt, acc) == kDfaTooLarge);
    EXPECT(dfa_validate(4097, 256, 0, cls, nxt, acc) == kDfaTooLarge);
    EXPECT(dfa_validate(0xFFFFFFFFu, 256, 0, cls, nxt, acc) == kDfaTooLarge);
    EXPECT(dfa_validate(3, 2, 3, cls, nxt, acc) == kDfaStart && dfa_validate(3, 2, 0xFFFFFFFFu, cls, nxt, acc) == kDfaStart);
    a.class_of[7] = 2;
    EXPECT(dfa_validate(3, 2, 0, cls, nxt, acc) == kDfaClass);
    a.class_of[7] = 0;
    a.next[5] = 3;
    EXPECT(dfa_validate(3, 2, 0, cls, nxt, acc) == kDfaNext);
    a.next[5] = 0xFFFF;
    EXPECT(dfa_validate(3, 2, 0, cls, nxt, acc) == kDfaNext);
    a.next[5] = 2;
    // the largest tables there can be validate: 32768 states of one class, 4096 states of 256 classes
    {
        std::vector<uint16_t> big(kDfaTableMax, 0);
        std::vector<uint64_t> bits(kDfaStatesMax / 64, 0);
        std::vector<uint8_t> zero(256, 0), identity(256);
        for (int b = 0; b < 256; b++) identity[b] = (uint8_t)b;
        big[kDfaStatesMax - 1] = kDfaStatesMax - 1;
        EXPECT(dfa_validate(kDfaStatesMax, 1, kDfaStatesMax - 1, zero.data(), big.data(), bits.data()) == kDfaOk);
        uint32_t st = 0;
        const std::vector<uint32_t> image = dfa_stage(kDfaStatesMax, 1, kDfaStatesMax - 1, zero.data(), big.data(), &st);
        EXPECT(image.size() == 64 + kDfaStatesMax / 2 && st == ((kDfaStatesMax - 1) | kDfaStop));   // (the last state loops)
        EXPECT((image[64] & 0xffffu) == kDfaStop && (image[64 + (kDfaStatesMax - 1) / 2] >> 16) == 0xffffu);
        big[kDfaStatesMax - 1] = 0;
        EXPECT(dfa_validate(4096, 256, 4095, identity.data(), big.data(), bits.data()) == kDfaOk);
        big[kDfaTableMax - 1] = 4096;
        EXPECT(dfa_validate(4096, 256, 4095, identity.data(), big.data(), bits.data()) == kDfaNext);
    }
    // absorbing states and the image
    const std::vector<uint8_t> absorbing = dfa_absorbing(3, 2, nxt);
    EXPECT(absorbing.size() == 3 && !absorbing[0] && absorbing[1] && absorbing[2]);
    uint32_t st = 99;
    const std::vector<uint32_t> image = dfa_stage(3, 2, 0, cls, nxt, &st);
    EXPECT(st == 0 && image.size() == dfa_image_dwords(3, 2) && image.size() == 64 + 3);
    EXPECT(((const uint8_t *)image.data())['a'] == 1 && ((const uint8_t *)image.data())['b'] == 0);
    const uint16_t *tab = (const uint16_t *)(image.data() + 64);
    for (int i = 0; i < 6; i++) EXPECT(tab[i] == (a.next[i] | kDfaStop));   // (every target is state 1 or 2)
    EXPECT(dfa_image_dwords(1, 1) == 65 && dfa_image_dwords(3, 1) == 66 && dfa_image_dwords(4096, 256) == 64 + (1u << 19));
    dfa_stage(3, 2, 2, cls, nxt, &st);
    EXPECT(st == (2 | kDfaStop));
    return 0;
}

int main()
{
    const uint8_t alphabet[] = {0x00, 'a', 'b', 0xff, 0xc3, 0xa9};
    const std::vector<Automaton> all = automata();
    for (const Automaton &a : all) {
        // which flank would change this automaton's verdict: NUL, 0xff or 'a' -- all three
        for (uint8_t flank : {(uint8_t)0x00, (uint8_t)0xff, (uint8_t)'a'})
            for (uint32_t start = 0; start < 16; start++) {
                for (size_t len = 0; len <= 17; len++)
                    for (int round = 0; round < 4; round++) {
                        bytes v = random_bytes(len, alphabet + (round & 1), sizeof(alphabet) - (round & 1));   // (odd rounds: no NUL)
                        if (check(a, v, start, flank)) return 1;
                    }
                for (size_t len : {255u, 256u, 257u, 5000u}) {
                    bytes v = random_bytes(len, alphabet + 1, sizeof(alphabet) - 1);
                    if (check(a, v, start, flank)) return 1;
                    for (size_t at : {(size_t)0, (size_t)1, (size_t)5, len / 2, len - 1}) {   // a NUL planted: the absorbing accept
                        bytes w = v;
                        w[at] = 0x00;
                        if (check(a, w, start, flank)) return 1;
                    }
                }
            }
    }
    if (early == 0) {
        printf("no walk stopped at an absorbing state in mid-row: the early exit is not tested\n");
        return 1;
    }
    if (check_helpers()) return 1;
    printf("column dfa ok: %ld cases, %ld of them stopped at an absorbing state with dwords of the row left unread\n", cases, early);
    return 0;
}
