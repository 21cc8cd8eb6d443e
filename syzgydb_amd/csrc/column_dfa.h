// column_dfa.h -- szg_mask_where_dfa (scan_column.cpp / kernels_column.hip): a deterministic byte automaton walked over
// each row of a text column.  Like column_str.h: the per-row predicate reads the heap through a functor `fetch(i)` = the
// aligned dword at byte 4 i and the tables through two more functors, so the same body serves the kernel (tables in LDS
// or in global memory) and a host program (tests/cpp/test_column_dfa.cpp runs it under the sanitizers).  The host-side
// helpers are here as well: the validation of a caller's tables, the absorbing states, the staged table.  No HIP
// runtime in here; plain C++ either way.
//
// The caller's automaton: class_of[256] maps a byte to its column, next[state * n_classes + class] is the transition,
// accept_bits the accepting states.  The STAGED table is `next` with bit 15 (kDfaStop) set in every entry whose target
// is absorbing -- a state whose every transition is to itself: "already matched" or "can no longer match" -- so a walk
// learns with the transition itself that nothing behind this byte can change its verdict, and stops reading the row.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define SZG_DFA_HD __host__ __device__ __forceinline__
#else
#define SZG_DFA_HD inline
#endif

namespace szgi {

constexpr uint32_t kDfaStatesMax = 32768;      // SZG_DFA_STATES_MAX: a state is 15 bits of a staged entry
constexpr uint32_t kDfaTableMax = 1u << 20;    // SZG_DFA_TABLE_MAX: n_states * n_classes
constexpr uint32_t kDfaStop = 0x8000;          // staged entries: the target is absorbing
constexpr uint32_t kDfaLdsEntries = 24576;     // the largest staged table the kernel copies into LDS (48 KiB)

// ---- the predicate --------------------------------------------------------------------------------------------------

// The state after feeding the bytes [start, start + len) of the heap from `state0`, or the absorbing state the walk met
// on its way.  state0 and every value of next(i) are staged entries: a state in bits 0..14, kDfaStop in bit 15.
// One dword is fetched, then up to four steps are taken: the four class lookups do not depend on the state, only the
// transitions form a chain.  The next dword is asked for before the chain starts.  Every dword it fetches holds a byte
// of the value; len == 0, or an absorbing state0, fetches nothing.
template <class Fetch, class ClassOf, class Next>
SZG_DFA_HD uint32_t dfa_walk(const Fetch &fetch, uint32_t start, uint32_t len, const ClassOf &class_of, const Next &next,
                             uint32_t n_classes, uint32_t state0)
{
    uint32_t s = state0;
    if (len == 0 || (s & kDfaStop)) return s & (kDfaStop - 1);
    uint32_t i = start >> 2, left = len;
    uint32_t nb = 4 - (start & 3);             // bytes of the value in the dword at hand
    if (nb > left) nb = left;
    uint32_t w = fetch(i) >> (8 * (start & 3));
    for (;;) {
        uint32_t ahead = 0;
        if (left > nb) ahead = fetch(i + 1);   // (holds byte start + (len - left) + nb of the value)
        const uint32_t c0 = class_of(w & 0xffu), c1 = class_of((w >> 8) & 0xffu), c2 = class_of((w >> 16) & 0xffu),
                       c3 = class_of(w >> 24);
        s = next(s * n_classes + c0);
        if (s & kDfaStop) break;
        if (nb > 1) {
            s = next(s * n_classes + c1);
            if (s & kDfaStop) break;
            if (nb > 2) {
                s = next(s * n_classes + c2);
                if (s & kDfaStop) break;
                if (nb > 3) {
                    s = next(s * n_classes + c3);
                    if (s & kDfaStop) break;
                }
            }
        }
        left -= nb;
        if (left == 0) break;
        i++, w = ahead;
        nb = left < 4 ? left : 4;
    }
    return s & (kDfaStop - 1);
}

SZG_DFA_HD bool dfa_accepts(const uint64_t *accept_bits, uint32_t state) { return (accept_bits[state >> 6] >> (state & 63)) & 1ull; }

// ---- the caller's tables (host) -------------------------------------------------------------------------------------

enum { kDfaOk = 0, kDfaNull, kDfaCounts, kDfaTooLarge, kDfaStart, kDfaClass, kDfaNext };

// The whole table against its own counts, before anything is staged: after kDfaOk no index the walk can form leaves the
// table.  kDfaTooLarge (beyond kDfaStatesMax / kDfaTableMax) is decided by the counts alone: such a table is not read.
inline int dfa_validate(uint32_t n_states, uint32_t n_classes, uint32_t start, const uint8_t *class_of, const uint16_t *next,
                        const uint64_t *accept_bits)
{
    if (!class_of || !next || !accept_bits) return kDfaNull;
    if (n_states == 0 || n_classes == 0 || n_classes > 256) return kDfaCounts;
    if (n_states > kDfaStatesMax || (uint64_t)n_states * n_classes > kDfaTableMax) return kDfaTooLarge;
    if (start >= n_states) return kDfaStart;
    for (uint32_t b = 0; b < 256; b++)
        if (class_of[b] >= n_classes) return kDfaClass;
    for (size_t i = 0, n = (size_t)n_states * n_classes; i < n; i++)
        if (next[i] >= n_states) return kDfaNext;
    return kDfaOk;
}

// absorbing[s] = every transition of state s is to s (a validated table)
inline std::vector<uint8_t> dfa_absorbing(uint32_t n_states, uint32_t n_classes, const uint16_t *next)
{
    std::vector<uint8_t> absorbing(n_states, 1);
    for (uint32_t s = 0; s < n_states; s++)
        for (uint32_t c = 0; c < n_classes && absorbing[s]; c++)
            if (next[(size_t)s * n_classes + c] != s) absorbing[s] = 0;
    return absorbing;
}

// dwords of the image the kernel reads: the class map (256 bytes), then the staged table, two entries a dword
inline size_t dfa_image_dwords(uint32_t n_states, uint32_t n_classes) { return 64 + ((size_t)n_states * n_classes + 1) / 2; }

// The image of a validated table (little-endian: class map bytes, staged entries as uint16, an odd count zero-padded)
// and the staged start state.
inline std::vector<uint32_t> dfa_stage(uint32_t n_states, uint32_t n_classes, uint32_t start, const uint8_t *class_of,
                                       const uint16_t *next, uint32_t *start_staged)
{
    const std::vector<uint8_t> absorbing = dfa_absorbing(n_states, n_classes, next);
    std::vector<uint32_t> image(dfa_image_dwords(n_states, n_classes), 0u);
    for (uint32_t b = 0; b < 256; b++) image[b / 4] |= (uint32_t)class_of[b] << (8 * (b % 4));
    for (size_t i = 0, n = (size_t)n_states * n_classes; i < n; i++) {
        const uint32_t e = next[i] | (absorbing[next[i]] ? kDfaStop : 0u);
        image[64 + i / 2] |= e << (16 * (i % 2));
    }
    *start_staged = start | (absorbing[start] ? kDfaStop : 0u);
    return image;
}

}  // namespace szgi
