// device_lists.h -- per-wave candidate lists shared by the scan and select kernels.
//
// A candidate is (ordered key << 32) | row; unsigned order is (key, row) order.
// WaveList keeps the kp best candidates a wave has seen, sorted ascending:
//  * kp <= 64: in registers, entry i in lane i.  Insert = one ballot, a popcount
//    and a one-lane wave shift (DPP wave_shr:1), about a dozen VALU ops;
//  * kp  > 64: in LDS (64 entries per chunk), shifted chunk by chunk.
// Only the owning wave touches its list.  DS operations of one wave complete in
// issue order, so no s_barrier is needed; the wave barriers stop the compiler
// from moving one lane's store across another lane's load (it reasons per
// thread).  Plain shared pointers keep the accesses ds_* instructions -- a
// volatile generic pointer turns them into flat_* ops that drain the whole
// global-load queue.
#pragma once

#include "kernels.h"

namespace szg {

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src)
{
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl(lo, src);
    hi = __shfl(hi, src);
    return ((uint64_t)hi << 32) | lo;
}

// value of lane `src`, src wave-uniform: v_readlane_b32 through a scalar register -- a few cycles, where
// __shfl (ds_bpermute_b32 through the LDS crossbar) costs ~100.  The list code broadcasts once per candidate that
// passes the pre-filter and once per insert; while a list is still filling (every wave's first kp rows; a wave of
// a 125 K-row shard never sees more than that) these broadcasts were most of the selection's cost.
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// lane i receives lane i-1's value (lane 0 keeps its own)
__device__ __forceinline__ uint64_t wave_shr1_u64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, 0x138,
                                                              0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(v >> 32),
                                                              (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF,
                                                              false);
    return ((uint64_t)hi << 32) | lo;
}

struct WaveList {
    uint64_t *lds;    // this wave's kp entries in LDS (always allocated: the block merge reads it)
    uint64_t mine;    // register form: entry `lane` (kp <= 64)
    uint64_t worst;   // current kp-th best (wave-uniform)
    float worst_key;  // its key as a float (+inf while the list is not full): the scan's cheap pre-filter --
                      // a row whose key is above it cannot enter the list; anything else (NaN included)
                      // takes the exact 64-bit path
    int kp;
    bool in_regs;

    __device__ __forceinline__ void init(uint64_t *lds_, int kp_, int lane)
    {
        lds = lds_;
        kp = kp_;
        in_regs = kp_ <= 64;
        mine = kInvalidCand;
        worst = kInvalidCand;
        worst_key = __builtin_inff();
        if (!in_regs)
            for (int i = lane; i < kp; i += 64) lds[i] = kInvalidCand;
    }

    // c is wave-uniform and c < worst
    __device__ __forceinline__ void insert(uint64_t c, int lane)
    {
        if (in_regs) {
            const int pos = __popcll(__ballot(mine < c));  // entries are unique, sorted ascending
            const uint64_t up = wave_shr1_u64(mine);
            mine = lane < pos ? mine : (lane == pos ? c : up);
            worst = readlane_u64(mine, kp - 1);
            return;
        }
        int pos = 0;
        for (int base = 0; base < kp; base += 64) {
            const int e = base + lane;
            const bool lt = e < kp && lds[e] < c;
            pos += __popcll(__ballot(lt));
        }
        // shift [pos, kp-2] one slot up, highest chunk first
        for (int base = ((kp - 1) / 64) * 64; base >= 0; base -= 64) {
            if (base + 63 <= pos) break;
            const int e = base + lane;
            const bool mv = e > pos && e < kp;
            uint64_t v = 0;
            if (mv) v = lds[e - 1];
            __builtin_amdgcn_wave_barrier();
            if (mv) lds[e] = v;
            __builtin_amdgcn_wave_barrier();
        }
        if (lane == 0) lds[pos] = c;
        __builtin_amdgcn_wave_barrier();
        worst = lds[kp - 1];
    }

    // offer the candidates of the lanes with `have` set (at most one per lane)
    __device__ __forceinline__ void offer(bool have, uint64_t c, int lane)
    {
        uint64_t m = __ballot(have && c < worst);
        if (!m) return;
        while (m) {
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            const uint64_t cc = readlane_u64(c, src);
            if (cc < worst) insert(cc, lane);
        }
        worst_key = worst == kInvalidCand ? __builtin_inff() : key_from_ordered((uint32_t)(worst >> 32));
    }

    // make the LDS copy current (before the block-wide merge)
    __device__ __forceinline__ void flush(int lane)
    {
        if (in_regs && lane < kp) lds[lane] = mine;
    }
};

// within each row of 16 lanes, lane j receives lane j-1's value (a row's lane 0 keeps its own)
__device__ __forceinline__ uint64_t row_shr1_u64(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, 0x111,
                                                              0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(v >> 32),
                                                              (int)(uint32_t)(v >> 32), 0x111, 0xF, 0xF,
                                                              false);
    return ((uint64_t)hi << 32) | lo;
}

// both halves of a 64-bit value through one in-row DPP move (CTRL: quad_perm, row_ror, row_mirror, row_half_mirror)
template <int CTRL>
__device__ __forceinline__ uint64_t row_dpp_u64(uint64_t v)
{
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    return ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false) << 32) |
           (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false);
}
// the in-row partners of a sorting network over 16 lanes: lane j receives the value of lane ...
enum RowPartner {
    kRowXor1 = 0xB1,     // j ^ 1   (quad_perm [1, 0, 3, 2])
    kRowXor2 = 0x4E,     // j ^ 2   (quad_perm [2, 3, 0, 1])
    kRowXor3 = 0x1B,     // j ^ 3   (quad_perm [3, 2, 1, 0])
    kRowXor4 = -4,       // j ^ 4   (two moves: j ^ 7, then j ^ 3)
    kRowXor7 = 0x141,    // j ^ 7   (row_half_mirror)
    kRowXor8 = 0x128,    // j ^ 8   (row_ror:8)
    kRowXor15 = 0x140,   // j ^ 15  (row_mirror)
};
template <int P>
__device__ __forceinline__ uint64_t row_partner_u64(uint64_t v)
{
    if constexpr (P == kRowXor4) {
        return row_dpp_u64<kRowXor3>(row_dpp_u64<kRowXor7>(v));
    } else {
        return row_dpp_u64<P>(v);
    }
}
// one compare-exchange step: a lane with `low` keeps the smaller of its value and its partner's, the others the larger
template <int P>
__device__ __forceinline__ uint64_t row_cex_u64(uint64_t v, bool low)
{
    const uint64_t p = row_partner_u64<P>(v);
    return ((p < v) == low) ? p : v;
}

// RowList: FOUR lists of m <= 16 candidates in one register pair, one per lane-row (lanes 16 c .. 16 c + 15): lane
// (c, j) holds entry j of lane-row c's list, sorted ascending, entries j >= m stay kInvalidCand.  Where every
// lane-row has candidates of its own to offer (the matrix sweep: lane-row c scores queries 4 c .. 4 c + 3), one round
// inserts one candidate into each of the four lists at once, with per-lane VALU work, row-wise DPP and the LDS
// crossbar only -- no value travels through a scalar register, where WaveList::insert is a chain through three.
struct RowList {
    uint64_t mine;   // entry `lane & 15` of this lane-row's list
    uint64_t worst;  // its entry m - 1 (uniform within the lane-row; kInvalidCand while the list fills)

    __device__ __forceinline__ void init()
    {
        mine = kInvalidCand;
        worst = kInvalidCand;
    }

    // One round.  act: the ballot of the lanes that still have a candidate (their bit of `left`) below their lane-row's
    // `worst`; a lane's candidate is (ukey << 32) | (row0 + (lane & 15)).  In every lane-row with such a lane the first of
    // them is retired: its candidate goes into the lane-row's list and its bit of `left` is cleared.  Lane-rows without
    // one change nothing.  (`left` is a wave-wide mask and not a flag per lane: it stays in a scalar register pair
    // whatever else the tile's code does, and the test of a round is one scalar AND.)
    __device__ __forceinline__ void round(uint64_t act, uint64_t &left, uint32_t ukey, uint32_t row0, int lane, int m)
    {
        const int j = lane & 15, base = lane & 48;
        const uint32_t slice = (uint32_t)(act >> base) & 0xFFFFu;  // this lane-row's lanes
        const bool on = slice != 0;
        const int first = (__ffs((int)slice) - 1) & 15;            // (slice == 0: lane 0, unused)
        const uint32_t ck = (uint32_t)__builtin_amdgcn_ds_bpermute((base + first) << 2, (int)ukey);
        const uint64_t cand = ((uint64_t)ck << 32) | (row0 + (uint32_t)first);
        // entries are unique and sorted ascending: the entries below the candidate are a prefix of the lane-row
        const int pos = __popc((uint32_t)(__ballot(mine < cand) >> base) & 0xFFFFu);
        const uint64_t up = row_shr1_u64(mine);
        if (on && j >= pos && j < m) mine = j == pos ? cand : up;
        left &= ~__ballot(on && j == first);
        worst = shfl_u64(mine, base + m - 1);
    }

    // A whole tile at once (crowded tiles, option sketch_bulk): every lane-row's list becomes the m smallest of its
    // entries and the candidates of its lanes with `pass` set -- what the rounds leave, bit for bit, since an insert is a
    // set operation on unique entries.  A fixed network of 15 compare-exchange steps over the lane-row: the 16 candidates
    // (kInvalidCand where `pass` is false: it sorts last and never enters) are sorted ascending by a bitonic sort in its
    // mirror form (blocks of 2, 4, 8, 16: partner j ^ (block - 1), then j ^ block/4 .. j ^ 1), laid reversed against the
    // sorted list -- the smaller of each pair are the 16 smallest of the 32, a bitonic sequence -- and that is merged
    // (j ^ 8, 4, 2, 1).  Per-lane VALU work and in-row DPP only; no loop, no scalar round trip, one broadcast at the end.
    __device__ __forceinline__ void merge_tile(bool pass, uint32_t ukey, uint32_t row0, int lane, int m)
    {
        const int j = lane & 15, base = lane & 48;
        const bool l1 = !(j & 1), l2 = !(j & 2), l4 = !(j & 4), l8 = !(j & 8);
        uint64_t v = pass ? (((uint64_t)ukey << 32) | (row0 + (uint32_t)j)) : kInvalidCand;
        v = row_cex_u64<kRowXor1>(v, l1);
        v = row_cex_u64<kRowXor3>(v, l2);
        v = row_cex_u64<kRowXor1>(v, l1);
        v = row_cex_u64<kRowXor7>(v, l4);
        v = row_cex_u64<kRowXor2>(v, l2);
        v = row_cex_u64<kRowXor1>(v, l1);
        v = row_cex_u64<kRowXor15>(v, l8);
        v = row_cex_u64<kRowXor4>(v, l4);
        v = row_cex_u64<kRowXor2>(v, l2);
        v = row_cex_u64<kRowXor1>(v, l1);
        const uint64_t rev = row_partner_u64<kRowXor15>(v);
        v = rev < mine ? rev : mine;
        v = row_cex_u64<kRowXor8>(v, l8);
        v = row_cex_u64<kRowXor4>(v, l4);
        v = row_cex_u64<kRowXor2>(v, l2);
        v = row_cex_u64<kRowXor1>(v, l1);
        mine = j < m ? v : kInvalidCand;
        worst = shfl_u64(mine, base + m - 1);
    }

    __device__ __forceinline__ float worst_key() const
    {
        return worst == kInvalidCand ? __builtin_inff() : key_from_ordered((uint32_t)(worst >> 32));
    }
};

// number of entries of sorted list[0..n) that are < c
__device__ __forceinline__ int lower_count(const uint64_t *list, int n, uint64_t c)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < c) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// block-wide k-select: rank-merge the waves' sorted lists (entries are unique)
// into one sorted list of kp entries at `out`.  Call with all threads of the block.
__device__ __forceinline__ void block_merge_lists(const uint64_t *lists, int nwaves, int kp,
                                                  uint64_t *out, int tid, int nthreads)
{
    for (int i = tid; i < kp; i += nthreads) out[i] = kInvalidCand;
    __syncthreads();
    const int total = nwaves * kp;
    for (int it = tid; it < total; it += nthreads) {
        const int w = it / kp;
        const int i = it - w * kp;
        const uint64_t c = lists[it];
        if (c == kInvalidCand) continue;
        int rank = i;
        for (int w2 = 0; w2 < nwaves; w2++) {
            if (w2 == w) continue;
            rank += lower_count(lists + (size_t)w2 * kp, kp, c);
            if (rank >= kp) break;
        }
        if (rank < kp) out[rank] = c;
    }
}

}  // namespace szg
