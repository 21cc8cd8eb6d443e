// row_offer.h -- one tile offered to a wave's row lists (RowList, device_lists.h): the selection step that the
// sketch-on-sketch join (kernels_join.hip) shares with the matrix sweep's row-list form, as a function.
// The matrix sweep (kernels_scan_mx.hip) still carries these steps inside its tile lambda.  Calling this function from
// there (rowlists_offer<NS, SZG_MX_ROUND_SKIP != 0>, the same statements in the same order) changes the bytes of 16 of
// its 20 gfx950 code objects -- every row-list form; the four collect objects stay (scripts/code_object_hashes.sh against
// the parent commit) -- so that switch wants the sweep's own measurements and suite behind it, and is left for a change
// of its own.  Until then a change to one copy is a change to the other.
#pragma once
#include "device_lists.h"

namespace szg {

// One tile offered to NS row lists at once: slot r of lane-row c is the list of one query,
// lane (c, j) offers row row0 + j to it with ordered key uk[r] where pass[r] is set (the pre-filter: the key is not above
// wk[r], the slot's worst key).  A crowded tile -- at least bulk_min passing pairs in the wave -- merges every slot with
// a passing lane whole (merge_tile); otherwise rounds retire one passing lane of every lane-row and slot at a time, 16
// at the most.  Both leave the same lists bit for bit.  wk[] is brought up to date.  Call with the whole wave.
// SKIP: a round leaves out the slots without a passing lane (wave-uniform: late tiles have a few passing lanes, in one or
// two of the slots); false runs all NS slots every round (the variant build -DSZG_MX_ROUND_SKIP=0).
template <int NS, bool SKIP = true>
__device__ __forceinline__ void rowlists_offer(RowList (&rls)[NS], const bool (&pass)[NS], const uint32_t (&uk)[NS], uint32_t row0,
                                               uint32_t row, int lane, int m, uint32_t bulk_min, float (&wk)[NS])
{
    uint64_t left[NS];
    uint32_t n_pass = 0;
#pragma unroll
    for (int r = 0; r < NS; r++) {
        left[r] = __ballot(pass[r]);
        n_pass += (uint32_t)__popcll(left[r]);
    }
    if (n_pass >= bulk_min) {
#pragma unroll
        for (int r = 0; r < NS; r++) {
            if (!left[r]) continue;  // (wave-uniform)
            rls[r].merge_tile(pass[r], uk[r], row0, lane, m);
            wk[r] = rls[r].worst_key();
        }
        return;
    }
    for (int round = 0; round < 16; round++) {
        uint64_t act[NS];
        uint64_t act_any = 0;
#pragma unroll
        for (int r = 0; r < NS; r++) {
            act[r] = left[r] & __ballot((((uint64_t)uk[r] << 32) | row) < rls[r].worst);
            act_any |= act[r];
        }
        if (!act_any) break;
#pragma unroll
        for (int r = 0; r < NS; r++) {
            if (SKIP && !act[r]) continue;
            rls[r].round(act[r], left[r], uk[r], row0, lane, m);
        }
    }
#pragma unroll
    for (int r = 0; r < NS; r++) wk[r] = rls[r].worst_key();
}

}  // namespace szg
