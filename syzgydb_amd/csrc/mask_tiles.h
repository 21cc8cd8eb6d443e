// mask_tiles.h -- the tile walk of the matrix sweep's masked form (kernels_scan_mx.hip with -DSZG_MX_MASKED; DESIGN.md 4.5
// item 14).  Plain C++, no HIP runtime: the kernel and tests/cpp/test_mask_tiles.cpp read the same function.
//
// A tile is 16 rows: tile T's rows are one aligned 16-bit slice of a mask word -- word T >> 2, shift 16 (T & 3).  A wave
// walks the tiles first, first + stride, ... below n_tiles; a tile none of whose rows is eligible (its slice of
// live AND allow is zero) is skipped.  Bits of the last word at positions past the rows are NOT trusted to be zero: the
// caller masks rows past n_rows itself, so a stale tail bit costs at most one tile read, never a wrong row.
#pragma once
#include <cstdint>

#include "scan_plan.h"

namespace szg {

struct MaskTile {
    uint64_t tile;   // the tile, or n_tiles: no further tile
    uint32_t slice;  // its eligible rows, bit t = row 16 tile + t (0 with tile == n_tiles)
};

SZG_PLAN_HD uint32_t mask_tile_slice(const uint64_t *words, uint64_t tile)
{
    return (uint32_t)(words[tile >> 2] >> (16 * (tile & 3))) & 0xFFFFu;
}

// The first tile T >= from of the walk from, from + stride, ... with T < n_tiles whose slice of live AND allow is not
// zero (a null pointer: all ones).  Reads words [from >> 2, (n_tiles - 1) >> 2] at most: none past ceil(rows / 64) - 1
// for n_tiles = ceil(rows / 16).  stride >= 1.
SZG_PLAN_HD MaskTile mask_next_tile(const uint64_t *live, const uint64_t *allow, uint64_t from, uint64_t stride, uint64_t n_tiles)
{
    for (uint64_t t = from; t < n_tiles; t += stride) {
        uint32_t s = 0xFFFFu;
        if (live) s &= mask_tile_slice(live, t);
        if (allow) s &= mask_tile_slice(allow, t);
        if (s) return MaskTile{t, s};
    }
    return MaskTile{n_tiles, 0u};
}

}  // namespace szg
