// scan_plan.h -- the plan of the one-sweep scan: which kernel a launch takes (scan_variant), its LDS (scan_lds_bytes),
// the merges' shapes, and the types, constants and row-shape table they are decided from.  Plain C++, no HIP runtime
// (tests/cpp/test_scan_plan.cpp); the definitions are scan_plan.cpp's, out of line: SZG_RING and SZG_GROUP_RING_ALT
// change the answers, and a variant build rebuilds only the objects it names.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SZG_PLAN_HD __host__ __device__ inline
#else
#define SZG_PLAN_HD inline
#endif

namespace szg {

// How the 64 lanes of a wave are laid over rows of r16 16-byte pieces:
// groups of L lanes take one row each, every lane P pieces of it.
struct RowMap {
    int r16;  // 16-byte pieces per (pitched) row
    int L;    // lanes per row
    int P;    // pieces per lane per row (L*P >= r16)
    int gpw;  // rows (lane groups) per wave iteration
    int pow2; // L is a power of two (groups are aligned: DPP reductions apply)
    int dense; // L*P == r16 and gpw*L == 64: every lane always has a piece of a row
};

// 4-bit rows, single-query scan: the query is quantized to balanced int4 digit planes of radix
// 16.  kPlanes4 digits carry |Q| < 16^kPlanes4 / 2; every plane costs one v_dot8_i32_i4 per
// dword of the row and one 16-byte LDS read per piece.  The quantization step enters the
// certification bound (key_eps) -- 4 planes (15 bits) still certify: the bound grows to
// ~4e-5 in cosine units against gaps of ~1e-2 between the k-th and the kp-th best key.
#ifndef SZG_PLANES4
#define SZG_PLANES4 4
#endif
constexpr int kPlanes4 = SZG_PLANES4;
constexpr double kQmax4 = kPlanes4 == 5 ? 480000.0 : 30000.0;

// Bytes of one prepared query as the scan stages it in LDS: float32 (float64 for
// 64-bit rows) per element, or integer digit planes of 16 bytes per piece for the
// exact-integer paths (3 int8 planes for 8-bit rows, 5 int4 planes for 4-bit rows).
SZG_PLAN_HD size_t query_lds_bytes(int qbits, int r16)
{
    switch (qbits) {
    case 4: return (size_t)r16 * 16 * kPlanes4;
    case 8: return (size_t)r16 * 16 * 3;
    case 16: return (size_t)r16 * 8 * 4;
    case 32: return (size_t)r16 * 4 * 4;
    default: return (size_t)r16 * 2 * 8;
    }
}

constexpr int kMaxSweepsPerLaunch = 16;
// ... but for the matrix sweep's wide form (two column blocks of 16 queries per row read, kernels_scan_mx.hip): the
// sketch pre-pass puts up to this many queries of a long call into one launch (option sketch_wide)
constexpr int kMatrixWideQueries = 32;
// ... and for its shared form (option sketch_share): one launch takes up to this many queries as two column groups of
// kMatrixWideQueries; paired blocks walk the same rows, one group each (share_map)
constexpr int kMatrixShareQueries = 64;
constexpr int kStepList = 256;  // row steps a wave compacts at a time (selective masks)

// The shared form's map from a block of a grid of G = 2 S blocks to its row slice and column group: the only place where
// the map and the slice count S are computed -- the kernel, its launcher and the host's list buffers all read it.
// A bijection onto [0, S) x {0, 1} for every even G.  G % 16 == 0: the two blocks of a slice are b and b + 8, which the
// round-robin dispatch over 8 XCDs places on one XCD (for speed only: nothing waits, nothing depends on placement);
// other even G: neighbours b, b + 1.
struct ShareSlot {
    uint32_t slice, group, slices;
};
constexpr int share_slices(int G) { return G / 2; }
// the grid of a shared launch over rows whose plain launch takes `grid` blocks: 2 S, S = max(1, grid / 2)
constexpr int share_grid(int grid) { return 2 * (grid / 2 > 1 ? grid / 2 : 1); }
SZG_PLAN_HD ShareSlot share_map(uint32_t b, uint32_t G)
{
    const uint32_t S = G / 2;
    if (G % 16 == 0) return ShareSlot{(b >> 4) * 8 + (b & 7), (b >> 3) & 1, S};
    return ShareSlot{b >> 1, b & 1, S};
}

// Which scan_kernel instantiation a launch takes: decided on the host by scan_variant -- the launcher dispatches on
// its answer, szg_debug_scan_plan reports it.
struct ScanVariant {
    int shaped;       // 0: the any-shape kernel; L * 100 + P: the kernel specialised for that row shape
    int deep;         // the any-shape kernel with the deep piece ring
    int ring_depth;   // 16-byte loads each lane keeps in flight
    int nontemporal;  // rows are loaded past the caches
    int group;        // queries of the launch scored per row read (1, 2 or 4; kMatrixQueries: the matrix sweep)
    int matrix;       // the matrix sweep (kernels_scan_mx.hip) serves the launch: one pass per kMatrixQueries queries
    int matrix_steps; // its form: 12 or 6 (64-byte steps per row fixed at compile time), 0 = the any-steps kernel
    int row_lists;    // the matrix sweep keeps its 16 lists as row lists (RowList, device_lists.h): kp <= kRowListMax
                      // under sketch_select = 0; else one WaveList per query and the serial inserts
    int wide;         // the matrix sweep's two-block form: one pass per kMatrixWideQueries queries (row lists only)
    // the matrix sweep's column blocks (what scan_lds_bytes takes as `matrix`): 2 = the wide form, 1, 0 = another kernel
    int matrix_blocks() const { return matrix ? (wide || share ? 2 : 1) : 0; }
    int share = 0;    // the two-block form shared between paired blocks (share_map): a launch of kMatrixWideQueries + 1 ..
                      // kMatrixShareQueries queries, one pass per column group of kMatrixWideQueries, both over one row read
                      // from HBM where the partner's lines are still on the die (its own launcher: launch_scan_share)
    int masked = 0;   // the matrix sweep's masked form (option sketch_masked; objects of their own, launch_scan_masked): the
                      // launch has tombstones or filter masks and takes the matrix sweep all the same
};
// What "automatic" (scan_group = 0) asks for, where a launch qualifies.
constexpr int kScanGroupAuto = 4;
// The matrix sweep: queries per pass, and the fewest queries of a launch that take it under sketch_matrix = 0 -- a pass
// costs about what a pass of the G = 1 kernel costs, and less than the G = 4 kernel's from 3 queries on (DESIGN.md 6,
// round 11).  A lone query keeps the G = 1 kernel.
constexpr int kMatrixQueries = 16;
constexpr int kMatrixMinQueries = 3;
constexpr int matrix_steps_form(int steps) { return steps == 12 || steps == 6 ? steps : 0; }
constexpr bool sketch_matrix_known(int64_t v) { return v == 0 || v == 1 || v == 2; }
// The matrix sweep's selection (option sketch_select): lists of up to kRowListMax entries live in the 16 lanes of a
// lane-row, four queries to a register pair, and take one candidate each per round (0 = automatic); 1 = the serial
// inserts into one WaveList per query, which longer lists always take.
constexpr int kRowListMax = 16;
constexpr bool sketch_select_known(int64_t v) { return v == 0 || v == 1; }
constexpr bool matrix_row_lists(int kp, int select_opt) { return select_opt == 0 && kp >= 1 && kp <= kRowListMax; }
// Crowded tiles of the row lists (option sketch_bulk): a tile whose pre-filter lets at least
// kBulkMin (query, row) pairs of the wave through merges every slot whole (RowList::merge_tile: a fixed sorting network
// in the lane-row) instead of retiring one lane per lane-row, slot and round.  0 = automatic (kBulkMin), 1 = never (rounds
// only), n >= 2 = tiles with at least n passing pairs (a tile of two blocks has at most 512: larger values are "never").
// Both routes leave the same lists bit for bit; routing and scan_variant do not depend on it.
constexpr uint32_t kBulkMin = 48;
constexpr uint32_t kBulkNever = 0xFFFFFFFFu;
constexpr bool sketch_bulk_known(int64_t v) { return v >= 0 && v <= 1024; }
constexpr uint32_t sketch_bulk_min(int bulk_opt) { return bulk_opt == 0 ? kBulkMin : (bulk_opt == 1 ? kBulkNever : (uint32_t)bulk_opt); }
// The wide form (option sketch_wide): a launch of more than kMatrixQueries and up to kMatrixWideQueries queries that the
// matrix sweep serves with row lists scores two column blocks of 16 queries per row read, where the two-block image,
// constants and lists fit 64 KiB of LDS (768 dimensions: lists of up to 15 entries; longer ones keep one block).
// 0 = automatic and 2 = wherever the shape allows differ on the host only (which calls form launches of 32); 1 = never.
constexpr bool sketch_wide_known(int64_t v) { return v == 0 || v == 1 || v == 2; }
// The shared form (option sketch_share): a launch of kMatrixWideQueries + 1 .. kMatrixShareQueries queries that the wide
// form would serve at 32 runs as two column groups on paired blocks.  0 = automatic and 2 = every sketch call of more
// than kMatrixWideQueries queries differ on the host only (which calls form such launches); 1 = never.
constexpr bool sketch_share_known(int64_t v) { return v == 0 || v == 1 || v == 2; }
// The masked form (option sketch_masked): 1 = a top-k launch with tombstones or filter masks takes
// the matrix sweep -- one block, wide, shared -- wherever the same launch without masks would; 0 = masked launches keep
// the one-query kernel.
constexpr bool sketch_masked_known(int64_t v) { return v == 0 || v == 1; }

// Ring depths of the G > 1 kernels.  A row-shape kernel of P pieces per lane exists at its shape's own depth (the
// G = 1 kernel's) and, where kGroupRingAlt divides P and differs from it, at kGroupRingAlt as well: scan_group_ring
// picks one of the two, 0 takes kGroupRingAuto where the shape has it and the shape's own depth elsewhere.
#ifndef SZG_GROUP_RING_ALT
#define SZG_GROUP_RING_ALT 6
#endif
#ifndef SZG_GROUP_RING_AUTO
#define SZG_GROUP_RING_AUTO SZG_GROUP_RING_ALT
#endif
constexpr int kGroupRingBase = 4, kGroupRingAlt = SZG_GROUP_RING_ALT, kGroupRingAuto = SZG_GROUP_RING_AUTO;
static_assert(kGroupRingAuto == kGroupRingBase || kGroupRingAuto == kGroupRingAlt, "automatic: a depth that is compiled");
constexpr bool scan_group_ring_known(int64_t v) { return v == 0 || v == kGroupRingBase || v == kGroupRingAlt; }
// depth of the G > 1 kernel of a shape whose own depth is d, P pieces per lane, under option value `want`
constexpr int scan_group_ring_of(int p, int d, int want)
{
    const bool has_alt = p % kGroupRingAlt == 0 && kGroupRingAlt != d;
    if (!has_alt) return d;
    const int w = want == 0 ? kGroupRingAuto : want;
    return w == kGroupRingAlt ? kGroupRingAlt : d;
}

// Ring depth.  HBM streams fastest with about 6-9 MB of reads in flight on the chip
// (scripts/readbw; deeper queues only lengthen the DRAM queues), so the ring is kept SHORT:
// 4 loads per lane for the any-shape kernels (8 when the candidate lists live in LDS, kp > 64,
// whose inserts stall longer).  Measured on one box, ring 8 -> 4: 1M x 768 f32 7.04 -> 7.12 TB/s,
// 4M x 768 8-bit 6.75 -> 6.97, 12.5M x 384 4-bit 6.31 -> 6.57.
//
// Row-shape kernels: lanes per row L, pieces per lane P and a ring depth D that DIVIDES P are
// compile-time constants, so after unrolling the ring every slot sits at a fixed position of
// the row: the row-finish test, the query offsets and the row jump are folded, no per-piece
// branch is left (12.5M x 384 4-bit with D = P = 3: 6.31 -> 6.77 TB/s).
#ifdef SZG_RING
constexpr int kRingShort = SZG_RING, kRingDeep = SZG_RING;
#define SZG_SHAPE_RING(d) SZG_RING
#else
constexpr int kRingShort = 4, kRingDeep = 8;
#define SZG_SHAPE_RING(d) d
#endif

// The row-shape kernels that exist, X(L, P, D) per row width: read by scan_variant (which launch takes one) and by
// the launcher of that width (which instantiates them).
#define SZG_SHAPES_4(X) X(4, 3, 3) X(4, 6, 6)    // tiled rows walk 4 lanes per row: 384 / 768 dims
#define SZG_SHAPES_8(X) X(4, 6, 6) X(4, 12, 4)
#define SZG_SHAPES_16(X)
#define SZG_SHAPES_32(X) X(8, 12, 4)             // linear rows, 8 lanes per row; (8, 24) unrolled over a whole row
                                                 // spills registers and measured slower than any-shape
#define SZG_SHAPES_64(X)

// What scan_variant decides from: one launch of the one-sweep scan.
struct ScanPlanIn {
    int qbits;
    RowMap map;
    bool tiled;
    int kp;                 // candidates kept per list (a collect launch keeps none: 0)
    bool collect;
    bool masked;
    int ring;               // tuning hook: >= 8 forces the deep ring (0 = chosen from kp)
    bool no_shape_kernels;  // tuning hook: always take the any-shape kernel
    int group = 1;          // the scan_group option (0 = automatic)
    int n_queries = 1;      // the launch's
    int block = 256;        // its threads
    int planes = 3;         // digit planes of a group's query images (which have to fit 64 KiB of LDS with the lists)
    int group_ring = 0;     // the scan_group_ring option (0 = automatic)
    int matrix_opt = 1;     // the sketch_matrix option (1 = off, what callers that do not know it get)
    bool norms = false;     // the launch has resident row norms (ScanArgs::row_norm) -- the matrix sweep needs them
    int select_opt = 0;     // the sketch_select option
    int wide_opt = 1;       // the sketch_wide option (1 = never, what callers that do not know it get)
    int share_opt = 1;      // the sketch_share option (1 = never, what callers that do not know it get)
    int masked_opt = 0;     // the sketch_masked option (0 = off, what callers that do not know it get)
};
ScanVariant scan_variant(const ScanPlanIn &in);

// LDS bytes launch_scan needs for (qbits, map, kp, block) at `group` queries per row read; planes = 2: the images of a
// group (group > 1, 8-bit rows) hold two digit planes
// matrix: the matrix sweep's column blocks (ScanVariant::matrix_blocks) -- per block kMatrixQueries
// two-plane images laid out for the matrix cores, their constants, and kMatrixQueries x waves lists of kp entries
// (its collect form keeps no lists: kp = 0, the images and constants alone -- 48.4 KiB for two blocks at 768 dimensions)
size_t scan_lds_bytes(int qbits, const RowMap &m, int kp, int block, int group = 1, int planes = 3, int matrix = 0);

// Merge n_lists sorted lists of kp candidates into ceil(n_lists/merge_fan(kp)) lists.
int merge_fan(int kp);
// Short lists (the sketch sweep; launch_merge_short, kernels.h): n_lists <= 1024 sorted block lists of m < kp entries per
// query that fit one block's LDS (merge_short_lds: the lists, each group of 64's kp best, a drop bound per group)
size_t merge_short_lds(int n_lists, int m, int kp);
bool merge_short_fits(int n_lists, int m, int kp);
// The selection's buffer: words of LDS the kernel compacts the entries under its threshold into (the tournament's
// per-group result lists, less two control words), and the most entries its bitonic network sorts -- the largest power
// of two that fits.  More entries under the threshold than that: the tournament.  (0: the launch always takes it.)
constexpr int merge_short_cap(int n_lists, int kp) { return (n_lists + 63) / 64 * kp - 2; }
constexpr int merge_short_sorts(int n_lists, int kp)
{
    int s = 0;
    for (int p = 1; p <= merge_short_cap(n_lists, kp); p <<= 1) s = p;
    return s;
}

}  // namespace szg
