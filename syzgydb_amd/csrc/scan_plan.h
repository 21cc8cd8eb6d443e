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
                      // from HBM where the partner's lines are still on the die (objects of their own)
    int masked = 0;   // the matrix sweep's masked form (option sketch_masked; objects of their own): the
                      // launch has tombstones or filter masks and takes the matrix sweep all the same
    int long_rows = 0;  // the matrix sweep's long-row form (rows of kLongMinSteps .. kLongMaxSteps steps; objects of their own,
                      // kernels_scan_mx.hip -DSZG_MX_LONG): the image may take the CU's whole LDS, blocks of up to kLongBlockMax
                      // threads; set together with matrix / wide / share.  A collect launch's long form (no lists, never
                      // shared) has objects of its own again (-DSZG_MX_LONG -DSZG_MX_COLLECT)
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

// The long-row form: top-k launches -- unmasked ones, and under sketch_masked = 1 masked ones, on the
// same plan -- over rows of kLongMinSteps .. kLongMaxSteps whole
// 64-byte steps (1 024 .. 4 096 dimensions), whose image is too large for the 64 KiB the other forms keep to.  A gfx950 CU
// has 160 KiB of LDS: a form that fits half of it runs two blocks of 256 threads per CU, as every other sweep over tiled
// 8-bit rows does; a larger one runs ONE block of kLongBlockMax threads per CU, which stages the image once for its eight
// waves -- either way a SIMD holds two waves.  Chosen by shape alone; sketch_matrix = 1 and sketch_wide = 1 leave it out
// as they leave out the forms below 16 steps.  Rows that the one-block form of 64 KiB serves at the default block (up to
// 1 856 dimensions at lists of 8) keep today's plan for every launch: the long forms measured slower there (scan_variant).
constexpr int kLongMinSteps = 16, kLongMaxSteps = 64;
constexpr int kLongBlockMax = 512;
constexpr int kLongRing = 8;  // 16-byte loads a lane keeps in flight (a tile is at least two turns of the ring)
constexpr size_t kLongLdsCu = 160u * 1024u, kLongLdsHalf = kLongLdsCu / 2;
constexpr bool scan_long_steps(int r16) { return r16 % 4 == 0 && r16 / 4 >= kLongMinSteps && r16 / 4 <= kLongMaxSteps; }
// Block size and LDS of the form with `blocks` column blocks (1, or 2: wide and shared) over rows of map m whose waves
// keep lists of kp entries: one column block runs two blocks of 256 per CU where image, constants and lists fit
// kLongLdsHalf; a larger one, and every two-block form, ONE block of kLongBlockMax where they fit kLongLdsCu (the lists
// grow with the waves); else, and for rows that the one-block form of 64 KiB serves, block = 0: the form does not serve.
// The launch path (sketch_plan.h) and the plan hooks both ask here.
// kp = 0 asks for the collect form (unmasked collect launches, no lists, a fourth word per query):
// 16 blocks (2 dim + 16) bytes -- blocks of 256 at 2 048 .. 2 496 dimensions, the block of kLongBlockMax beyond and for
// two column blocks (which fit through 2 496 dimensions).
struct LongPlan {
    int block, per_cu;
    size_t lds;
};
LongPlan scan_long_plan(const RowMap &m, int kp, int blocks);

// The sample pass of a top-k search of large k through the sketch (kernels_sample_mx.hip): LDS of a launch of nb column
// blocks over rows of `steps` 64-byte steps -- per block an image of 2 KiB per step and three words per query -- and the
// form that serves it.  Within 64 KiB: blocks of up to 256 threads, as ever.  Rows whose one-block image passes 64 KiB
// (32 steps and more) take the LONG instantiation by the long sweep's rule: blocks of 256, two per CU, where one image fits
// kLongLdsHalf, else ONE block of kLongBlockMax per CU; two column blocks where they fit kLongLdsCu, on that block.  block = 0:
// no form serves (two blocks of 16 .. 31 steps, which pass 64 KiB on rows the 64 KiB forms keep; two of 40 steps and more).
constexpr size_t sample_lds_bytes(uint32_t steps, int nb)
{
    return (size_t)nb * steps * 2 * 64 * 16 + (size_t)3 * kMatrixQueries * nb * sizeof(float);
}
struct SampleShape {
    int block, per_cu;
    bool long_form;
    size_t lds;
};
constexpr SampleShape sample_shape(uint32_t steps, int nb)
{
    const size_t lds = sample_lds_bytes(steps, nb), kShort = 64u * 1024u;
    if (nb != 1 && nb != 2) return SampleShape{0, 0, false, lds};
    if (sample_lds_bytes(steps, 1) <= kShort) return lds <= kShort ? SampleShape{256, 2, false, lds} : SampleShape{0, 0, false, lds};
    if (steps > (uint32_t)kLongMaxSteps) return SampleShape{0, 0, false, lds};
    if (nb == 1 && lds <= kLongLdsHalf) return SampleShape{256, 2, true, lds};
    if (lds <= kLongLdsCu) return SampleShape{kLongBlockMax, 1, true, lds};
    return SampleShape{0, 0, false, lds};
}
// its grid over `tiles` sample tiles, one per wave and turn: within 64 KiB up to eight blocks of four waves per CU, as ever;
// a long block stages its image once, so the grid is the blocks the card holds at once
constexpr uint64_t sample_grid(uint64_t tiles, int cu_count, const SampleShape &sh)
{
    const uint64_t waves = (uint64_t)(sh.block > 0 ? sh.block : 256) / 64;
    const uint64_t need = (tiles + waves - 1) / waves, most = (uint64_t)cu_count * (sh.long_form ? (uint64_t)sh.per_cu : 8u);
    const uint64_t g = need < most ? need : most;
    return g < 1 ? 1 : g;
}
// the fit rule at its edges: 31 | 32 steps (64 KiB), 39 | 40 (half a CU; two blocks against the whole), 64 | 65 (the longest rows)
static_assert(sample_lds_bytes(32, 1) == 65728 && sample_lds_bytes(39, 2) == 160128, "2 KiB per step and block + 192 bytes");
static_assert(sample_shape(31, 1).block == 256 && !sample_shape(31, 1).long_form && sample_shape(31, 2).block == 0, "64 KiB forms");
static_assert(sample_shape(32, 1).block == 256 && sample_shape(32, 1).long_form && sample_shape(32, 1).per_cu == 2, "32 steps");
static_assert(sample_shape(39, 1).block == 256 && sample_shape(40, 1).block == kLongBlockMax && sample_shape(40, 1).per_cu == 1, "80 KiB");
static_assert(sample_shape(32, 2).block == kLongBlockMax && sample_shape(39, 2).block == kLongBlockMax && sample_shape(40, 2).block == 0,
              "two blocks: through 39 steps, on the block of 512");
static_assert(sample_shape(64, 1).block == kLongBlockMax && sample_shape(65, 1).block == 0 && sample_shape(32, 3).block == 0, "the ends");
// (256 CUs; a long block of 512: one per CU, eight waves -- 1 000 tiles are 125 blocks, 10 000 the card's 256)
static_assert(sample_grid(1000, 256, sample_shape(64, 1)) == 125 && sample_grid(10000, 256, sample_shape(64, 1)) == 256 &&
              sample_grid(10000, 256, sample_shape(32, 1)) == 512 && sample_grid(10000, 256, sample_shape(12, 1)) == 2048 &&
              sample_grid(0, 256, sample_shape(32, 1)) == 1, "the grid: the blocks the card holds at once");

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

// The forms of the matrix sweep (kernels_scan_mx.hip): one object per form and metric, named by four facts.  The table of
// the forms that exist, X(name, long rows, masked, shared, collect) -- the build's objects (kernels_scan_<name>_c / _e),
// their launchers (kernels.h) and launch_scan's route all come from it; a form's index is its place in the table.
#define SZG_MATRIX_FORMS(X)                                                                                     \
    X(mx, 0, 0, 0, 0) X(mxc, 0, 0, 0, 1) X(mxs, 0, 0, 1, 0) X(mxm, 0, 1, 0, 0) X(mxms, 0, 1, 1, 0)                  \
    X(mxl, 1, 0, 0, 0) X(mxls, 1, 0, 1, 0) X(mxlm, 1, 1, 0, 0) X(mxlms, 1, 1, 1, 0) X(mxlc, 1, 0, 0, 1)
struct MatrixForm {
    bool long_rows, masked, share, collect;
};
constexpr bool operator==(const MatrixForm &a, const MatrixForm &b)
{
    return a.long_rows == b.long_rows && a.masked == b.masked && a.share == b.share && a.collect == b.collect;
}
#define SZG_FORM_ROW(name, l, m, s, c) MatrixForm{l != 0, m != 0, s != 0, c != 0},
constexpr MatrixForm kMatrixForms[] = {SZG_MATRIX_FORMS(SZG_FORM_ROW)};
#undef SZG_FORM_ROW
constexpr int kMatrixFormCount = (int)(sizeof(kMatrixForms) / sizeof(kMatrixForms[0]));
// a form's index in the table; -1: no such form is built (a masked or shared collect form)
constexpr int matrix_form_index(const MatrixForm &f)
{
    for (int i = 0; i < kMatrixFormCount; i++)
        if (kMatrixForms[i] == f) return i;
    return -1;
}
// the form that serves a launch whose variant names the matrix sweep (v.matrix)
constexpr MatrixForm matrix_form_of(const ScanVariant &v, bool collect)
{
    return MatrixForm{v.long_rows != 0, v.masked != 0, v.share != 0, collect};
}
// What a launch of the matrix sweep has beyond its plan input: the rows' 64-byte steps as the kernel reads them
// (ScanArgs::steps), whether it has block lists (top-k) and a collect buffer with its counter (collect), its grid and LDS.
struct MatrixLaunch {
    int steps;
    bool lists, collect_out;
    int grid;
    size_t lds;
};
// The last check before a kernel of form f: scan_variant's conditions for that form, once more, on the launch as it
// stands -- a launch that does not meet every one of them must not reach the kernel (it would read or write out of bounds).
// True for exactly one form per launch that scan_variant planned, matrix_form_of's (tests/cpp/test_scan_plan.cpp).
bool matrix_launch_ok(const MatrixForm &f, const ScanPlanIn &in, const ScanVariant &v, const MatrixLaunch &l);

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
