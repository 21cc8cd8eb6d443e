// kernels_scan_mx.hip -- the one-sweep scan's matrix form: up to 16 queries of a launch scored
// per row read, on the matrix cores, with the one-sweep kernel's output contract (sorted block lists of a.kp entries).
//
// Serves unmasked top-k sweeps over TILED 8-bit rows of whole 64-byte steps whose queries carry two digit planes
// (ScanArgs::planes == 2), with resident norms (ScanArgs::row_norm) and lists in registers (kp <= 64): today the
// sketch index.  scan_variant (scan_plan.cpp) decides; everything else keeps scan_kernel.
// With -DSZG_MX_COLLECT the file builds the COLLECT form instead (objects of their own): the same
// pass over the rows and the same keys, no lists -- every (query, row) pair whose key is at or below the query's
// threshold is appended to that query's buffer (radius searches through the sketch, scan_radius.cpp).
//
// The pass over the rows is mq_score_i8s_kernel's (kernels_mq_i8.hip): one wave per tile of 16 rows; the B operand of
// a 64-byte step is the row bytes as loaded (lane = chunk * 16 + row holds 16 consecutive elements) xor 0x80808080, the
// A operand the same elements of a digit plane of 16 queries (lane = chunk * 16 + query) from an image in LDS.  Both
// operands use the same lane -> K mapping, so the products pair element with element.  One v_mfma_i32_16x16x64_i8 per
// plane and step: two per step, where the grouped VALU kernel spends 8 v_dot4 per query, row and piece.  After a tile,
// lane (chunk c, row t) holds the exact integer plane sums M, L of queries 4c .. 4c + 3 against row t.
//
// Keys.  v' = v - 128, n = 2 v' + 1, Q = 128 m + l (|Q| <= 16000), so sum Q n = 2 (128 M + L) + sum Q.  M and L are
// exact integers.  The float chain from there is: one conversion of 128 M + L (the shaped kernels combine the planes
// as integers, |128 M + L| <= 16000 * 128 * 64 * STEPS < 2^31 for STEPS <= 16; the any-STEPS kernel takes
// fmaf(128, float(M), float(L)): two conversions and one fused rounding), fmaf(2, dot, qconst), and then cosine:
// the product with qscale, the reciprocal square root of the resident norm (itself one conversion and one addition)
// and the last product -- Euclidean: -2 qscale, qnorm2 + norm and one fmaf.  At most 8 roundings of values bounded by
// Qmax * 128 * dim in units of sum v n, where key_eps' integer branch (scan_query.cpp) allows for 16: the keys of
// this kernel stay inside that branch's bound for Qmax = 16000, and the same operations as RowAcc<8>::key_of form them.
// They are NOT bit-identical to the grouped kernel's, which rounds four per-lane partial sums before adding them.
//
// Selection.  Each lane keeps the current worst_key of its four queries; a tile pays one compare per (row, query) pair
// and ONE ballot, and only a tile with a passing lane goes on to the exact 64-bit inserts.  Two forms, a template
// argument (ROWS; scan_variant decides, option sketch_select):
//  * row lists (a.kp <= kRowListMax = 16): the 16 rows a tile offers to query 4c + r already sit
//    in the 16 lanes of lane-row c, so that query's list lives there too -- four RowLists (device_lists.h), slot r of
//    lane-row c the list of query 4c + r, lane (c, j) entry j: 8 registers for the 16 lists.  A round takes one ballot
//    per slot, retires the first passing lane of every lane-row (its key comes over the LDS crossbar, its row number
//    is the tile's first plus its lane), counts the entries below it within the lane-row, shifts by row_shr:1 and
//    refreshes the lane-row's worst entry: up to 16 inserts per round, no scalar round trip, the four slots four
//    independent chains; a slot none of whose lanes has a candidate left is skipped (measured: the same at 16 live
//    queries, 3 % faster at one to three).  At most 16 rounds per tile, the bound in the loop itself.  There is no
//    serial route beside the rounds for tiles with few passing lanes: launches of one to four live queries, where
//    few lanes pass in every tile, measure the same under both forms, so it has nothing to win.
//    The lanes of a slot that still have a candidate are a 64-bit wave mask in scalar registers (a round's test is one
//    scalar AND).  A CROWDED tile -- kBulkMin passing (query, row) pairs of the wave or more, option sketch_bulk: a
//    wave's first few tiles, which would take 16, 9, 7 ... rounds -- skips the rounds: every slot with a passing lane
//    is merged whole with its 16 candidates by a fixed sorting network in the lane-row (RowList::merge_tile; DESIGN.md
//    4.5 item 11).
//  * serial inserts (16 < a.kp <= 64, or sketch_select = 1): per wave and query a WaveList of a.kp entries in
//    registers (16 lists, one VGPR pair each), offered to query by query, one candidate at a time.
// The row-list form also exists with TWO column blocks (NB = 2; DESIGN.md 4.5 item 10, option sketch_wide): a launch of
// 17 .. 32 queries scores 32 per row read -- four matrix instructions per step on one load and one xor of the row
// bytes, eight RowLists per lane-row -- where both blocks' images, constants and lists fit 64 KiB of LDS.
// An insert is a set operation on unique entries: both forms leave the same lists bit for bit.  At the end of a group
// the lists go to the same LDS slots and are merged per query into the block's sorted list: exactly the block's best
// a.kp rows, as scan_kernel leaves them.
#include "kernels.h"
#include "device_lists.h"
#ifdef SZG_MX_MASKED
#include "mask_tiles.h"
#endif

#ifndef SZG_SCAN_METRIC
#error "kernels_scan_mx.hip needs SZG_SCAN_METRIC (0 or 1)"
#endif
// The row lists keep the pending lanes of every slot as 64-bit wave masks (finish_tile: left[], act[]).  The SLP
// vectorizer pairs such masks into <2 x i64> values and the gfx950 instruction selector of ROCm 7.2's clang dies on them
// (a segmentation fault in InstrEmitter::AddRegisterOperand, in whichever kernel form the pairing hits).  This file is
// compiled with -fno-slp-vectorize, and -DSZG_MX_NO_SLP beside it says so (Makefile MX_FLAGS).
#ifndef SZG_MX_NO_SLP
#error "kernels_scan_mx.hip: compile with -fno-slp-vectorize -DSZG_MX_NO_SLP (the Makefile's MX_FLAGS)"
#endif

namespace szg {

namespace {

typedef int v4i32 __attribute__((ext_vector_type(4)));
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

constexpr int kMxQ = kMatrixQueries;

// one 64-byte step of 16 tiled rows is one contiguous KiB read once per pass: stream it past the caches (a template
// fact -- a run-time flag is folded into one plain load, see mq_device.h)
template <bool NT>
__device__ __forceinline__ u32x4 load_rows(const uint8_t *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    else return *reinterpret_cast<const u32x4 *>(p);
}

// ring depth (16-byte loads a lane keeps in flight) of the shaped kernels; divides STEPS
#ifndef SZG_MX_S12_RING
#define SZG_MX_S12_RING 6
#endif
#ifndef SZG_MX_S6_RING
#define SZG_MX_S6_RING 3
#endif
// the rounds of the row lists skip a slot none of whose lanes has a candidate left
#ifndef SZG_MX_ROUND_SKIP
#define SZG_MX_ROUND_SKIP 1
#endif
template <int STEPS>
constexpr int mx_ring()
{
    return STEPS == 12 ? SZG_MX_S12_RING : (STEPS == 6 ? SZG_MX_S6_RING : 4);
}

// STEPS = 64-byte steps per row, a compile-time fact (12, 6: the tile's steps are unrolled, slot = step % D, the A
// operands travel one phase ahead in a double buffer) or 0: any whole-step row, a rotating ring of 4.
// ROWS: the wave's 16 lists are four RowLists (a.kp <= kRowListMax), else 16 WaveLists -- a template fact, so that the
// tile loop of either form carries no trace of the other.
// NB: column blocks of 16 queries scored per row read, 1 or 2 (the wide form, row lists only).
// A group is 16 NB queries.  The image, the constants and the lists gain a block index; per 64-byte step the row bytes
// are loaded and XORed once and feed 2 NB matrix instructions (planes m, l of each block, the same B operand), every
// block with accumulators and double-buffered A operands of its own.  After a tile lane (c, t) holds the sums of
// queries 16 b + 4 c + r against row t: lane-row c keeps 4 NB RowLists, slot 4 b + r the list of that query.  The
// keys of a (query, row) pair are formed by the same operations as with one block: bit-identical.
// (the shaped one-block row-list kernels run four waves per SIMD: their bound is 128 registers, said here so that the
// whole-tile merge cannot cost them that row by a register or two)
// COLLECT: the collect form (radius searches through the sketch).  The tile loop, the operand
// traffic, the ring, the norms and the key chain are the ones above -- a (query, row) pair gets the same key bit for
// bit -- but there are no lists: a slot's key is tested against its query's threshold (ScanArgs::thr_ukeys, staged in
// LDS beside the constants) and the passing rows are appended to that query's buffer, as scan_kernel's collect form
// does it.  Instantiated with ROWS set (neither list form is alive in it).
// With -DSZG_MX_SHARE the file builds the SHARED form of the two-block row-list kernel instead (objects of their own;
// DESIGN.md 4.5 item 13, option sketch_share): a launch of 33 .. kMatrixShareQueries queries as two column groups of 32 on
// a grid of 2 S blocks.  share_map (scan_plan.h) gives a block its row slice and its group; the block stages only its
// own group's image, constants and lists and takes one turn of the loop over the groups; the two blocks of a slice walk
// the same tiles, so whichever reads a line second finds it in its XCD's L2 or in the Infinity Cache.  No block waits
// for another and nothing depends on where or when a partner runs.  The keys are formed by the same operations.
// With -DSZG_MX_MASKED the file builds the MASKED forms of the top-k kernels instead (objects of their own, and with
// -DSZG_MX_SHARE on top the masked shared form; DESIGN.md 4.5 item 14, option sketch_masked): launches with tombstones
// (a.live_bits) or filter masks (query q of the launch: a.allow_bits + q * a.allow_stride).  A tile's 16 rows are one
// aligned 16-bit slice of a mask word (mask_tiles.h).  The pre-filter's pass[r] gains "this row is eligible for this slot's
// query": an ineligible row never enters a list, never moves a bound and never counts towards a crowded tile, so a block
// leaves exactly its best a.kp ELIGIBLE rows, as scan_kernel's masked forms do.  The live slice and the allow slice of a
// launch whose queries share one mask (no allow words, or stride 0) are wave-uniform: mask_next_tile walks the wave from
// its tile to the next one of its stride with an eligible row -- scalar loads, nothing per lane -- and a tile without one
// is neither loaded nor multiplied; the ring's look-ahead points at the tile the walk found.  With per-query masks the
// walk sees the live words alone, and lane t < 4 NB of every lane-row fetches slot t's 16-bit allow slice beside the norm
// (the idle columns read the launch's last query's); the finish hands slot r's slice to the lane-row's 16 lanes.
#if defined(SZG_MX_MASKED)
#define SZG_MX_KERNEL_ARGS const ScanMaskedArgs ma
#elif defined(SZG_MX_SHARE)
#define SZG_MX_KERNEL_ARGS const ScanShareArgs sa
#else
#define SZG_MX_KERNEL_ARGS const ScanArgs a
#endif
// (the masked Euclidean 12-step one-block row-list kernel needs 10 registers more than the 128 of four waves per SIMD: it
// takes the bound of the other forms, 2 -- no kernel of this file uses scratch)
#ifdef SZG_MX_MASKED
#define SZG_MX_FOUR_WAVES(METRIC, STEPS) (!((METRIC) == kEuclidean && (STEPS) == 12))
#else
#define SZG_MX_FOUR_WAVES(METRIC, STEPS) true
#endif
template <int METRIC, int STEPS, bool NT, bool ROWS, int NB = 1, bool COLLECT = false>
__global__ __launch_bounds__(256, (ROWS && NB == 1 && STEPS != 0 && SZG_MX_FOUR_WAVES(METRIC, STEPS)) ? 4 : 2) void scan_mx_kernel(SZG_MX_KERNEL_ARGS)
{
#ifdef SZG_MX_MASKED
    static_assert(!COLLECT, "the masked forms: top-k");
    const ScanArgs &a = ma.a;
    [[maybe_unused]] const ScanMaskedArgs &sa = ma;  // (the shared form reads sa.hi)
#endif
#ifdef SZG_MX_SHARE
    static_assert(NB == 2 && ROWS && !COLLECT, "the shared form: two column blocks, row lists, top-k");
#ifndef SZG_MX_MASKED
    const ScanArgs &a = sa.a;
#endif
    const ShareSlot slot = share_map(blockIdx.x, gridDim.x);
#endif
    static_assert(NB == 1 || (NB == 2 && ROWS), "two column blocks: row lists only");
    static_assert(!COLLECT || ROWS, "the collect form is instantiated once per shape");
    static_assert(16 * NB <= kMatrixWideQueries, "the launch's constants are sized by kMatrixWideQueries");
    constexpr int kQ = kMxQ * NB;  // queries of a group
    constexpr int NS = 4 * NB;     // slots (queries) per lane
    static_assert(STEPS == 0 || (STEPS % 2 == 0 && STEPS % mx_ring<STEPS>() == 0), "even phases, ring divides the row");
    static_assert(STEPS <= 16, "the integer plane combine needs |128 M + L| < 2^31");
    extern __shared__ __align__(16) uint8_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = blockDim.x >> 6;
    const int steps = STEPS ? STEPS : (int)a.steps;
    // row lists: tiles with this many passing pairs or more are merged whole (option sketch_bulk)
    [[maybe_unused]] const uint32_t bulk_min = sketch_bulk_min(a.bulk);
    const int n16 = steps * 2 * 64;  // 16-byte words of a block's image: [step][plane m, l][chunk * 16 + query]

    // LDS: the group's image [block] | qscale, qconst, qnorm2 [16 NB] | the wave lists [query of the group][wave][kp]
    uint4 *image = reinterpret_cast<uint4 *>(smem);
    // (the collect form: | the thresholds' ordered keys [16 NB], and no lists)
    float *qtab = reinterpret_cast<float *>(smem + (size_t)NB * n16 * 16);
    [[maybe_unused]] uint64_t *lists = reinterpret_cast<uint64_t *>(smem + (size_t)NB * n16 * 16 + 3 * kQ * sizeof(float));

    const int trow = lane & 15;
    const int c = lane >> 4;
    const RowLayout lay{a.pitch, a.tiled, a.steps};
    const uint64_t n_tiles = ((uint64_t)a.n_rows + 15) / 16;
#ifdef SZG_MX_SHARE
    const uint64_t tile_stride = (uint64_t)slot.slices * nwaves;
    const uint64_t tile_first = (uint64_t)slot.slice * nwaves + wave;
#else
    const uint64_t tile_stride = (uint64_t)gridDim.x * nwaves;
    const uint64_t tile_first = (uint64_t)blockIdx.x * nwaves + wave;
#endif
    // (the masked forms walk on "no further tile": no fixed count)
    [[maybe_unused]] const uint64_t n_it = tile_first < n_tiles ? (n_tiles - tile_first + tile_stride - 1) / tile_stride : 0;
    const uint64_t last_row = a.n_rows ? (uint64_t)a.n_rows - 1 : 0;
    // (a row past the end of the last tile, or a tile past the wave's last: a valid row, read and discarded)
    auto row_ptr = [&](uint64_t tile) -> const uint8_t * {
        return a.rows + piece_offset(lay, min(tile * 16 + trow, last_row), (uint32_t)c);
    };
#ifdef SZG_MX_MASKED
    // the words the walk reads (wave-uniform); per-query masks are read per slot instead
    const bool per_query = a.allow_bits != nullptr && a.allow_stride != 0;
    const uint64_t *const m_live = a.live_bits;
    const uint64_t *const m_allow = per_query ? nullptr : a.allow_bits;
    uint32_t m_slice = 0xFFFFu;  // the eligible rows of the tile at hand, by the walk's words
    uint32_t m_esl = 0xFFFFu;    // per-query masks: the allow slice of slot (lane & (NS - 1)) of this lane-row
#endif

#ifdef SZG_MX_SHARE
    // (one turn, for the block's own group; the launcher admits 33 .. 64 queries: both groups hold a live query)
    for (int qi = (int)slot.group * kQ, turn = 0; turn < 1 && qi < a.n_queries; turn++) {
#else
    for (int qi = 0; qi < a.n_queries; qi += kQ) {
        if (qi) __syncthreads();  // the previous group's lists have been merged, its image is free
#endif
        // column x of the group holds query min(qi + x, n_queries - 1): the idle columns of the launch's last group score
        // its last query again, offer nothing and write no lists
        for (int i0 = tid; i0 < NB * n16; i0 += blockDim.x) {
            const int blk = NB == 1 ? 0 : (i0 >= n16 ? 1 : 0), i = i0 - blk * n16;
            const int x = i & 15, chunk = (i >> 4) & 3, p = (i >> 6) & 1, st = i >> 7;
            const int q = min(qi + blk * kMxQ + x, a.n_queries - 1);
            // (the staged query is [plane h, m, l][piece]: the all-zero h plane stays behind)
            const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.query) +
                                                               (size_t)q * a.query_stride) +
                               (size_t)(1 + p) * a.map.r16 + (st * 4 + chunk);
            image[i0] = *src;
        }
#pragma unroll
        for (int x = 0; x < kQ; x++) {
            const int q = min(qi + x, a.n_queries - 1);  // (block-uniform: scalar loads of the arguments)
#ifdef SZG_MX_SHARE
            const bool hi_ = q >= kMatrixWideQueries;  // (q < kMatrixShareQueries: the launcher's bound)
            float qs = hi_ ? sa.hi.qscale[q - kMatrixWideQueries] : a.qscale[q];
            float qc = hi_ ? sa.hi.qconst[q - kMatrixWideQueries] : a.qconst[q];
            float qn = hi_ ? sa.hi.qnorm2[q - kMatrixWideQueries] : a.qnorm2[q];
#else
            float qs = a.qscale[q], qc = a.qconst[q], qn = a.qnorm2[q];
#endif
            if (a.qmeta) scan_qmeta(a.qmeta, q, &qs, &qc, &qn);  // (prepared on the card: the table holds every query)
            [[maybe_unused]] uint32_t tk = 0;
            if constexpr (COLLECT) tk = q < kMaxSweepsPerLaunch ? a.thr_ukeys[q] : a.thr_ukeys_hi[q - kMaxSweepsPerLaunch];
            if (tid == x) {
                qtab[x] = qs;
                qtab[kQ + x] = qc;
                qtab[2 * kQ + x] = qn;
                if constexpr (COLLECT) reinterpret_cast<uint32_t *>(qtab)[3 * kQ + x] = tk;
            }
        }
        // ROWS: slot 4 b + r of lane-row c is the list of query 16 b + 4 c + r; else one whole-wave list per query (the
        // unused form is dead code: no registers)
        RowList rls[NS];
        WaveList wls[kMxQ];
        if constexpr (COLLECT) {
        } else if constexpr (ROWS) {
#pragma unroll
            for (int r = 0; r < NS; r++) rls[r].init();
        } else {
#pragma unroll
            for (int x = 0; x < kMxQ; x++) wls[x].init(lists, a.kp, lane);  // (register lists: flushed by hand below)
        }
        float wk[NS];  // worst_key of this lane's queries (+inf while a list fills); collect: their thresholds
        [[maybe_unused]] uint32_t tu[NS];  // collect: the thresholds' ordered keys (the exact test)
        bool live[NS];
#pragma unroll
        for (int r = 0; r < NS; r++) {
            wk[r] = __builtin_inff();
            live[r] = qi + (r >> 2) * kMxQ + c * 4 + (r & 3) < a.n_queries;
        }
        float qsv[NS], qcv[NS], qnv[NS];
#ifdef SZG_MX_MASKED
        // per-query masks: the mask of this lane's slot as 16-bit slices, one per tile (little-endian words)
        const uint16_t *m_q16 = nullptr;
        if (per_query) {
            const int s_ = trow & (NS - 1);
            const int q_ = min(qi + (s_ >> 2) * kMxQ + c * 4 + (s_ & 3), a.n_queries - 1);
            m_q16 = reinterpret_cast<const uint16_t *>(a.allow_bits + (size_t)q_ * a.allow_stride);
        }
#endif

        // ---- the tile is done: keys of 4 NB queries x 1 row per lane, one compare each, one ballot for the tile
        auto finish_tile = [&](uint64_t tile, const v4i32 (&accM)[NB], const v4i32 (&accL)[NB], float norm) {
            const uint64_t row = tile * 16 + trow;
            const bool row_ok = row < a.n_rows;
            float key[NS];
            bool pass[NS];
            bool any = false;
            [[maybe_unused]] const float inv = __frsqrt_rn(norm);
#ifdef SZG_MX_MASKED
            // is this lane's row eligible for slot r's query?  (one mask: the walk's slice; per-query masks: slot r's slice
            // sits in lane r of the lane-row)
            bool elig[NS];
#pragma unroll
            for (int r = 0; r < NS; r++) elig[r] = ((m_slice >> trow) & 1u) != 0;
            if (per_query) {  // (wave-uniform)
#pragma unroll
                for (int r = 0; r < NS; r++) {
                    // (every lane takes part in the exchange: no short-circuit in front of it -- a lane whose row is dead
                    // still holds a slot's slice)
                    const uint32_t sl = (uint32_t)__shfl((int)m_esl, (lane & 48) + r);
                    elig[r] = elig[r] & (((sl >> trow) & 1u) != 0);
                }
            }
#endif
#pragma unroll
            for (int r = 0; r < NS; r++) {
                float dot;
                if constexpr (STEPS != 0) dot = (float)(accM[r >> 2][r & 3] * 128 + accL[r >> 2][r & 3]);
                else dot = fmaf(128.0f, (float)accM[r >> 2][r & 3], (float)accL[r >> 2][r & 3]);
                const float d2 = fmaf(2.0f, dot, qcv[r]);  // sum Q n
                float k_;
                if constexpr (METRIC == kCosine) k_ = -(d2 * qsv[r]) * inv;
                else k_ = fmaf(-2.0f * qsv[r], d2, qnv[r] + norm);
                k_ = fminf(k_, 3.0e38f);
                key[r] = k_;
#ifdef SZG_MX_MASKED
                pass[r] = row_ok && live[r] && elig[r] && !(k_ > wk[r]);
#else
                pass[r] = row_ok && live[r] && !(k_ > wk[r]);
#endif
                any = any || pass[r];
            }
            if (!__ballot(any)) return;
            if constexpr (COLLECT) {
                // Behind the tile's one ballot: per slot the exact test, and one ballot whose four 16-lane slices belong
                // to four different queries (lane-row c of slot r: query 16 (r >> 2) + 4 c + (r & 3)).  The first hit
                // lane of a slice claims the slice's popcount on its query's counter, every hit lane writes its entry at
                // base + rank while that is inside the buffer; the counter keeps counting past the cap (the host's
                // overflow sign).  Rows past n_rows and idle columns never pass the pre-filter (row_ok, live).
#pragma unroll
                for (int r = 0; r < NS; r++) {
                    const uint32_t uk = ordered_key(key[r]);
                    const bool hit = pass[r] && uk <= tu[r];
                    const uint64_t b = __ballot(hit);
                    if (!b) continue;  // (wave-uniform)
                    const uint32_t slice = (uint32_t)(b >> (16 * c)) & 0xFFFFu;
                    const uint32_t rank = (uint32_t)__popc(slice & ((1u << trow) - 1u));
                    const size_t q = (size_t)(qi + (r >> 2) * kMxQ + c * 4 + (r & 3));
                    uint32_t base = 0;
                    if (hit && rank == 0) base = atomicAdd(a.collect_count + q * kCandCountStride, (uint32_t)__popc(slice));
                    base = __shfl(base, slice ? c * 16 + __ffs((int)slice) - 1 : lane);
                    if (hit) {
                        const uint32_t idx = base + rank;
                        if (idx < a.collect_cap) a.collect_buf[q * a.collect_cap + idx] = ((uint64_t)uk << 32) | (uint32_t)row;
                    }
                }
            } else if constexpr (ROWS) {
                // Rounds: the 16 rows offered to query 4 c + r sit in the 16 lanes of lane-row c, so one round retires
                // one passing lane of every lane-row and slot -- up to 16 NB inserts, 4 NB independent chains (the slots).
                // A round retires a lane of every lane-row that still has one: 16 rounds always suffice, and the bound
                // stands in the loop itself.
                uint32_t uk[NS];
#pragma unroll
                for (int r = 0; r < NS; r++) uk[r] = ordered_key(key[r]);
                const uint32_t row0 = (uint32_t)(tile * 16);
                // the lanes whose candidate has not been retired, slot by slot, as scalar masks
                uint64_t left[NS];
#pragma unroll
                for (int r = 0; r < NS; r++) left[r] = __ballot(pass[r]);
                uint32_t n_pass = 0;
#pragma unroll
                for (int r = 0; r < NS; r++) n_pass += (uint32_t)__popcll(left[r]);
                // A crowded tile (a wave's first few: its lists are filling, or their bounds still loose) would pay as
                // many rounds as its fullest lane-row and slot has passing lanes.  From bulk_min passing pairs on -- a
                // scalar count -- every slot with a passing lane is merged whole instead (RowList::merge_tile).
                if (n_pass >= bulk_min) {
#pragma unroll
                    for (int r = 0; r < NS; r++) {
                        if (!left[r]) continue;  // (wave-uniform)
                        rls[r].merge_tile(pass[r], uk[r], row0, lane, a.kp);
                        wk[r] = rls[r].worst_key();
                    }
                    return;
                }
                for (int round = 0; round < 16; round++) {
                    uint64_t act[NS];
                    uint64_t act_any = 0;
#pragma unroll
                    for (int r = 0; r < NS; r++) {
                        act[r] = left[r] & __ballot((((uint64_t)uk[r] << 32) | (uint32_t)row) < rls[r].worst);
                        act_any |= act[r];
                    }
                    if (!act_any) break;
#pragma unroll
                    for (int r = 0; r < NS; r++) {
                        // (wave-uniform: late tiles have a few passing lanes, in one or two of the slots)
                        if (SZG_MX_ROUND_SKIP && !act[r]) continue;
                        rls[r].round(act[r], left[r], uk[r], row0, lane, a.kp);
                    }
                }
#pragma unroll
                for (int r = 0; r < NS; r++) wk[r] = rls[r].worst_key();
            } else {
#pragma unroll
                for (int x = 0; x < kMxQ; x++) {
                    const int r = x & 3;
                    const bool have = pass[r] && c == (x >> 2);
                    if (!__ballot(have)) continue;
                    wls[x].offer(have, ((uint64_t)ordered_key(key[r]) << 32) | (uint32_t)row, lane);
                    if (c == (x >> 2)) wk[r] = wls[x].worst_key;
                }
            }
        };
        auto read_consts = [&]() {
#pragma unroll
            for (int r = 0; r < NS; r++) {
                const int x = (r >> 2) * kMxQ + c * 4 + (r & 3);  // this slot's column of the group
                qsv[r] = qtab[x];
                qcv[r] = qtab[kQ + x];
                qnv[r] = qtab[2 * kQ + x];
                if constexpr (COLLECT) {  // the float pre-filter's threshold takes the place of the lists' worst key
                    tu[r] = reinterpret_cast<const uint32_t *>(qtab)[3 * kQ + x];
                    wk[r] = key_from_ordered(tu[r]);
                }
            }
        };
        const v4i32 *qimg = reinterpret_cast<const v4i32 *>(smem) + lane;

        if constexpr (STEPS != 0) {
            constexpr int D = mx_ring<STEPS>();
            u32x4 ring[D];
            v4i32 accM[NB], accL[NB];
#pragma unroll
            for (int b = 0; b < NB; b++) accM[b] = accL[b] = v4i32{0, 0, 0, 0};
#ifdef SZG_MX_MASKED
            // (a wave with no eligible tile: mt.tile == n_tiles -- the ring's first loads read the last row and nobody
            // consumes them)
            MaskTile mt = mask_next_tile(m_live, m_allow, tile_first, tile_stride, n_tiles);
            uint64_t tile = mt.tile;
#else
            uint64_t tile = tile_first;
#endif
            const uint8_t *cur = row_ptr(tile);
            // the ring's first D steps (D <= STEPS: all inside the first tile); the rows do not depend on the image
#pragma unroll
            for (int u = 0; u < D; u++) {
                ring[u] = load_rows<NT>(cur + (size_t)u * 1024);
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();  // the image and the constants are complete
            read_consts();
            // the A operands travel one phase (step) ahead of the matrix instructions that use them, in a double buffer
            v4i32 qbuf[2][NB][2];
            auto read_phase = [&](int st_, v4i32 (&dst)[NB][2]) {
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    dst[b][0] = qimg[((b * STEPS + st_) * 2 + 0) * 64];
                    dst[b][1] = qimg[((b * STEPS + st_) * 2 + 1) * 64];
                }
            };
            read_phase(0, qbuf[0]);
#ifdef SZG_MX_MASKED
            while (tile < n_tiles) {
                // the look-ahead points at the next tile with an eligible row (none: this tile again, as below)
                const MaskTile nx = mask_next_tile(m_live, m_allow, tile + tile_stride, tile_stride, n_tiles);
                const uint8_t *nxt = nx.tile < n_tiles ? row_ptr(nx.tile) : cur;
                m_slice = mt.slice;
                if (per_query) m_esl = m_q16[tile];  // (arrives with the norm)
#else
            for (uint64_t it = 0; it < n_it; it++, tile += tile_stride) {
                // (past the wave's last tile: its own tile again -- D loads nobody consumes)
                const uint8_t *nxt = it + 1 < n_it ? row_ptr(tile + tile_stride) : cur;
#endif
                const float norm = a.row_norm[min(tile * 16 + trow, last_row)];  // arrives while the tile's steps run
#pragma unroll
                for (int st = 0; st < STEPS; st++) {
                    const u32x4 v_ = ring[st % D];
                    // this slot's next load: the step D ahead, in this tile or the next
                    ring[st % D] = st + D < STEPS ? load_rows<NT>(cur + (size_t)(st + D) * 1024)
                                                  : load_rows<NT>(nxt + (size_t)(st + D - STEPS) * 1024);
                    __builtin_amdgcn_sched_barrier(0);
                    v4i32 bop;
                    bop[0] = (int)(v_.x ^ 0x80808080u);
                    bop[1] = (int)(v_.y ^ 0x80808080u);
                    bop[2] = (int)(v_.z ^ 0x80808080u);
                    bop[3] = (int)(v_.w ^ 0x80808080u);
                    read_phase((st + 1) % STEPS, qbuf[(st + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    // (the tile's first matrix instructions start from a literal zero: no accumulator clearing per tile)
#pragma unroll
                    for (int b = 0; b < NB; b++) {
                        accM[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qbuf[st & 1][b][0], bop, st == 0 ? v4i32{0, 0, 0, 0} : accM[b], 0, 0, 0);
                        accL[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(qbuf[st & 1][b][1], bop, st == 0 ? v4i32{0, 0, 0, 0} : accL[b], 0, 0, 0);
                    }
                }
                finish_tile(tile, accM, accL, norm);
                cur = nxt;
#ifdef SZG_MX_MASKED
                mt = nx;
                tile = nx.tile;
#endif
            }
        } else {
            constexpr int D = 4;
            u32x4 ring[D];
            v4i32 accM[NB], accL[NB];
#pragma unroll
            for (int b = 0; b < NB; b++) accM[b] = accL[b] = v4i32{0, 0, 0, 0};
#ifdef SZG_MX_MASKED
            // the issue side and the consume side walk the same tiles, each on its own (the walk is a function of the
            // words); a tile past the walk's end (n_tiles) is the last row again, loaded and never consumed
            const MaskTile mt0 = mask_next_tile(m_live, m_allow, tile_first, tile_stride, n_tiles);
            uint64_t itile = mt0.tile, ctile = mt0.tile;
            uint32_t c_slice = mt0.slice;
            int is = 0, cs = 0;
            const uint8_t *iptr = row_ptr(mt0.tile);
            float norm = 0.0f;
#define SZG_MX_NEXT_I itile = mask_next_tile(m_live, m_allow, itile + tile_stride, tile_stride, n_tiles).tile;
#define SZG_MX_NEXT_C                                                                                      \
    {                                                                                                      \
        const MaskTile n_ = mask_next_tile(m_live, m_allow, ctile + tile_stride, tile_stride, n_tiles);    \
        ctile = n_.tile;                                                                                   \
        c_slice = n_.slice;                                                                                \
    }
#define SZG_MX_TILE_START if (per_query) m_esl = m_q16[ctile];
#define SZG_MX_TILE_END m_slice = c_slice;
#else
            const uint64_t NP = n_it * (uint64_t)steps;  // 64-byte steps of this wave's tiles, walked as one stream
            uint64_t itile = tile_first, ctile = tile_first;
            int is = 0, cs = 0;
            const uint8_t *iptr = row_ptr(tile_first);
            float norm = 0.0f;
#define SZG_MX_NEXT_I itile += tile_stride;
#define SZG_MX_NEXT_C ctile += tile_stride;
#define SZG_MX_TILE_START
#define SZG_MX_TILE_END
#endif
#define SZG_MX_ISSUE(u)                                                                  \
    {                                                                                    \
        ring[u] = load_rows<NT>(iptr);                                                   \
        if (++is == steps) {                                                             \
            is = 0;                                                                      \
            SZG_MX_NEXT_I                                                                \
            iptr = row_ptr(itile);                                                       \
        } else {                                                                         \
            iptr += 1024;                                                                \
        }                                                                                \
    }
#define SZG_MX_CONSUME(u)                                                                \
    {                                                                                    \
        const u32x4 v_ = ring[u];                                                        \
        if (cs == 0) {                                                                   \
            norm = a.row_norm[min(ctile * 16 + trow, last_row)];                         \
            SZG_MX_TILE_START                                                            \
        }                                                                                \
        v4i32 bop_;                                                                      \
        bop_[0] = (int)(v_.x ^ 0x80808080u);                                             \
        bop_[1] = (int)(v_.y ^ 0x80808080u);                                             \
        bop_[2] = (int)(v_.z ^ 0x80808080u);                                             \
        bop_[3] = (int)(v_.w ^ 0x80808080u);                                             \
        _Pragma("unroll") for (int b_ = 0; b_ < NB; b_++) {                             \
            const v4i32 am_ = qimg[((b_ * steps + cs) * 2 + 0) * 64];                    \
            const v4i32 al_ = qimg[((b_ * steps + cs) * 2 + 1) * 64];                    \
            accM[b_] = __builtin_amdgcn_mfma_i32_16x16x64_i8(am_, bop_, accM[b_], 0, 0, 0); \
            accL[b_] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al_, bop_, accL[b_], 0, 0, 0); \
        }                                                                                \
        if (++cs == steps) {                                                             \
            SZG_MX_TILE_END                                                              \
            finish_tile(ctile, accM, accL, norm);                                        \
            _Pragma("unroll") for (int b_ = 0; b_ < NB; b_++)                            \
                accM[b_] = accL[b_] = v4i32{0, 0, 0, 0};                                 \
            cs = 0;                                                                      \
            SZG_MX_NEXT_C                                                                \
        }                                                                                \
    }
#ifndef SZG_MX_MASKED
            uint64_t issued = D, consumed = 0;
#endif
#pragma unroll
            for (int u = 0; u < D; u++) {
                SZG_MX_ISSUE(u)
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();  // the image and the constants are complete
            read_consts();
#ifdef SZG_MX_MASKED
            // (no fixed count of steps: the stream ends on "no further tile")
            while (ctile < n_tiles) {
#pragma unroll
                for (int u = 0; u < D; u++) {
                    if (ctile < n_tiles) {
                        SZG_MX_CONSUME(u)
                        SZG_MX_ISSUE(u)
                    }
                }
            }
#else
            while (consumed + 2 * D <= NP) {
#pragma unroll
                for (int u = 0; u < D; u++) {
                    SZG_MX_CONSUME(u)
                    SZG_MX_ISSUE(u)
                    __builtin_amdgcn_sched_barrier(0);
                }
                consumed += D;
                issued += D;
            }
            while (consumed < NP) {
#pragma unroll
                for (int u = 0; u < D; u++) {
                    if (consumed < NP) {
                        SZG_MX_CONSUME(u)
                        consumed++;
                        if (issued < NP) {
                            SZG_MX_ISSUE(u)
                            issued++;
                        }
                    }
                }
            }
#endif
#undef SZG_MX_ISSUE
#undef SZG_MX_CONSUME
#undef SZG_MX_NEXT_I
#undef SZG_MX_NEXT_C
#undef SZG_MX_TILE_START
#undef SZG_MX_TILE_END
        }

        // block-wide k-select over the waves' lists, query by query
        if constexpr (COLLECT) {
        } else if constexpr (ROWS) {
#pragma unroll
            for (int r = 0; r < NS; r++)
                if (trow < a.kp)
                    lists[((size_t)((r >> 2) * kMxQ + c * 4 + (r & 3)) * nwaves + wave) * a.kp + trow] = rls[r].mine;
        } else {
#pragma unroll
            for (int x = 0; x < kMxQ; x++)
                if (lane < a.kp) lists[((size_t)x * nwaves + wave) * a.kp + lane] = wls[x].mine;
        }
        if constexpr (!COLLECT) {
            __syncthreads();
            for (int x = 0; x < kQ && qi + x < a.n_queries; x++)  // (block-uniform)
#ifdef SZG_MX_SHARE
                block_merge_lists(lists + (size_t)x * nwaves * a.kp, nwaves, a.kp,
                                  a.block_lists + ((size_t)(qi + x) * slot.slices + slot.slice) * a.kp, tid, blockDim.x);
#else
                block_merge_lists(lists + (size_t)x * nwaves * a.kp, nwaves, a.kp,
                                  a.block_lists + ((size_t)(qi + x) * gridDim.x + blockIdx.x) * a.kp, tid, blockDim.x);
#endif
        }
        // loads and stores share one vmcnt on gfx9: drain the list stores once per group, so that the next group's ring
        // gets counted waits (as scan_kernel does)
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    }
}

#if defined(SZG_MX_MASKED) && defined(SZG_MX_SHARE)
template <int STEPS>
hipError_t launch_mxms_steps(const ScanMaskedArgs &s, int grid, int block, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true, 2>), dim3(grid), dim3(block), lds, stream, s);
    return hipGetLastError();
}
#elif defined(SZG_MX_MASKED)
template <int STEPS>
hipError_t launch_mxm_steps(const ScanMaskedArgs &s, bool rows, bool wide, int grid, int block, size_t lds, hipStream_t stream)
{
    if (wide) hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true, 2>), dim3(grid), dim3(block), lds, stream, s);
    else if (rows) hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true>), dim3(grid), dim3(block), lds, stream, s);
    else hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, false>), dim3(grid), dim3(block), lds, stream, s);
    return hipGetLastError();
}
#elif defined(SZG_MX_SHARE)
// the rows' loads of the shared form: streamed past the caches like the two-block form's (1), or plain (0) -- the second
// reader of a line has to find it on the die (DESIGN.md 6, round 15 keeps the measured choice)
#ifndef SZG_MX_SHARE_NT
#define SZG_MX_SHARE_NT 1
#endif
template <int STEPS>
hipError_t launch_mxs_steps(const ScanShareArgs &s, int grid, int block, size_t lds, hipStream_t stream)
{
    hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, SZG_MX_SHARE_NT != 0, true, 2>), dim3(grid), dim3(block), lds, stream, s);
    return hipGetLastError();
}
#elif !defined(SZG_MX_COLLECT)
template <int STEPS>
hipError_t launch_mx_steps(const ScanArgs &a, bool rows, bool wide, int grid, int block, size_t lds, hipStream_t stream)
{
    if (wide) hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true, 2>), dim3(grid), dim3(block), lds, stream, a);
    else if (rows) hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true>), dim3(grid), dim3(block), lds, stream, a);
    else hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, false>), dim3(grid), dim3(block), lds, stream, a);
    return hipGetLastError();
}
#else
template <int STEPS>
hipError_t launch_mxc_steps(const ScanArgs &a, bool wide, int grid, int block, size_t lds, hipStream_t stream)
{
    if (wide) hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true, 2, true>), dim3(grid), dim3(block), lds, stream, a);
    else hipLaunchKernelGGL((scan_mx_kernel<SZG_SCAN_METRIC, STEPS, true, true, 1, true>), dim3(grid), dim3(block), lds, stream, a);
    return hipGetLastError();
}
#endif

}  // namespace

}  // namespace szg

// (defined by its qualified name: it has to match its declaration in kernels.h)
#define SZG_CAT2(a, b) a##b
#define SZG_CAT(a, b) SZG_CAT2(a, b)
#if defined(SZG_MX_MASKED)
// the masked forms of ONE metric (objects of their own, -DSZG_MX_MASKED; with -DSZG_MX_SHARE the masked shared form)
namespace szg {
namespace {
// (scan_variant's conditions, once more, for every masked form: a launch that does not meet them must not reach these kernels)
bool mx_masked_ok(const ScanMaskedArgs &s, const ScanVariant &v, int block, size_t lds)
{
    const ScanArgs &a = s.a;
    return v.matrix && v.masked && s.masked == 1 && scan_masked(a) && v.nontemporal && a.tiled && a.steps != 0 &&
           (int)a.steps * 4 == a.map.r16 && a.planes == 2 && a.row_norm && a.block_lists && a.kp >= 1 && a.kp <= 64 && !a.collect &&
           a.n_queries >= 1 && block >= 64 && block <= 256 && block % 64 == 0 && lds <= 64u * 1024u &&
           v.matrix_steps == matrix_steps_form((int)a.steps) && (v.row_lists != 0) == matrix_row_lists(a.kp, a.select);
}
}  // namespace
}  // namespace szg
#if defined(SZG_MX_SHARE)
hipError_t szg::SZG_CAT(launch_scan_mxms_m, SZG_SCAN_METRIC)(const ScanMaskedArgs &s, const ScanVariant &v, int grid, int block,
                                                           size_t lds, hipStream_t stream)
{
    const ScanArgs &a = s.a;
    // exactly the planned form: row lists, 33 .. 64 queries, an even grid -- share_map pairs its blocks -- the two-block LDS
    if (!mx_masked_ok(s, v, block, lds) || !v.share || v.wide || !v.row_lists || a.kp > kRowListMax || a.wide == 1 ||
        s.hi.share == 1)
        return hipErrorInvalidValue;
    if (a.n_queries <= kMatrixWideQueries || a.n_queries > kMatrixShareQueries) return hipErrorInvalidValue;
    if (grid < 2 || grid % 2) return hipErrorInvalidValue;
    if (lds != scan_lds_bytes(8, a.map, a.kp, block, kMatrixWideQueries, a.planes, 2)) return hipErrorInvalidValue;
    switch (v.matrix_steps) {
    case 12: return launch_mxms_steps<12>(s, grid, block, lds, stream);
    case 6: return launch_mxms_steps<6>(s, grid, block, lds, stream);
    default: return launch_mxms_steps<0>(s, grid, block, lds, stream);
    }
}
#else
hipError_t szg::SZG_CAT(launch_scan_mxm_m, SZG_SCAN_METRIC)(const ScanMaskedArgs &s, const ScanVariant &v, int grid, int block,
                                                          size_t lds, hipStream_t stream)
{
    const ScanArgs &a = s.a;
    if (!mx_masked_ok(s, v, block, lds) || v.share) return hipErrorInvalidValue;
    const bool rows = v.row_lists != 0;
    // the wide form: row lists, 17 .. kMatrixWideQueries queries, exactly the two-block LDS; every other launch holds at most
    // kMaxSweepsPerLaunch
    const bool wide = v.wide != 0;
    if (wide && (!rows || a.wide == 1 || a.n_queries <= kMatrixQueries || a.n_queries > kMatrixWideQueries ||
                 lds != scan_lds_bytes(8, a.map, a.kp, block, kMatrixWideQueries, a.planes, v.matrix_blocks())))
        return hipErrorInvalidValue;
    if (!wide && (a.n_queries > kMaxSweepsPerLaunch || lds != scan_lds_bytes(8, a.map, a.kp, block, kMatrixQueries, a.planes, 1)))
        return hipErrorInvalidValue;
    switch (v.matrix_steps) {
    case 12: return launch_mxm_steps<12>(s, rows, wide, grid, block, lds, stream);
    case 6: return launch_mxm_steps<6>(s, rows, wide, grid, block, lds, stream);
    default: return launch_mxm_steps<0>(s, rows, wide, grid, block, lds, stream);
    }
}
#endif
#elif defined(SZG_MX_SHARE)
// the shared form of ONE metric (objects of their own, -DSZG_MX_SHARE)
hipError_t szg::SZG_CAT(launch_scan_mxs_m, SZG_SCAN_METRIC)(const ScanShareArgs &s, const ScanVariant &v, int grid, int block,
                                                          size_t lds, hipStream_t stream)
{
    const ScanArgs &a = s.a;
    // (scan_variant's conditions, once more; and exactly the planned form: unmasked top-k with row lists, 33 .. 64 queries,
    // an even grid -- share_map pairs its blocks -- and the two-block LDS)
    if (!v.matrix || !v.share || v.wide || !v.row_lists || !v.nontemporal || !a.tiled || a.steps == 0 ||
        (int)a.steps * 4 != a.map.r16 || a.planes != 2 || !a.row_norm || !a.block_lists || a.kp < 1 || a.kp > kRowListMax ||
        !matrix_row_lists(a.kp, a.select) || a.collect || scan_masked(a) || a.wide == 1 || s.hi.share == 1 || block < 64 ||
        block > 256 || block % 64 || lds > 64u * 1024u)
        return hipErrorInvalidValue;
    if (a.n_queries <= kMatrixWideQueries || a.n_queries > kMatrixShareQueries) return hipErrorInvalidValue;
    if (grid < 2 || grid % 2) return hipErrorInvalidValue;
    if (lds != scan_lds_bytes(8, a.map, a.kp, block, kMatrixWideQueries, a.planes, 2)) return hipErrorInvalidValue;
    if (v.matrix_steps != matrix_steps_form((int)a.steps)) return hipErrorInvalidValue;
    switch (v.matrix_steps) {
    case 12: return launch_mxs_steps<12>(s, grid, block, lds, stream);
    case 6: return launch_mxs_steps<6>(s, grid, block, lds, stream);
    default: return launch_mxs_steps<0>(s, grid, block, lds, stream);
    }
}
#elif defined(SZG_MX_COLLECT)
// the collect form of ONE metric (objects of their own, -DSZG_MX_COLLECT): v names the form
hipError_t szg::SZG_CAT(launch_scan_mxc_m, SZG_SCAN_METRIC)(const ScanArgs &a, const ScanVariant &v, int grid, int block,
                                                          size_t lds, hipStream_t stream)
{
    // (scan_variant's conditions, once more: a launch that does not meet them must not reach these kernels)
    if (!v.matrix || !v.nontemporal || !a.tiled || a.steps == 0 || (int)a.steps * 4 != a.map.r16 || a.planes != 2 ||
        !a.row_norm || !a.collect || !a.collect_buf || !a.collect_count || a.n_queries < 1 || scan_masked(a) || block < 64 ||
        block > 256 || block % 64 || lds > 64u * 1024u)
        return hipErrorInvalidValue;
    if (v.matrix_steps != matrix_steps_form((int)a.steps)) return hipErrorInvalidValue;
    // the wide form: a launch of 17 .. kMatrixWideQueries queries (the constants' and thresholds' arrays hold that many)
    // and exactly the two-block LDS; every other launch holds at most kMaxSweepsPerLaunch
    const bool wide = v.wide != 0;
    if (wide && (a.wide == 1 || a.n_queries <= kMatrixQueries || a.n_queries > kMatrixWideQueries)) return hipErrorInvalidValue;
    if (!wide && a.n_queries > kMaxSweepsPerLaunch) return hipErrorInvalidValue;
    if (lds != scan_lds_bytes(8, a.map, 0, block, wide ? kMatrixWideQueries : kMatrixQueries, a.planes, v.matrix_blocks()))
        return hipErrorInvalidValue;
    switch (v.matrix_steps) {
    case 12: return launch_mxc_steps<12>(a, wide, grid, block, lds, stream);
    case 6: return launch_mxc_steps<6>(a, wide, grid, block, lds, stream);
    default: return launch_mxc_steps<0>(a, wide, grid, block, lds, stream);
    }
}
#else
// the matrix sweep of ONE metric (one object each, as the scan objects): v names the form (ScanVariant::matrix_steps)
hipError_t szg::SZG_CAT(launch_scan_mx_m, SZG_SCAN_METRIC)(const ScanArgs &a, const ScanVariant &v, int grid, int block,
                                                         size_t lds, hipStream_t stream)
{
    // (scan_variant's conditions, once more: a launch that does not meet them must not reach these kernels)
    if (!v.matrix || !v.nontemporal || !a.tiled || a.steps == 0 || (int)a.steps * 4 != a.map.r16 || a.planes != 2 ||
        !a.row_norm || a.kp < 1 || a.kp > 64 || a.collect || scan_masked(a) || block < 64 || block > 256 || block % 64 ||
        lds > 64u * 1024u)
        return hipErrorInvalidValue;
    if (v.matrix_steps != matrix_steps_form((int)a.steps)) return hipErrorInvalidValue;
    // (row lists hold at most kRowListMax entries: a longer list must never reach that form)
    if ((v.row_lists != 0) != matrix_row_lists(a.kp, a.select)) return hipErrorInvalidValue;
    const bool rows = v.row_lists != 0;
    // the wide form: row lists, a launch of 17 .. kMatrixWideQueries queries (the constants' arrays hold that many),
    // option sketch_wide not 1, and exactly the two-block LDS; every other launch holds at most kMaxSweepsPerLaunch
    const bool wide = v.wide != 0;
    if (wide && (!rows || a.wide == 1 || a.n_queries <= kMatrixQueries || a.n_queries > kMatrixWideQueries ||
                 lds != scan_lds_bytes(8, a.map, a.kp, block, kMatrixWideQueries, a.planes, v.matrix_blocks())))
        return hipErrorInvalidValue;
    if (!wide && a.n_queries > kMaxSweepsPerLaunch) return hipErrorInvalidValue;
    switch (v.matrix_steps) {
    case 12: return launch_mx_steps<12>(a, rows, wide, grid, block, lds, stream);
    case 6: return launch_mx_steps<6>(a, rows, wide, grid, block, lds, stream);
    default: return launch_mx_steps<0>(a, rows, wide, grid, block, lds, stream);
    }
}
#endif  // SZG_MX_COLLECT
