// kernels.h -- launch-side declarations shared by the HIP kernel files and the
// C-ABI implementation (scan_api.cpp).  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_plan.h"

namespace szg {

constexpr int kEuclidean = 0;  // collection.go:186-189
constexpr int kCosine = 1;

// A candidate is one packed 64-bit word: (ordered key << 32) | local row.
// Unsigned comparison of the word orders by key, ties by lower row.
constexpr uint64_t kInvalidCand = 0xFFFFFFFFFFFFFFFFull;

// float -> uint32 so that unsigned order == float order (NaN sorts last).
__host__ __device__ inline uint32_t ordered_key(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float key_from_ordered(uint32_t u)
{
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// Where a row's 16-byte pieces live in the resident mirror.
//   linear: row-major, `pitch` bytes per row.
//   tiled : tiles of 16 rows; inside a tile the 64-byte step s of all 16 rows is one
//           contiguous KiB ([step][row & 15][piece & 3]).  A wave instruction that reads one
//           64-byte step of 16 rows -- the walk of short rows and the MFMA operand layout of
//           the shared sweeps -- then reads 1 KiB contiguous instead of sixteen 64-byte
//           segments (a bare read of which tops out at 6.2 TB/s, scripts/readbw).  Needs
//           pitch % 64 == 0; rows are allocated in multiples of 16.
struct RowLayout {
    uint32_t pitch;
    uint32_t tiled;
    uint32_t steps;  // pitch / 64 when tiled
};
__host__ __device__ inline uint64_t piece_offset(const RowLayout &l, uint64_t row, uint32_t j)
{
    if (!l.tiled) return row * l.pitch + (uint64_t)j * 16;
    return (row >> 4) * ((uint64_t)l.steps * 1024) + (uint64_t)(j >> 2) * 1024 + (row & 15) * 64 + (j & 3) * 16;
}
__host__ __device__ inline uint64_t layout_bytes(const RowLayout &l, uint64_t rows)
{
    return l.tiled ? ((rows + 15) >> 4) * ((uint64_t)l.steps * 1024) : rows * (uint64_t)l.pitch;
}

// Hit counters of the fused selection sit one per 128-byte line: the waves claim their slots
// with returning atomics, mostly at the end of the sweep, and atomics on one line serialise
// (~12 ns each) -- 48 counters in two lines made a 46 us tail on a 190 us sweep.
constexpr int kCandCountStride = 32;  // 32-bit words

// Exact integer shared sweep (mq_score_i8_kernel): the query as kMqPlanes balanced int8 digit
// planes of radix 128.  Every plane costs one MFMA and one 16-byte LDS read per query block
// and 64-byte row step; 2 planes (|Q| <= 16000, ~14 bits) keep the certification bound at
// ~2e-4 in cosine units, still far inside the gap between the k-th and the kp-th best key.
#ifndef SZG_MQ_PLANES
#define SZG_MQ_PLANES 2
#endif
constexpr int kMqPlanes = SZG_MQ_PLANES;
constexpr double kMqQmax = kMqPlanes == 2 ? 16000.0 : 1000000.0;

// per-query constants of the integer paths, as the row finish consumes them
struct QConst {
    float qscale, qconst, qnorm2, norm_bias;
};

struct ScanArgs {
    const uint8_t *rows;        // resident mirror: n_rows x pitch bytes, little-endian elements
    uint32_t n_rows;
    uint32_t pitch;             // bytes, multiple of 16
    uint32_t tiled, steps;      // RowLayout of `rows`
    int dim;
    RowMap map;
    const uint64_t *live_bits;  // nullable: bit r == 0 -> tombstoned
    const uint64_t *allow_bits; // nullable: bit r == 0 -> filtered out (collection.go:592)
    const void *query;          // device, piece-swizzled (see prep_query in scan_api.cpp)
    int n_queries;              // queries walked back to back by one launch
    uint32_t query_stride;      // bytes between consecutive swizzled queries
    uint32_t allow_stride;      // words between consecutive queries' allow masks
    // integer paths (4/8-bit rows): query ~ qscale * Q, qconst = sum Q, norm_bias turns
    // the row's integer sums into sum n^2 without the padding; qnorm2 = sum g^2 (euclid)
    // (sized for the matrix sweep's wide launch, kMatrixWideQueries; every other launch holds up to kMaxSweepsPerLaunch)
    float qscale[kMatrixWideQueries], qconst[kMatrixWideQueries], qnorm2[kMatrixWideQueries];
    double norm_bias;
    int no_shape_kernels;       // tuning hook: always take the any-shape kernel
    int ring;                   // tuning hook: >= 8 forces the deep ring (0 = chosen from kp)
    int mask_dense;             // masked sweep that reads every row and applies the masks at the row finish
                                // (most rows pass); 0 = rows are tested before their loads are issued
    int group;                  // option scan_group: queries of the launch scored per row read where the launch
                                // qualifies (scan_variant); 0 = automatic, 1 = one query per row read
    int kp;                     // candidates kept per list (top-k mode)
    uint64_t *block_lists;      // [n_queries][grid][kp] sorted ascending (top-k mode)
    // collect mode (radius search / escalation): every row of sweep s with key <= thr_ukeys[s] is appended to
    // collect_buf + s * collect_cap; the sweep's hit counter is collect_count[s * kCandCountStride] (it may
    // exceed collect_cap: the caller then reruns that query with a larger buffer)
    int collect;
    uint32_t thr_ukeys[kMaxSweepsPerLaunch];
    uint64_t *collect_buf;
    uint32_t collect_cap;
    uint32_t *collect_count;
    // (behind everything the kernels without groups read: their argument offsets, and so their code, stay as they were)
    const float *row_norm;      // nullable: resident norms of rows [0, n_rows) (launch_row_norms' 8-bit form).  A launch
                                // that takes a G > 1 variant reads them instead of summing the norm in the sweep.
    int planes;                 // 8-bit rows: int8 digit planes the queries carry, 3 (0 means 3) or 2 -- the h plane of
                                // the image is all zero; G > 1 variants then neither stage nor read it
    int group_ring;             // option scan_group_ring: ring depth of the G > 1 row-shape kernels that carry more than
                                // one (scan_variant); 0 = automatic
    int matrix;                 // option sketch_matrix: 0 = automatic (the matrix sweep where the launch qualifies and holds
                                // kMatrixMinQueries queries), 1 = never, 2 = wherever the shape allows, whatever the count
    int select;                 // option sketch_select: how the matrix sweep keeps its lists -- 0 = automatic (row lists
                                // where kp <= kRowListMax), 1 = the serial inserts (one WaveList per query) everywhere
    int wide;                   // option sketch_wide: 1 = a launch never takes the matrix sweep's two-block form; 0, 2 = a
                                // launch of more than kMatrixQueries queries takes it where it qualifies (the host decides
                                // which calls form such launches)
    int bulk;                   // option sketch_bulk: from how many passing (query, row) pairs on a tile of the row-list matrix
                                // sweep merges every slot whole (sketch_bulk_min) -- 0 = automatic, 1 = never, n >= 2 = n
    // collect mode of the matrix sweep's wide launch: the thresholds of sweeps kMaxSweepsPerLaunch .. kMatrixWideQueries - 1
    // (behind everything else, like row_norm: the offsets the other kernels read stay as they were)
    uint32_t thr_ukeys_hi[kMatrixWideQueries - kMaxSweepsPerLaunch];
    // (behind everything else again) null, or the constants of the launch's queries on the card, five doubles each
    // (query_prep.h, kQueryPrepMeta: written by launch_query_prep ahead of the launch on its stream; option query_prep):
    // the kernels then take float(qscale), float(qconst), float(qnorm2) of query q from qmeta[5 q + 2, 3, 4] -- the
    // conversions the host makes when it fills the arrays above, which are not read -- a shared launch all its 64
    const double *qmeta;
};
// a query's constants as the row finish consumes them, from the card's table (ScanArgs::qmeta)
__device__ inline void scan_qmeta(const double *qmeta, int q, float *qscale, float *qconst, float *qnorm2)
{
    *qscale = (float)qmeta[5 * q + 2];
    *qconst = (float)qmeta[5 * q + 3];
    *qnorm2 = (float)qmeta[5 * q + 4];
}
// the collect threshold of sweep s of a launch (s < kMatrixWideQueries)
__host__ __device__ inline uint32_t &scan_thr_ukey(ScanArgs &a, int s)
{
    return s < kMaxSweepsPerLaunch ? a.thr_ukeys[s] : a.thr_ukeys_hi[s - kMaxSweepsPerLaunch];
}

// The matrix sweep's shared launch (option sketch_share; scan_plan.h share_map) holds up to kMatrixShareQueries queries.
// What it needs beyond ScanArgs rides behind it in a struct of its own, which only the shared kernels take: ScanArgs --
// its size is part of every scan kernel's descriptor -- and with it the code of every other kernel stay as they were.
struct ScanShareHi {
    // the constants of queries kMatrixWideQueries .. kMatrixShareQueries - 1 of the launch (ScanArgs holds the first 32)
    float qscale[kMatrixShareQueries - kMatrixWideQueries], qconst[kMatrixShareQueries - kMatrixWideQueries],
        qnorm2[kMatrixShareQueries - kMatrixWideQueries];
    int share;  // option sketch_share: 1 = a launch never takes the shared form
};
struct ScanShareArgs {
    ScanArgs a;
    ScanShareHi hi;
};

inline bool scan_masked(const ScanArgs &a) { return a.live_bits != nullptr || a.allow_bits != nullptr; }
// what scan_variant decides from (scan_plan.h), for the launch `a` describes at `block` threads
inline ScanPlanIn scan_plan_in(int qbits, const ScanArgs &a, int block)
{
    ScanPlanIn in{qbits, a.map, a.tiled != 0, a.kp, a.collect != 0, scan_masked(a), a.ring, a.no_shape_kernels != 0};
    in.group = a.group;
    in.n_queries = a.n_queries;
    in.block = block;
    in.planes = a.planes;
    in.group_ring = a.group_ring;
    in.matrix_opt = a.matrix;
    in.norms = a.row_norm != nullptr;
    in.select_opt = a.select;
    in.wide_opt = a.wide;
    return in;
}
// queries per row read of the variant launch_scan takes for `a`
inline int scan_group_of(int qbits, const ScanArgs &a, int block) { return scan_variant(scan_plan_in(qbits, a, block)).group; }
// passes over the rows that launch_scan makes for `a`: one per group of its queries
inline int scan_passes(int qbits, const ScanArgs &a, int block)
{
    const int group = scan_group_of(qbits, a, block);
    return (a.n_queries + group - 1) / group;
}
// would launch_scan read resident row norms for `a`, if it had them (a G > 1 variant or the matrix sweep)?  The caller
// then asks for them (scan_row_norms) before it launches.
inline bool scan_wants_norms(int qbits, const ScanArgs &a, int block)
{
    ScanPlanIn in = scan_plan_in(qbits, a, block);
    in.norms = true;
    return scan_variant(in).group > 1;
}

// Fused dequantize + distance + select.  QBITS in {4,8,16,32,64}.
hipError_t launch_scan(int qbits, int metric, const ScanArgs &a, int grid, int block,
                       hipStream_t stream);
// The launchers behind it, one per object of the build (m0 = Euclidean, m1 = cosine), declared once for the object that
// defines one -- by its qualified name, so a definition that does not match is a compile error -- and for its caller.
// kernels_scan.hip -DSZG_QBITS=q -DSZG_SCAN_METRIC=m: every launch of that width and metric starts here
#define SZG_DECL_SCAN(q)                                                                   \
    hipError_t launch_scan_q##q##m0(const ScanArgs &a, int grid, int block, hipStream_t stream); \
    hipError_t launch_scan_q##q##m1(const ScanArgs &a, int grid, int block, hipStream_t stream);
SZG_DECL_SCAN(4) SZG_DECL_SCAN(8) SZG_DECL_SCAN(16) SZG_DECL_SCAN(32) SZG_DECL_SCAN(64)
#undef SZG_DECL_SCAN
// ... with -DSZG_GROUP_FORM=f on top: the G > 1 kernels of 8-bit rows in one form (bit 0 = two digit planes, bit 1 =
// resident norms); kernels_scan_mx.hip: the matrix sweep (mx) and, with -DSZG_MX_COLLECT, its collect form (mxc)
#define SZG_DECL_SCAN_V(name) \
    hipError_t name(const ScanArgs &a, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
#define SZG_DECL_G8(f) SZG_DECL_SCAN_V(launch_scan_g8m0f##f) SZG_DECL_SCAN_V(launch_scan_g8m1f##f)
SZG_DECL_G8(0) SZG_DECL_G8(1) SZG_DECL_G8(2) SZG_DECL_G8(3)
SZG_DECL_SCAN_V(launch_scan_mx_m0) SZG_DECL_SCAN_V(launch_scan_mx_m1)
SZG_DECL_SCAN_V(launch_scan_mxc_m0) SZG_DECL_SCAN_V(launch_scan_mxc_m1)
#undef SZG_DECL_G8
#undef SZG_DECL_SCAN_V
// The matrix sweep's shared form (kernels_scan_mx.hip with -DSZG_MX_SHARE: objects of their own): ONE launch of 33 ..
// kMatrixShareQueries top-k queries over 8-bit tiled rows, on a grid of 2 S blocks (share_map); the lists go to
// a.block_lists as [n_queries][S][a.kp].  Everything that is not exactly that form is hipErrorInvalidValue.
hipError_t launch_scan_share(int qbits, int metric, const ScanArgs &a, const ScanShareHi &hi, int grid, int block,
                             hipStream_t stream);
hipError_t launch_scan_mxs_m0(const ScanShareArgs &s, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
hipError_t launch_scan_mxs_m1(const ScanShareArgs &s, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
// what scan_variant decides from for a shared launch
inline ScanPlanIn scan_share_plan_in(int qbits, const ScanArgs &a, const ScanShareHi &hi, int block)
{
    ScanPlanIn in = scan_plan_in(qbits, a, block);
    in.share_opt = hi.share;
    return in;
}
// The matrix sweep's masked forms (option sketch_masked; kernels_scan_mx.hip with -DSZG_MX_MASKED, and with -DSZG_MX_SHARE
// on top for the shared form: objects of their own): a top-k launch with tombstones (a.live_bits) or filter masks
// (query q of the launch reads a.allow_bits + q * a.allow_stride) in the form the same launch without masks would take.
// The option rides behind ScanArgs in a struct that only these kernels take, as ScanShareHi does: ScanArgs, and with it the
// code of every other kernel, stay as they were.  hi: the shared form's constants (zero for the other forms).
struct ScanMaskedArgs {
    ScanArgs a;
    ScanShareHi hi;
    int masked;  // option sketch_masked: 1 = masked launches take the matrix sweep where they qualify
};
// what scan_variant decides from for a launch that may take a masked form (share_opt: the sketch_share option)
inline ScanPlanIn scan_masked_plan_in(int qbits, const ScanArgs &a, int share_opt, int masked_opt, int block)
{
    ScanPlanIn in = scan_plan_in(qbits, a, block);
    in.share_opt = share_opt;
    in.masked_opt = masked_opt;
    return in;
}
// ONE masked top-k launch of the matrix sweep: scan_variant must name the masked form for exactly this launch (up to 16
// queries, 17 .. 32 wide, 33 .. 64 shared: hi as launch_scan_share takes it, its `share` the option); everything else is
// hipErrorInvalidValue.  The lists go to a.block_lists as the unmasked form of the same launch leaves them.
hipError_t launch_scan_masked(int qbits, int metric, const ScanArgs &a, const ScanShareHi &hi, int masked_opt, int grid, int block,
                              hipStream_t stream);
hipError_t launch_scan_mxm_m0(const ScanMaskedArgs &s, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
hipError_t launch_scan_mxm_m1(const ScanMaskedArgs &s, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
hipError_t launch_scan_mxms_m0(const ScanMaskedArgs &s, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
hipError_t launch_scan_mxms_m1(const ScanMaskedArgs &s, const ScanVariant &v, int grid, int block, size_t lds, hipStream_t stream);
// ---- kernels_sample_mx.hip: the sample pass of a top-k search of large k through the sketch (option sketch_topk_collect;
// sample_plan.h has the arithmetic) ----------------------------------------------------------------------------------
// One launch scores sample tiles 0 .. tiles - 1 -- tile j of the sample is tile j * stride of the rows -- against the
// launch's 1 .. 16 nb queries (nb = 1, 2 column blocks) and writes keys[q * slots + 16 j + t], the ordered key of row t of
// the tile for query q, 0xFFFFFFFF where the row does not exist or is not eligible (a.live_bits; a.allow_bits: query q
// reads a.allow_bits + q * a.allow_stride).  Of `a` the rows, their layout and norms, the queries, their constants and the
// masks are read; tiled 8-bit rows in whole 64-byte steps, two-plane queries, an image of nb blocks within 64 KiB of LDS
// (sample_mx_lds_bytes) -- everything else is hipErrorInvalidValue.
struct SampleArgs {
    ScanArgs a;
    uint32_t stride, tiles, slots;  // slots = 16 * tiles
    uint32_t *keys;
};
size_t sample_mx_lds_bytes(uint32_t steps, int nb);
hipError_t launch_sample_mx(int metric, const SampleArgs &s, int nb, int grid, int block, hipStream_t stream);
// One block per query: out[2 q] = the rank[q]-th smallest (1-based) of keys[q * slots .. + slots), out[2 q + 1] = the
// slots that hold a key; fewer of them than the rank (or rank 0): out[2 q] = 0xFFFFFFFF.
struct SampleSelectArgs {
    const uint32_t *keys;
    uint32_t slots;
    uint32_t rank[kMatrixWideQueries];
    uint32_t *out;
};
hipError_t launch_sample_select(const SampleSelectArgs &s, int n_queries, hipStream_t stream);

// ---- shared (multi-query) sweeps (mq_device.h, kernels_mq*.hip): every row width, cosine and Euclidean ----------
// queries per shared sweep: 48 (3 blocks of 16) for the int8 sweeps (4- and 8-bit rows), whose LDS images are 2-4
// bytes per element and query; 96 for the bfloat16 sweeps (16-, 32- and 64-bit rows, and 8-bit rows in batches of
// more than 48 top-k queries): 2 bytes
constexpr int kMqMaxQueries = 96;
struct MqArgs {
    const uint8_t *rows;      // resident mirror
    uint32_t n_rows;
    uint32_t pitch;
    uint32_t tiled, steps;    // RowLayout of `rows`
    int r16;                  // 16-byte pieces per row
    int dim;
    const void *queries;      // device: LDS image [piece][query block][group of 4][16 queries][4 floats]
    int n_queries;            // <= 16 * query blocks
    int metric;               // kCosine: image = q/|q|, key = -cos.  kEuclidean: image = the scan's
                              // prepared query (maxInt*q for quantized rows), key = |n - image|^2
    float qnorm2[kMqMaxQueries];  // euclid: |image_q|^2 per query
    float qsum[kMqMaxQueries];    // 8-bit rows through the bfloat16 sweep: the sum of the query's (rounded) image values
    float norm_bias;          // integer sweep: turns 4*(sum v'^2 + sum v') into sum n^2 of the real elements
    float *keys;              // out: [n_queries][key_stride] ranking keys
    size_t key_stride;        // floats, multiple of 4, >= n_rows
    const uint8_t *zero16;    // 16 zero bytes (address idle lanes read)
    // fused selection (collect != 0): instead of writing the score matrix, every (query,
    // row) whose key is <= thr[query] and whose mask bits allow it is appended to the
    // query's candidate buffer; thr comes from a sweep of a prefix of the rows
    int n_groups;                // int8 sweep: query groups of 48 one launch walks (0 / 1: one); image g at
    uint32_t group_stride;       // queries + g * group_stride bytes, thr / keys / candidates indexed by 48 g + q
    int shape_kernels;           // int8 sweep: take the row-shape-specialised kernel where one exists
    int collect;
    const float *thr;            // [n_queries]
    uint64_t *cand_buf;          // [n_queries][cand_cap]  (ordered key << 32 | row)
    uint32_t *cand_count;        // [n_queries * kCandCountStride]; may exceed cand_cap (then the batch is redone)
    uint32_t cand_cap;
    const uint64_t *live_bits;   // nullable
    const uint64_t *allow_bits;  // nullable, per query
    uint32_t allow_stride;
    const float *row_norm;       // resident row norms (launch_row_norms): 16-bit rows (nullable: the direct bfloat16
                                 // sweep then sums its own) and 8-/4-bit rows (the shape kernels REQUIRE them; without,
                                 // the any-shape kernel runs)
};
// per query: the kp best of its candidate buffer, sorted, as one list [n_queries][kp]
hipError_t launch_cand_select(const uint64_t *cand_buf, const uint32_t *cand_count, uint32_t cand_cap,
                              int kp, int n_queries, uint64_t *lists, hipStream_t stream);
// The tail of a fused-selection batch in one launch (kernels_mq.hip: cand_refine_kernel): the kp best of each query's
// collected candidates -- mode 0: by the collected key; 1 / 2 (bfloat16 sweeps, cosine / euclid): the candidates
// within the sweep's error band of the kp-th best are scored again in float32 first, band_edge[q] tells the host
// where the band ended -- followed by the query's n_sent sentinel rows: lists [n_queries][kp + n_sent].  A band that
// does not fit sets cand_count[q] to 0xFFFFFFFF (the batch is redone through the score matrix).
bool cand_refine_applies(int kp, uint32_t cand_cap, int dim, bool rescore);
hipError_t launch_cand_refine(int mode, const uint8_t *rows, RowLayout layout, int dim, const double *q64,
                              const double *qscale, const double *qnorm2, const uint64_t *cand_buf, uint32_t *cand_count,
                              uint32_t cand_cap, int kp, int n_queries, const uint64_t *sent, int n_sent,
                              uint64_t *lists, float *band_edge, int row_bits, hipStream_t stream);
// float32 re-score of the collected candidates of a bfloat16 sweep (32-bit rows, or 16-bit rows of whole 16-byte
// pieces, decoded to n = 2v - 65535): replaces the key in every candidate word; qscale[q] = 1/|q| (cosine) or the
// prepared query's scale (euclid: 1, or 65535 for 16-bit rows), the float32 query is (float)(q64 * qscale)
hipError_t launch_cand_rescore(int metric, const uint8_t *rows, RowLayout layout, int dim, const double *q64,
                               const double *qscale, uint64_t *cand_buf, const uint32_t *cand_count,
                               uint32_t cand_cap, int n_queries, int row_bits, hipStream_t stream);

// Exact integer shared sweep for 8- and 4-bit rows, both metrics (v_mfma_i32_16x16x64_i8).  MqArgs.queries is
// the image [64-byte step][digit plane h,m,l][query block][lane = chunk*16 + query][16 bytes]
// of the queries' balanced int8 digit planes (prep_query), followed by the float table
// [qscale | qconst | qnorm2][48]; MqArgs.norm_bias as ScanArgs.norm_bias.
// row_bits = 4: two B operands per piece (high / low nibbles as unsigned bytes), the image
// is [step][plane][even, odd elements][query block][lane][16 bytes] and the table's qconst
// entries hold -15 * sum Q (n = 2x - 15).
size_t mq_i8_image_bytes(int row_bits, int r16, int nb);   // digit image only
size_t mq_i8_lds_bytes(int row_bits, int r16, int nb, int groups = 1);  // groups x (image + constants + thresholds) + hit buffers
hipError_t launch_mq_score_i8(int row_bits, const MqArgs &a, int nb, int grid, hipStream_t stream);  // nb = 1..3
// bfloat16 shared sweep, both metrics (v_mfma_f32_16x16x32_bf16): 64-, 32- and 16-bit rows of any dimension in the
// row-major layout (16-bit rows with resident norms take the direct form, without them the LDS-staged one), and tiled
// 8-bit rows (whole 64-byte steps; needs MqArgs::row_norm and qsum).  MqArgs.queries is the image
// [32-element step][query block][lane = k-group*16 + query][8 bf16 = elements 8*k-group + 0..7 of the step]
// (zeros where the row has ended).  Its keys only rank: launch_cand_refine / launch_cand_rescore score again.
size_t mq_bf16_image_bytes(int row_bits, int r16, int nb);
size_t mq_bf16_lds_bytes(int row_bits, int r16, int nb);
hipError_t launch_mq_score_bf16(int row_bits, const MqArgs &a, int nb, int grid, hipStream_t stream);  // nb = 1..6
hipError_t launch_mq_select(const float *keys, size_t key_stride, uint32_t n_rows,
                            const uint64_t *live_bits, const uint64_t *allow_bits,
                            uint32_t allow_stride, int kp, int n_queries, int blocks_per_query,
                            uint64_t *block_lists, hipStream_t stream, float *thr_out = nullptr,
                            uint32_t *count_zero = nullptr);  // thr_out: one block per query; also
                                                              // writes thr[q] and zeroes count_zero[q]

// Lists are [n_queries][n_lists][kp]; the output is [n_queries][n_out][kp].
// out_stride (a merge down to ONE list per query only): entries between the queries' lists in `out` (0 = kp); the
// entries behind each list are left alone
hipError_t launch_merge(const uint64_t *in, int n_lists, int kp, int n_queries, uint64_t *out,
                        hipStream_t stream, int out_stride = 0);
// Short lists (the sketch sweep): [n_queries][n_lists][m] sorted block lists, m < kp, merged in ONE launch into the
// kp best per query at out + q * out_stride, followed by the drop bound at [kp]: the smallest m-th entry of a full
// list (kInvalidCand if none is full).  Serves where merge_short_fits (scan_plan.h) says so.
hipError_t launch_merge_short(const uint64_t *in, int n_lists, int m, int kp, int n_queries, uint64_t *out,
                              int out_stride, hipStream_t stream);

struct RerankOut {
    double dist;    // the reference's float64 distance (collection.go:812-832)
    uint32_t row;   // local row
    uint32_t ukey;  // the scan's ordered key for that row
};

// Exact float64 distances, reference operation order, for n candidates of each of
// n_queries queries: query_f64 [n_queries][dim], cands/out [n_queries][n_cands_max].
// n_cands_dev (nullable): the candidate count of query q is min(n_cands_dev[q * n_dev_stride], n_cands_max), read on
// the device (collect sweeps: the hit counters, no host round trip between the sweep and its re-rank).
// sorts each query's re-ranked hits out[q * cap .. + min(count[q * count_stride], cap)) by distance, ascending, when the
// list has 2 .. kSortHitsMax entries (longer lists are left as they are)
constexpr int kSortHitsMax = 2048;
hipError_t launch_sort_hits(RerankOut *out, const uint32_t *count, uint32_t count_stride, uint32_t cap, int n_queries,
                            hipStream_t stream);
hipError_t launch_rerank(int qbits, int metric, const uint8_t *rows, RowLayout layout, int dim,
                         const double *query_f64, const uint64_t *cands, const uint32_t *n_cands_dev,
                         uint32_t n_cands_max, int n_queries, RerankOut *out, hipStream_t stream,
                         uint32_t n_dev_stride = 0);

// The same for pairs of STORED rows (computeAverageDistance, collection.go:372-398): out[i] =
// c.distance(row left_rows[i], row (uint32)right_cands[i]), both decoded exactly on the device.
hipError_t launch_rerank_pairs(int qbits, int metric, const uint8_t *rows, RowLayout layout, int dim,
                               const uint32_t *left_rows, const uint64_t *right_cands, uint32_t n_pairs,
                               RerankOut *out, hipStream_t stream);

// ---- kernels_query_prep.hip: a sketch batch's queries prepared on the card (option query_prep) ------------------------
// From nq float64 queries of `dim` elements at d_q64 (unscaled; gs > 0: each element is divided by gs first, the
// Euclidean sketch's scale) to their 8-bit one-sweep images (qsw_bytes = 3 * r16 * 16 apart at d_qsw, `planes` digit
// planes) and constants (d_meta: qnorm, m1, qscale, qconst, qnorm2 per query), by the rule of query_prep.h: the bytes
// and bit patterns of the host form.  One workgroup per query.
hipError_t launch_query_prep(const double *d_q64, int nq, int dim, double gs, int cosine, int planes, int r16, uint32_t qsw_bytes,
                             uint8_t *d_qsw, double *d_meta, hipStream_t stream);

// Page-in transform: n_rows rows in the reference encoding at `ref` (big-endian 16/32/64-bit,
// row_bytes apart) <-> rows [first_row, first_row + n_rows) of the resident mirror `rows`.
// 8-bit sketch of float32 rows for the cosine pre-pass (kernels_exact.hip): rows [first_row, first_row + n_rows) of
// `src` (or the listed rows), written into `dst` in its resident layout; *max_ang = max over the rows of the angular
// distance row <-> sketch (bits of a double); rows without a direction or with a non-finite element are reported
hipError_t launch_sketch_build(const uint8_t *src, RowLayout src_lay, int src_bits, int dim, uint8_t *dst, RowLayout dst_lay,
                               uint64_t first_row, uint64_t n_rows, const uint32_t *row_list,
                               unsigned long long *max_ang, uint32_t *exc_rows, uint32_t *exc_count, uint32_t exc_cap,
                               double gscale, int max_only, hipStream_t stream);
// (gscale > 0: Euclidean form -- one scale for the whole collection, *max_ang = largest Euclidean distance row <->
//  sketch; max_only: report the largest finite |x_i| of the rows instead of building anything -- the bits of a float
//  for src_bits = 32, of a double for src_bits = 64 (float64 rows, option sketch_f64); any other width is refused)
hipError_t launch_repack(int qbits, uint8_t *ref, uint32_t row_bytes, uint8_t *rows, RowLayout layout,
                         uint64_t first_row, uint64_t n_rows, int to_reference, hipStream_t stream);

// Row gather (szg_index_compact / szg_index_reorder): row dst_first_row + i of `dst` = row list[i] of `src`, i < n, each
// side in its own layout (linear or tiled, r16 16-byte pieces per row); list == nullptr: the identity -- the "place"
// step from a linear stage into the resident layout.  No decode: a piece's bytes do not depend on its row's number.
hipError_t launch_gather_rows(const uint8_t *src, RowLayout src_lay, uint8_t *dst, RowLayout dst_lay, uint32_t r16,
                              const uint64_t *list, uint64_t n, uint64_t dst_first_row, hipStream_t stream);

// ---- kernels_bulk.hip: the scatters of the bulk mutations ------------------------------------------------------------
// Row scatter, the mirror image of the gather: row list[i] of `dst` = row i of `src`, i < n, each side in its own
// layout.  list is never null and holds no row twice; an entry >= dst_rows is skipped.
hipError_t launch_scatter_rows(const uint8_t *src, RowLayout src_lay, uint8_t *dst, RowLayout dst_lay, uint32_t r16,
                               const uint64_t *list, uint64_t n, uint64_t dst_rows, hipStream_t stream);
// out[list[i]] = in[i], i < n, elements of `elem` = 8 or 4 bytes (column values, row norms); an entry >= out_n is skipped
hipError_t launch_column_scatter(const void *in, uint32_t elem, const uint64_t *list, uint64_t n, void *out, uint64_t out_n,
                                 hipStream_t stream);

// Rows [dst_first_row, +n_rows) of the mirror directly in the resident layout: synthetic
// (src == nullptr, see szg_index_synth; seed_first_row indexes the PRNG stream) or
// quantized + packed from float64 vectors on the device.
hipError_t launch_synth(int qbits, uint8_t *rows, RowLayout layout, uint64_t dst_first_row, int dim,
                        uint64_t n_rows, uint64_t seed, uint64_t seed_first_row, const double *src,
                        hipStream_t stream);

// launch_synth's second form for a source that stays where the caller has it on the card: elements of type src_type
// (SZG_SRC_*: float64, float32, float16, bfloat16, aligned to the element only), row_stride elements from one source
// row to the next, destination row dst_first_row + i from source row src_index[i] (a device array; nullptr: row i).
// The bytes are launch_synth's on the values widened to float64.  n_rows * pitch / 16 must fit 2^39 (one launch).
hipError_t launch_ingest(int qbits, uint8_t *rows, RowLayout layout, uint64_t dst_first_row, int dim, uint64_t n_rows,
                         const void *data, int src_type, uint64_t row_stride, const uint64_t *src_index, hipStream_t stream);

// launch_ingest backwards (szg_index_fetch_rows_dev): entry i of the launch, i < n, is resident row src_first + i of
// `rows` -- or, with `list` (a device array), row list[i] - list_base where that is below shard_rows; other entries
// are skipped: they are another shard's -- and its dim elements are decoded exactly (decodeVector's float64), converted
// to dst_type (SZG_SRC_*: float64 as it is, float32 by one round-to-nearest-even, float16 / bfloat16 from that float32
// by one more) and stored at data[i * row_stride + e].  data is device memory of the rows' device, aligned to its
// element; the 16-byte store form is taken where data and row_stride * sizeof(element) are multiples of 16.
// n * ceil(dim * qbits / 128) must fit 2^39 (one launch).
hipError_t launch_fetch(int qbits, const uint8_t *rows, RowLayout layout, int dim, uint64_t n, const uint64_t *list,
                        uint64_t list_base, uint64_t shard_rows, uint64_t src_first, void *data, int dst_type,
                        uint64_t row_stride, hipStream_t stream);

// out[i * dim + e] = the float64 of element e of source row src_index[i] (a device array; nullptr: row i) of vectors
// in device memory as launch_ingest takes them, widened exactly: a batch of queries for the host's preparation.
hipError_t launch_widen_rows(double *out, int dim, uint64_t n, const void *data, int src_type, uint64_t row_stride,
                             const uint64_t *src_index, hipStream_t stream);

// Resident row norms (shared sweeps), out[first_row + i] for rows [first_row, first_row + n_rows) of the mirror:
// 16-bit rows (linear): the float32 sum of n^2, n = 2v - 65535, over the row's real elements, as the direct bfloat16
// sweep summed it; 8- and 4-bit rows (either layout): (float)(4 * sum (x'^2 + x')) + norm_bias, the int8 sweeps' norm.
hipError_t launch_row_norms(int bits, const uint8_t *rows, const RowLayout &lay, int dim, float norm_bias, uint64_t first_row,
                            uint64_t n_rows, float *out, hipStream_t stream);

// device float64 primitive probe (tests)
hipError_t launch_f64_probe(int op, const double *a, const double *b, double *out, uint64_t n,
                            hipStream_t stream);

// live-bit maintenance
hipError_t launch_fill_bits(uint64_t *bits, uint64_t n_rows, uint64_t n_words, hipStream_t stream);

// ---- device-resident filter masks (kernels_mask.hip): the words of one shard per launch.  A shard's mask is n_pairs
// 16-byte pairs of words (ceil(n_rows / 64) words rounded up to an even count); bits at positions >= n_rows are 0.
// bit (r - first) of the zeroed `words` is set for every listed row r in [first, first + n_rows) (64-bit atomic OR)
hipError_t launch_mask_from_rows(const uint64_t *rows, uint64_t n_listed, uint64_t first, uint64_t n_rows, uint64_t *words,
                                 hipStream_t stream);
// out = a op b (SZG_MASK_*; b null for NOT; out may be a), the tail cleared; *count += the bits set in out
hipError_t launch_mask_combine(int op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n_pairs, uint64_t n_rows,
                               uint64_t *count, hipStream_t stream);
// the per-query mask slots of a batch, n_pairs pairs each, from resident masks: src[q] null = all ones
struct MaskGatherTable {
    const uint64_t *src[kMqMaxQueries];
};
hipError_t launch_mask_gather(const MaskGatherTable &t, int n_queries, uint64_t *dst, uint64_t n_pairs, hipStream_t stream);
// a mask carried across a compaction / reorder: bit i of new_words = bit list[i] of old_words, i < n; bits at
// positions >= n of the n_pairs pairs are stored as 0 (list[i] < the rows old_words cover)
hipError_t launch_mask_gather_rows(const uint64_t *old_words, const uint64_t *list, uint64_t n, uint64_t *new_words,
                                   uint64_t n_pairs, hipStream_t stream);

// ---- kernels_column.hip: resident metadata columns, ONE shard's part per launch -------------------------------------
// Where a comparison's verdicts go: pair i of `out` = the verdicts of rows [128 i, 128 i + 128) & pair i of `present`
// (null: every row present) & pair i of `base` (null: none), bits at positions >= n_rows stored as 0;
// *count += the bits set in out.  n_rows <= 128 * n_pairs; no element at a position >= n_rows is loaded.
struct ColumnWhere {
    const uint64_t *present;
    const uint64_t *base;
    uint64_t *out;
    uint64_t n_pairs, n_rows;
    uint64_t *count;
};
constexpr int kColumnInMax = 1024;  // constants of an IN-list (held in LDS)
// op: SZG_CMP_* (EQ NE LT LE GT GE), IEEE rules
hipError_t launch_column_cmp_f64(const double *values, int op, double constant, const ColumnWhere &w, hipStream_t stream);
// sorted: device, ascending, no NaN, n_sorted <= kColumnInMax
hipError_t launch_column_in_f64(const double *values, const double *sorted, uint32_t n_sorted, const ColumnWhere &w,
                                hipStream_t stream);
// code_bits: device, ceil(n_codes / 64) words; a code >= n_codes fails
hipError_t launch_column_codes_u32(const uint32_t *values, const uint64_t *code_bits, uint32_t n_codes, const ColumnWhere &w,
                                   hipStream_t stream);
hipError_t launch_column_present(const ColumnWhere &w, hipStream_t stream);
// text columns (column_str.h): refs = one {uint32 start, uint32 len} per row into `heap` (device, 16-byte aligned, every
// reference inside it); op: SZG_CMP_* / SZG_STR_*; constant: device, ceil(len / 4) dwords, the last one zero-padded,
// len <= SZG_STR_PATTERN_MAX
hipError_t launch_column_str(const uint64_t *refs, const uint8_t *heap, int op, const uint32_t *constant, uint32_t len,
                             const ColumnWhere &w, hipStream_t stream);
// a byte automaton over each row of a text column (column_dfa.h): image = the class map and the staged table as
// dfa_stage makes them, accept_bits = ceil(n_states / 64) words, both on the device and checked by dfa_validate on the
// host.  A table of at most kDfaLdsEntries entries is walked in LDS, a larger one in global memory.
hipError_t launch_column_dfa(const uint64_t *refs, const uint8_t *heap, const uint32_t *image, const uint64_t *accept_bits,
                             uint32_t n_states, uint32_t n_classes, uint32_t start_staged, const ColumnWhere &w,
                             hipStream_t stream);

// ---- kernels_column_carry.hip: columns carried across a compaction / reorder, ONE part per launch --------------------
// out[at[i]] = values[list[i]], i < n, elements of `elem` = 8 or 4 bytes; at null: out[i]; list null: values[i]
hipError_t launch_carry_gather(const void *values, uint32_t elem, const uint64_t *list, const uint64_t *at, void *out,
                               uint64_t n, hipStream_t stream);
// A text part's rows list[0 .. n) (null: rows 0 .. n - 1): refs_out[i] = refs[list[i]], starts[i] = the lengths of
// refs_out[0 .. i) added up (64-bit), sums[carry_scan_blocks(n)] = the lengths of all of them.  sums: scratch of
// carry_scan_blocks(n) + 1 words.  Three launches, none of whose blocks waits for another.
uint64_t carry_scan_blocks(uint64_t n);
hipError_t launch_carry_ref_starts(const uint64_t *refs, const uint64_t *list, uint64_t n, uint64_t *refs_out,
                                   uint64_t *starts, uint64_t *sums, hipStream_t stream);
// The 16-byte pieces [piece0, piece0 + n_pieces) of the rows' bytes laid back to back (row i's at starts[i], `total`
// in all, zero from there on) into dst (16-byte aligned, n_pieces pieces), read from old_heap through refs (both as
// launch_carry_ref_starts left them).  Only dwords of old_heap that hold a byte of a row are read.
hipError_t launch_carry_move_bytes(const uint8_t *old_heap, const uint64_t *refs, const uint64_t *starts, uint64_t n,
                                   uint64_t total, uint64_t piece0, uint64_t n_pieces, uint8_t *dst, hipStream_t stream);
// out[at[i]] (at null: out[i]) = the reference {base + starts[i], length of refs[i]}; base + total < 2^32
hipError_t launch_carry_new_refs(const uint64_t *refs, const uint64_t *starts, uint64_t n, uint64_t base, const uint64_t *at,
                                 uint64_t *out, hipStream_t stream);

}  // namespace szg
