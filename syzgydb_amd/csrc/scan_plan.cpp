// scan_plan.cpp -- the decisions of the one-sweep scan (scan_plan.h), host arithmetic only; one copy per library.
#include "scan_plan.h"

namespace szg {

static constexpr int kWave = 64;
static constexpr size_t kLdsMax = 64u * 1024u;

// The instantiation a launch takes.  Row-shape kernels serve unmasked sweeps over dense maps whose lists stay in
// registers; everything else is the any-shape kernel, with the deep ring when the lists live in LDS (kp > 64).
ScanVariant scan_variant(const ScanPlanIn &in)
{
    const RowMap &m = in.map;
    ScanVariant v{};
    [[maybe_unused]] int shape_p = 0;  // pieces per lane of the row-shape kernel taken
    v.deep = ((!in.collect && in.kp > 64) || in.ring >= 8) ? 1 : 0;
    v.ring_depth = v.deep ? kRingDeep : kRingShort;
    v.nontemporal = (m.L >= 8 || in.tiled) ? 1 : 0;  // whole 128-byte lines per load instruction (load_piece)
    if (!in.masked && m.dense && m.L * m.gpw == kWave && !in.no_shape_kernels && !v.deep) {
#define SZG_IS_SHAPE(l, p, d)                  \
    if (m.L == l && m.P == p) {                \
        v.shaped = l * 100 + p;                \
        v.ring_depth = SZG_SHAPE_RING(d);      \
        shape_p = p;                           \
    }
        switch (in.qbits) {
        case 4: SZG_SHAPES_4(SZG_IS_SHAPE) break;
        case 8: SZG_SHAPES_8(SZG_IS_SHAPE) break;
        case 16: SZG_SHAPES_16(SZG_IS_SHAPE) break;
        case 32: SZG_SHAPES_32(SZG_IS_SHAPE) break;
        default: SZG_SHAPES_64(SZG_IS_SHAPE) break;
        }
#undef SZG_IS_SHAPE
    }
    // Queries scored per row read (option scan_group; 0 = kScanGroupAuto): 8-bit top-k sweeps without masks whose lists
    // stay in registers (v.deep: kp > 64, or the deep ring asked for).  No larger than the launch can fill -- 1 query
    // takes G = 1, 2 take G = 2 -- and than fits 64 KiB of LDS beside the block's lists.
    v.group = 1;
    if (in.qbits == 8 && !in.collect && !in.masked && !v.deep) {
        int g = in.group == 0 ? kScanGroupAuto : in.group;
        if (g != 2 && g != 4) g = 1;
        while (g > 1 && g / 2 >= in.n_queries) g /= 2;
        while (g > 1 && scan_lds_bytes(in.qbits, m, in.kp, in.block, g, in.planes) > kLdsMax) g /= 2;
        v.group = g;
        // The grouped row-shape kernels spend G times the arithmetic per piece, so a slot of the ring comes round
        // G times later than in the G = 1 kernel: they carry a depth of their own (option scan_group_ring).
        if (g > 1 && v.shaped) v.ring_depth = scan_group_ring_of(shape_p, v.ring_depth, in.group_ring);
    }
    // The matrix sweep (kernels_scan_mx.hip; option sketch_matrix): unmasked 8-bit sweeps with the short ring over TILED
    // rows of whole 64-byte steps, whose queries carry two digit planes and whose rows' norms are resident, under
    // scan_group = 0 only (1, 2 and 4 name the VALU kernels).  From kMatrixMinQueries queries on (sketch_matrix = 2: from
    // one); a lone query of an automatic launch keeps the G = 1 kernel.  Top-k launches keep lists of 1 .. 64 entries.
    // Its collect form (radius searches through the sketch) keeps none, so neither kp nor the
    // selection matter, and the two-block form needs the images and constants alone (48.4 KiB at 768 dimensions).  A
    // launch that must keep the one-query collect kernel (a query swept again on its own) says matrix_opt = 1.
    // A masked top-k launch takes it under sketch_masked = 1 (the masked form: the same launches, the same LDS -- the
    // masks need none); a masked collect launch never does.
    const int list_kp = in.collect ? 0 : in.kp;
    const bool masked_form = in.masked && in.masked_opt == 1 && !in.collect;
    if (in.qbits == 8 && (!in.masked || masked_form) && !v.deep && (in.collect || in.kp >= 1) && in.tiled && m.r16 > 0 && m.r16 % 4 == 0 &&
        in.planes == 2 && in.norms && in.group == 0 && in.matrix_opt != 1 &&
        in.n_queries >= (in.matrix_opt == 2 ? 1 : kMatrixMinQueries) && in.block >= kWave && in.block <= 256 &&
        in.block % kWave == 0 && scan_lds_bytes(in.qbits, m, list_kp, in.block, kMatrixQueries, in.planes, 1) <= kLdsMax) {
        v.matrix = 1;
        v.masked = masked_form ? 1 : 0;
        v.matrix_steps = matrix_steps_form(m.r16 / 4);
        v.group = kMatrixQueries;
        v.shaped = 0;
        v.ring_depth = v.matrix_steps == 12 ? 6 : (v.matrix_steps == 6 ? 3 : 4);
        // its selection (option sketch_select): short lists as row lists, one candidate into each of the 16 per round
        v.row_lists = !in.collect && matrix_row_lists(in.kp, in.select_opt) ? 1 : 0;
        // The wide form (option sketch_wide): a launch of 17 .. kMatrixWideQueries queries with row lists (or none)
        // scores two column blocks per row read where both blocks' images, constants and lists fit 64 KiB of LDS; where
        // they do not (768 dimensions with lists of 16), the launch keeps one block and walks its queries in groups of 16.
        if ((in.collect || v.row_lists) && in.wide_opt != 1 && in.n_queries > kMatrixQueries &&
            in.n_queries <= kMatrixWideQueries &&
            scan_lds_bytes(in.qbits, m, list_kp, in.block, kMatrixWideQueries, in.planes, 2) <= kLdsMax) {
            v.wide = 1;
            v.group = kMatrixWideQueries;
        }
        // The shared form (option sketch_share): a top-k launch of 33 .. kMatrixShareQueries queries under exactly the
        // conditions of the wide form -- row lists, the two-block LDS -- as two column groups of 32 on paired blocks.
        if (v.row_lists && in.wide_opt != 1 && in.share_opt != 1 && in.n_queries > kMatrixWideQueries &&
            in.n_queries <= kMatrixShareQueries &&
            scan_lds_bytes(in.qbits, m, list_kp, in.block, kMatrixWideQueries, in.planes, 2) <= kLdsMax) {
            v.share = 1;
            v.group = kMatrixWideQueries;
        }
    }
    return v;
}

size_t scan_lds_bytes(int qbits, const RowMap &m, int kp, int block, int group, int planes, int matrix)
{
    // per column block: 16 two-plane images (32 bytes per piece and query) | qscale, qconst, qnorm2 | 16 x waves lists
    // (kp = 0, its collect form: a fourth word per query, the threshold, and no lists)
    if (matrix)
        return (size_t)matrix * kMatrixQueries *
               ((size_t)m.r16 * 32 + (kp == 0 ? 4 : 3) * sizeof(float) + (size_t)(block / kWave) * kp * sizeof(uint64_t));
    // per query of a group: query image + per-wave candidate lists; per-wave lists of row steps that survive the masks
    // (the two-plane images exist in the G > 1 kernels only: a lone query stages the whole image, its h plane all zero)
    const size_t image = qbits == 8 && group > 1 && planes == 2 ? (size_t)m.r16 * 32 : query_lds_bytes(qbits, m.r16);
    return (size_t)group * (image + (size_t)(block / kWave) * kp * sizeof(uint64_t)) +
           (size_t)(block / kWave) * kStepList * sizeof(uint32_t);
}

int merge_fan(int kp)
{
    if (kp <= 128) return kWave;                       // tournament: one list per lane
    return kp >= 4096 ? 2 : (8192 / kp < 32 ? 8192 / kp : 32);  // rank merge, <= 64 KiB of LDS
}

size_t merge_short_lds(int n_lists, int m, int kp)
{
    const size_t groups = (size_t)(n_lists + kWave - 1) / kWave;
    return ((size_t)n_lists * m + groups * kp + groups) * sizeof(uint64_t);
}

bool merge_short_fits(int n_lists, int m, int kp)
{
    return n_lists >= 1 && n_lists <= 16 * kWave && m >= 1 && m < kp && merge_short_lds(n_lists, m, kp) <= kLdsMax;
}

}  // namespace szg
