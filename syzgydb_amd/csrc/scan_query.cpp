// scan_query.cpp -- the query as the kernels want it, and the bounds on what their arithmetic loses.
#include "scan_internal.h"
#include "key_bound.h"
#include "query_prep.h"

namespace szgi {

szg::RowMap choose_map(int r16, bool tiled)
{
    if (tiled) return szg::RowMap{r16, 4, r16 / 4, 16, 1, 1};  // one 64-byte step of 16 rows per load   // Groups of L lanes per row, P pieces per lane.
    // 1) Exact power-of-two groups (L*P == r16): every lane always holds a piece (the
    //    kernel's dense phase), reductions are DPP.  The SMALLEST such L >= 8 wins: a
    //    group still reads whole 128-byte lines per load, and the fewer lanes share a
    //    row, the more pieces each walks between two row finishes (measured on
    //    1M x 768 f32: L=8 6.80 TB/s, L=16 6.73, L=32 6.47, L=64 6.44; 8-bit: L=8 5.9 vs
    //    L=16 5.75 vs L=32 3.8).  L=4 (64-byte segments) only when nothing wider is exact.
    for (int L : {8, 16, 32, 64, 4})
        if (r16 % L == 0) return szg::RowMap{r16, L, r16 / L, 64 / L, 1, 1};
    // 2) Otherwise maximise lane utilisation, with a bonus for power-of-two groups.
    szg::RowMap best{r16, 64, (r16 + 63) / 64, 1, 1, 0};
    double best_score = -1;
    const int pmax = std::max(1, (r16 + 63) / 64 + 8);
    for (int P = 1; P <= pmax; P++) {
        const int need = (r16 + P - 1) / P;  // lanes a row needs at P pieces per lane
        if (need > 64) continue;
        int cand[2] = {need, 1};
        while (cand[1] < need) cand[1] <<= 1;  // next power of two
        for (int L : cand) {
            if (L > 64) continue;
            const int gpw = 64 / L;
            const double util = (double)gpw * r16 / (64.0 * P);
            const bool pow2 = (L & (L - 1)) == 0;
            const double score = util * (pow2 ? 1.3 : 1.0);
            if (score > best_score + 1e-9) {
                best_score = score;
                best = szg::RowMap{r16, L, P, gpw, pow2 ? 1 : 0, 0};
            }
        }
    }
    best.dense = (best.L * best.P == r16 && best.gpw * best.L == 64) ? 1 : 0;
    return best;
}

int row_format(int dim, int quant_bits, RowFormat *f)
{
    if (dim <= 0 || dim > (1 << 20)) return fail(SZG_E_INVALID, "dim out of range");
    const int64_t rb = row_bytes_of(quant_bits, dim);
    if (rb < 0) return fail(SZG_E_INVALID, "unsupported quantization (reference panics, collection.go:809)");
    f->row_bytes = (uint32_t)rb;
    f->pitch = (uint32_t)((rb + 15) & ~15ll);
    // 4- and 8-bit rows of whole 64-byte steps live in 16-row tiles (kernels.h, RowLayout): their
    // single-query walk and the shared sweeps then read 1 KiB runs instead of 64-byte segments
    // (+8-12 % on 4-bit rows, +2.5 % on 8-bit rows; float rows measured -1..0 % and stay linear:
    // scripts/dev_tiles.sh, dev_tiles_all.sh).  SZG_TILES_ALL / SZG_NO_TILES override for A/B runs.
    const bool tiled = (quant_bits <= 8 || getenv("SZG_TILES_ALL") != nullptr) && f->pitch % 64 == 0 &&
                       getenv("SZG_NO_TILES") == nullptr;
    f->layout = szg::RowLayout{f->pitch, tiled ? 1u : 0u, tiled ? f->pitch / 64u : 0u};
    f->map = choose_map((int)(f->pitch / 16), tiled);
    f->qsw_bytes = szg::query_lds_bytes(quant_bits, f->map.r16);
    return f->qsw_bytes > 48u * 1024u ? SZG_E_UNSUPPORTED : SZG_OK;
}

// round to nearest (ties away from zero), NaN -> 0, clamped to +-lim: query_prep.h's, with the rest of the 8-bit rule
inline long long round_clamp(double t, double lim) { return szg::qp_round_clamp(t, lim); }

// Query as the scan wants it (see RowAcc in kernels_scan.hip):
//  * 16/32/64-bit rows: float (double for 64-bit), pre-normalised for cosine,
//    pre-scaled by maxInt for 16-bit euclid, laid out [chunk][piece][4];
//  * 8/4-bit rows: the prepared real query v (q/|q| for cosine, maxInt*q for
//    euclid) quantized to integers Q_i = round(v_i / qscale) and split into
//    balanced digit planes (3 x int8 radix 128, or 5 x int4 radix 16), one
//    16-byte plane word per 16-byte piece of the row.
// The constants every path needs (norms of the caller's and of the prepared query); returns the largest
// |prepared element| and the scale q -> prepared query.
static double prep_query_norms(const szg_index *ix, const double *q, QMeta *meta, double *scale_out)
{
    *meta = QMeta{};
    double vmax;  // (query_prep.h: the sums in element order, vmax by std::max's rule)
    szg::qp_norms(q, ix->dim, ix->metric == SZG_COSINE ? 1 : 0, ix->bits, &meta->m1, scale_out, &meta->qnorm2, &vmax);
    meta->qnorm = szg::qp_canon(std::sqrt(meta->qnorm2));
    return vmax;
}

// Shared sweeps stage their own image of the batch; the single-query form below is only needed if a query of the
// batch escalates (a collect sweep), so a batch prepares just the constants and builds that form on demand.
void prep_query_meta(const szg_index *ix, const double *q, QMeta *meta)
{
    double scale;
    (void)prep_query_norms(ix, q, meta, &scale);
}

void prep_query(const szg_index *ix, const double *q, uint8_t *out_sw, QMeta *meta)
{
    const int dim = ix->dim, bits = ix->bits;
    const int E = 128 / bits;
    const int r16 = ix->map.r16;
    memset(out_sw, 0, ix->qsw_bytes);
    double scale;
    const double vmax = prep_query_norms(ix, q, meta, &scale);
    if (bits == 8) {  // the rule of query_prep.h, which the card follows too (option query_prep)
        meta->qscale = szg::qp_step(vmax, scan_qmax8(ix));
        meta->qconst = szg::qp_image8(q, dim, scale, meta->qscale, scan_planes(ix), r16, out_sw);
        return;
    }
    if (bits == 4) {
        const double Qmax = szg::kQmax4;
        const double qs = (vmax > 0 && std::isfinite(vmax)) ? vmax / Qmax : 1.0;
        meta->qscale = qs;
        double sumQ = 0.0;
        uint32_t *planes = reinterpret_cast<uint32_t *>(out_sw);
        for (int e = 0; e < dim; e++) {
            long long Q = round_clamp(q[e] * scale / qs, Qmax);
            sumQ += (double)Q;
            const int j = e / E, i = e % E;
            {
                // byte b of the piece holds element 2b in its high nibble, 2b+1 in the low one
                const int bb = i / 2, d = bb / 4, kb = bb % 4;
                const int t4 = 2 * kb + ((i % 2 == 0) ? 1 : 0);
                for (int x = 0; x < szg::kPlanes4; x++) {  // plane x carries the digit of weight 16^x
                    long long dig;
                    if (x < szg::kPlanes4 - 1) {
                        dig = ((Q + 8) & 15) - 8;
                        Q = (Q - dig) >> 4;
                    } else {
                        dig = Q;
                    }
                    planes[((size_t)x * r16 + j) * 4 + d] |= (uint32_t)(dig & 0xF) << (4 * t4);
                }
            }
        }
        meta->qconst = sumQ;
        return;
    }
    for (int e = 0; e < dim; e++) {
        const double v = q[e] * scale;
        const int j = e / E, i = e % E;
        if (bits == 64) {
            reinterpret_cast<double *>(out_sw)[(size_t)j * 2 + i] = v;
        } else {
            const int c = i / 4, m = i % 4;
            reinterpret_cast<float *>(out_sw)[((size_t)c * r16 + j) * 4 + m] = (float)v;
        }
    }
}

int scan_planes(const szg_index *ix)
{
    return ix->bits == 8 && ix->is_sketch && ix->sketch_planes != 3 ? 2 : 3;
}

// Bound on |scan key - real-number key| (see DESIGN.md "certification"): the arithmetic is key_bound.h's, a pure
// function of what is gathered here.
double key_eps(const szg_index *ix, double key, const QMeta &m)
{
    szg::KeyBoundIn b;
    b.dim = ix->dim;
    b.bits = ix->bits;
    b.cosine = ix->metric == SZG_COSINE ? 1 : 0;
    b.planes = scan_planes(ix);
    b.mq_planes = szg::kMqPlanes;
    b.mq = m.mq;
    b.mq_bf16 = m.mq_bf16;
    b.mq_int = m.mq_int;
    b.qnorm = m.qnorm;
    b.qnorm2 = m.qnorm2;
    b.qscale = m.qscale;
    b.mq_qscale = m.mq_qscale;
    return szg::key_bound(b, key);
}

// ---- shared sweeps: B queries share one pass of the corpus ------------

// 8-bit rows in whole 64-byte steps (the tiled layout) through the bfloat16 sweep -- their codes are exact in bfloat16,
// 96 queries share a pass instead of 48 (kernels_mq_bf16d.hip: mq_score_bf16d8_kernel).  SZG_BF16_8BIT=0 keeps them on the int8 sweep.
static bool bf16_takes_8bit(const szg_index *ix, bool radius, int nq)
{
    if (radius || nq <= 48) return false;  // (a radius IS the threshold: the band of the rounded query would be collected too)
    static const bool on = []() {
        const char *e = getenv("SZG_BF16_8BIT");
        if (getenv("SZG_NO_ROW_NORMS")) return false;  // (the kernel takes the rows' norms from the resident array)
        return e ? atoi(e) != 0 : SZG_BF16_8BIT_DEFAULT != 0;
    }();
    return on && ix->bits == 8 && ix->layout.tiled && ix->mq_bf16;
}
bool mq_uses_i8(const szg_index *ix, bool radius, int nq)
{
    return (ix->bits == 8 || ix->bits == 4) && ix->mq_i8 && !bf16_takes_8bit(ix, radius, nq);
}
// the bfloat16 sweep: 64-, 32- and 16-bit rows of any dimension (not the experimental tiled layout of wide rows), and
// tiled 8-bit rows
bool mq_uses_bf16(const szg_index *ix, bool radius, int nq)
{
    if (bf16_takes_8bit(ix, radius, nq)) return true;
    if (!ix->mq_bf16 || ix->layout.tiled) return false;
    return ix->bits == 64 || ix->bits == 32 || ix->bits == 16;
}

// round to nearest even, as v_cvt_pk_bf16_f32 does (NaN stays NaN)
uint16_t bf16_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// the prepared real query of the integer sweeps: q/|q| (cosine) or maxInt*q (euclid)
double mq_int_scale(const szg_index *ix, double m1)
{
    if (ix->metric == SZG_COSINE) return m1 > 0 ? 1.0 / std::sqrt(m1) : 0.0;
    return (double)((1u << ix->bits) - 1u);
}

// int8 sweep: quantization step, the integer query Q (dim values) and its digit sum
void prep_mq_int(const szg_index *ix, const double *q, QMeta *meta, int32_t *Qout)
{
    const double scale = mq_int_scale(ix, meta->m1);
    double vmax = 0.0;
    for (int e = 0; e < ix->dim; e++) vmax = std::max(vmax, std::fabs(q[e] * scale));
    const double Qmax = szg::kMqQmax;
    const double qs = (vmax > 0 && std::isfinite(vmax)) ? vmax / Qmax : 1.0;
    const double inv = scale / qs;
    long long sumQ = 0;
    for (int e = 0; e < ix->dim; e++) {
        const long long Q = round_clamp(q[e] * inv, Qmax);
        Qout[e] = (int32_t)Q;
        sumQ += Q;
    }
    meta->mq_int = true;
    meta->mq_qscale = qs;
    meta->mq_qconst = (double)sumQ;
}

int mq_blocks(const szg_index *ix, int nq, bool radius)
{   // query blocks of 16 the batch gets (nq = the queries left in the call), or 0 when the shared sweep does not apply
    if (!ix->multi_query || nq < ix->mq_min) return 0;
    const bool bf16 = mq_uses_bf16(ix, radius, nq), i8 = mq_uses_i8(ix, radius, nq);
    if (!bf16 && !i8) return 0;  // (switched off, or the experimental tiled layout of wide rows): one sweep per query
    int nb = std::min((nq + 15) / 16, std::min(ix->mq_blocks_max, bf16 ? 6 : 3));
    auto fits = [&](int n) {  // the image (+ tables, hit buffers, staging) must fit LDS
        if (bf16) return szg::mq_bf16_lds_bytes(ix->bits, ix->map.r16, n) <= 160u * 1024u;
        return szg::mq_i8_lds_bytes(ix->bits, ix->map.r16, n) <= 150u * 1024u;
    };
    while (nb > 0 && !fits(nb)) nb--;
    return nb;
}

}  // namespace szgi

// host-only test hook: key_bound.h's answer, no handle and no device (family: 0 the one-sweep kernel, 1 the int8 shared
// sweep, 2 the bfloat16 shared sweep, 3 the plain float32 shared sweep)
int szg_debug_key_eps(int dim, int quant_bits, int metric, int planes, int mq_planes, int family, double key, double qnorm,
                      double qnorm2, double qscale, double mq_qscale, double *eps)
{
    using szgi::fail;
    if (!eps) return fail(SZG_E_INVALID, "null argument");
    if (dim <= 0 || dim > (1 << 20)) return fail(SZG_E_INVALID, "dim out of range");
    if (szgi::row_bytes_of(quant_bits, dim) < 0) return fail(SZG_E_INVALID, "unsupported quantization");
    if (metric != SZG_COSINE && metric != SZG_EUCLIDEAN) return fail(SZG_E_INVALID, "unknown metric");
    if (planes != 2 && planes != 3) return fail(SZG_E_INVALID, "planes is 2 or 3");
    if (mq_planes != 0 && mq_planes != 2 && mq_planes != 3) return fail(SZG_E_INVALID, "mq_planes is 0 (the build's), 2 or 3");
    if (family < 0 || family > 3) return fail(SZG_E_INVALID, "family is 0 (one sweep), 1 (int8), 2 (bfloat16) or 3 (float32)");
    if (family == 1 && quant_bits > 8) return fail(SZG_E_INVALID, "the int8 shared sweep serves 8- and 4-bit rows");
    szg::KeyBoundIn b;
    b.dim = dim;
    b.bits = quant_bits;
    b.cosine = metric == SZG_COSINE ? 1 : 0;
    b.planes = planes;
    b.mq_planes = mq_planes ? mq_planes : szg::kMqPlanes;
    b.mq = family >= 2;
    b.mq_bf16 = family == 2;
    b.mq_int = family == 1;
    b.qnorm = qnorm;
    b.qnorm2 = qnorm2;
    b.qscale = qscale;
    b.mq_qscale = mq_qscale;
    *eps = szg::key_bound(b, key);
    return SZG_OK;
}
