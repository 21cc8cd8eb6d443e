// query_prep.h -- the rule by which a query becomes the 8-bit one-sweep kernels' image and constants, stated once: the
// host form (prep_query's 8-bit branch, scan_query.cpp) and the kernel that prepares a sketch batch on the card (option
// query_prep; kernels_query_prep.hip) both compute from here, so that nothing downstream -- the sweeps, key_eps, the
// certificates -- can tell which side prepared a query: same bytes, same constants, bit for bit.  Plain C++, no HIP
// runtime and no handle types, usable from host and device code: tests/cpp/test_query_prep.cpp compiles it on its own
// under the address and undefined-behaviour sanitizers.
//
// A query q of `dim` float64 elements (for a Euclidean sketch already divided by the collection's scale) becomes
//   m1      sum q_e^2, added in element order
//   scale   cosine: 1 / sqrt(m1), or 0 where m1 is not above 0; Euclid: 2^bits - 1 on rows of up to 16 bits, else 1
//   v_e     q_e * scale                                    (the prepared query)
//   qnorm2  sum v_e^2, added in element order; qnorm = sqrt(qnorm2)
//   vmax    max |v_e| by std::max's rule: a NaN element never becomes the maximum
//   qs      vmax / Qmax where vmax is above 0 and finite, else 1      (Qmax: qp_qmax8, by the digit planes)
//   Q_e     round_clamp(q_e * scale / qs, Qmax): that expression's order, ties away from zero, NaN -> 0
//   qconst  sum Q_e (integers below 2^53: exact in any order)
// (a constant that comes out a NaN is stored as the one quiet NaN of qp_canon)
// and Q_e is split into balanced digits of radix 128, the low one first: ((Q + 64) & 127) - 64, the rest (Q - digit) >> 7;
// the image's top plane (plane 3 - planes) takes what is left.  Plane 0 is the h plane (x 16384), 1 the m plane (x 128),
// 2 the l plane; a two-plane image leaves plane 0 all zero.  Element e's digit of plane x is byte (e % 16) % 4 of the
// 32-bit word (x * r16 + e / 16) * 4 + (e % 16) / 4 of the image, r16 the row's 16-byte pieces; the image is 3 * r16 * 16
// bytes whatever the plane count, and every byte that no element reaches is zero.
//
// The two sums in element order are what makes the card's constants the host's: the kernel adds them on one lane, left to
// right, with explicit multiplications and additions (its unit is compiled without contraction, as this header's host
// callers are: x86-64 code without FMA).
//
// NOT covered here, and prepared on the host as before: the 4-bit and float forms of prep_query, the shared sweeps'
// images (prep_mq_int and the bfloat16 images), and with them every pipeline but the sketch top-k call's -- the radius
// pipelines and the large-k collect pipeline need the constants on the host before their sweeps, the full-precision
// fall-back prepares float forms.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SZG_QP_HD __host__ __device__ inline
#else
#define SZG_QP_HD inline
#endif

namespace szg {

// the constants of a prepared query in the order the kernel writes them (d_meta: kQueryPrepMeta doubles per query)
constexpr int kQueryPrepMeta = 5;
enum QueryPrepSlot { kQpQnorm = 0, kQpM1 = 1, kQpQscale = 2, kQpQconst = 3, kQpQnorm2 = 4 };

struct QueryPrepConsts {
    double qnorm, m1, qscale, qconst, qnorm2;
};

// |Q| <= this with `planes` int8 digit planes (key_bound.h's plane_qmax: the bound reads the same numbers)
SZG_QP_HD double qp_qmax8(int planes) { return planes == 2 ? 16000.0 : 1000000.0; }

// the scale q -> prepared query
SZG_QP_HD double qp_scale(int cosine, int bits, double m1)
{
    if (cosine) return m1 > 0 ? 1.0 / sqrt(m1) : 0.0;
    return bits <= 16 ? (double)((1u << bits) - 1u) : 1.0;
}

// A constant that is a NaN (m1, qnorm2, qnorm of a query with a NaN element, or with an infinite one under cosine,
// where inf * 0 makes one) is stored as THE quiet NaN 0x7FF8000000000000: processors and compilers differ in the sign
// and payload of a NaN they make or pass on (an x86 makes the negative one, constant folding and other processors the
// positive one), nothing downstream reads either -- such a query never settles through the sketch -- and "the same
// constants on every side" then holds for these bytes too.  The arithmetic before this last step sees the NaN as it came.
SZG_QP_HD double qp_canon(double x)
{
    if (x == x) return x;
    const uint64_t quiet = 0x7FF8000000000000ull;
    double r;
    memcpy(&r, &quiet, sizeof(r));
    return r;
}

// std::max(vmax, f) as the host has always taken it: f replaces vmax only where vmax < f, so a NaN never enters.  The
// maximum of a set by this rule does not depend on the order (NaNs are skipped, the rest is totally ordered).
SZG_QP_HD double qp_max(double vmax, double f) { return vmax < f ? f : vmax; }

// the quantisation step
SZG_QP_HD double qp_step(double vmax, double Qmax)
{
    return (vmax > 0 && vmax <= 1.7976931348623157e308) ? vmax / Qmax : 1.0;  // (above 0 and finite)
}

// round to nearest (ties away from zero) without a libm call; NaN -> 0, clamped to +-lim.
// Any rounding rule serves: Q only has to be within 1/2 of v/qscale (key_eps).
SZG_QP_HD long long qp_round_clamp(double t, double lim)
{
    if (!(t == t)) return 0;
    if (t > lim) t = lim;
    if (t < -lim) t = -lim;
    return (long long)(t + (t >= 0 ? 0.5 : -0.5));
}

SZG_QP_HD long long qp_quantize(double q, double scale, double qs, double Qmax)
{
    const double v = q * scale;  // (a value of its own: never one fused operation with the division)
    return qp_round_clamp(v / qs, Qmax);
}

// The digit of Q that plane x of an image with `planes` planes carries (x in 3 - planes .. 2): the balanced digits from
// the low end, and all that is left in the top plane.  As a byte: (uint8_t)(int8_t)digit.
SZG_QP_HD long long qp_digit(long long Q, int x, int planes)
{
    const int top = 3 - planes;
    for (int p = 2; p > x; p--) {
        const long long dig = ((Q + 64) & 127) - 64;
        Q = (Q - dig) >> 7;
    }
    return x > top ? ((Q + 64) & 127) - 64 : Q;
}

// where element e's digit of plane x lies: the 32-bit word of the image, and the byte in it
SZG_QP_HD size_t qp_word(int x, int r16, int e) { return ((size_t)x * r16 + e / 16) * 4 + (e % 16) / 4; }
SZG_QP_HD int qp_byte(int e) { return (e % 16) % 4; }
SZG_QP_HD size_t qp_image_bytes(int r16) { return (size_t)r16 * 16 * 3; }

// ---- the host form ---------------------------------------------------------------------------------------------------

// m1, the scale, qnorm2 and vmax of a query (every row width: prep_query_norms)
inline void qp_norms(const double *q, int dim, int cosine, int bits, double *m1_out, double *scale_out, double *qnorm2_out,
                     double *vmax_out)
{
    double m1 = 0.0;
    for (int i = 0; i < dim; i++) m1 += q[i] * q[i];
    const double scale = qp_scale(cosine, bits, m1);
    double nrm = 0.0, vmax = 0.0;
    for (int e = 0; e < dim; e++) {
        const double v = q[e] * scale;
        nrm += v * v;
        vmax = qp_max(vmax, fabs(v));
    }
    *m1_out = qp_canon(m1);
    *scale_out = scale;
    *qnorm2_out = qp_canon(nrm);
    *vmax_out = vmax;
}

// the digit planes of a query whose scale and step are known: the image (qp_image_bytes(r16) bytes, zeroed here), and
// the digit sum
inline double qp_image8(const double *q, int dim, double scale, double qs, int planes, int r16, uint8_t *image)
{
    const double Qmax = qp_qmax8(planes);
    memset(image, 0, qp_image_bytes(r16));
    long long sumQ = 0;
    for (int e = 0; e < dim; e++) {
        const long long Q = qp_quantize(q[e], scale, qs, Qmax);
        sumQ += Q;
        for (int x = 2; x >= 3 - planes; x--)
            image[qp_word(x, r16, e) * 4 + qp_byte(e)] = (uint8_t)(int8_t)qp_digit(Q, x, planes);
    }
    return (double)sumQ;
}

// a whole query of an 8-bit index: image and constants
inline void query_prep8(const double *q, int dim, int cosine, int planes, int r16, uint8_t *image, QueryPrepConsts *c)
{
    double scale, vmax;
    qp_norms(q, dim, cosine, 8, &c->m1, &scale, &c->qnorm2, &vmax);
    c->qnorm = qp_canon(sqrt(c->qnorm2));
    c->qscale = qp_step(vmax, qp_qmax8(planes));
    c->qconst = qp_image8(q, dim, scale, c->qscale, planes, r16, image);
}

}  // namespace szg
