// key_bound.h -- the bound on |scan key - real-number key| of every sweep's arithmetic (DESIGN.md "certification").
// Plain C++, no HIP runtime and no handle: key_eps (scan_query.cpp) fills a KeyBoundIn from the handle and the query's
// QMeta, the host-only hook szg_debug_key_eps and tests/cpp/test_key_bound.cpp read the same function.
#pragma once
#include <cmath>

#include "scan_plan.h"

namespace szg {

struct KeyBoundIn {
    int dim = 0, bits = 0;
    int cosine = 0;     // the collection's metric: 1 cosine, 0 Euclid
    int planes = 3;     // digit planes of the one-sweep 8-bit query (scan_planes: 2 on a sketch index, else 3)
    int mq_planes = 2;  // digit planes of the int8 shared sweep (kMqPlanes)
    // which arithmetic gave the key (QMeta): a shared float32 sweep, its bfloat16 form, the int8 shared sweep; none: the
    // one-sweep kernel
    bool mq = false, mq_bf16 = false, mq_int = false;
    double qnorm = 0, qnorm2 = 0;      // |g| and |g|^2 of the prepared query g, in the key's units
    double qscale = 0, mq_qscale = 0;  // quantization step of the one-sweep integer query / of the int8 shared sweep's
};

inline double plane_qmax(int planes) { return planes == 2 ? 16000.0 : 1000000.0; }

inline double key_bound(const KeyBoundIn &b, double key)
{
    const double k = std::fabs(key);
    const double dim = (double)b.dim;
    if (b.mq) {
        // shared sweep: float32 everywhere (quantized rows decode to exact integers first).
        // cosine: dot and norm each carry <= (dim+16) u relative error.  euclid: the key is
        // |x|^2 - 2 x.g + |g|^2, three float32 sums whose magnitudes are bounded by
        // (|x| + |g|)^2 <= (2|g| + sqrt(key))^2 -- an absolute bound, far looser than the
        // difference form's when rows sit far from the origin; certification then simply
        // escalates more often.
        // (64-bit rows are narrowed to float32 element by element first: one more rounding of 2^-24 per operand,
        // i.e. u |x||g| on the dot product and 2u |x|^2 on the norm -- four more units of n cover both)
        const double u = 0x1p-24, n = dim + 16.0 + (b.bits == 64 ? 4.0 : 0.0);
        if (b.mq_bf16) {
            // bfloat16 sweep: each operand is rounded to 8 significant bits -- a bfloat16 keeps 7 fraction bits, so the
            // spacing at 1 is 2^-7 and round-to-nearest moves a value by at most 2^-8 of itself (the query once more
            // from float32) -- the products are exact in float32 and summed by the matrix core in float32.
            // |sum bf(x_i) bf(g_i) - sum x_i g_i| <= c |x| |g| (Cauchy-Schwarz) with
            // c = (1 + 2^-8)^2 (1 + 2^-24) - 1 < 1.01 * 2^-7; the float32 part of the bound is doubled (the
            // accumulation order and rounding of the matrix core are its own).  (Rounds 2-3 had 2^-9 per operand
            // here, i.e. half this band: a 2-dimensional corpus far from the origin, where both elements can round
            // the same way, showed a key 0.0044 off -- scripts/fuzz_gpu.py seed 311.  At >= 16 dimensions the
            // errors never lined up, which is why nothing had caught it.)
            const double c = 1.01 * 0x1p-7;
            if (b.cosine) return c + 4.0 * n * u + 1e-6;
            // euclid: the key moves by 2 c |x| |g|, and |x| <= |g| + d with d^2 <= key + 2 c |x| |g|
            // gives |x| <= 1.1 |g| + sqrt(key) for this c; the last term keeps key - eps(key) monotone
            const double s = 2.0 * b.qnorm + std::sqrt(k);
            return 2.0 * c * b.qnorm * (1.1 * b.qnorm + std::sqrt(k)) + c * c * b.qnorm2 + 3.0 * n * u * s * s + 1e-30;
        }
        if (b.cosine) return 2.0 * n * u;
        const double s = 2.0 * b.qnorm + std::sqrt(k);
        return 1.5 * n * u * s * s + 1e-30;
    }
    if (b.mq_int) {
        // as the integer branch below with the sweep's own quantization step; the row operand is
        // v' = v - 128 (8-bit rows) or the nibble x in 0..15 (4-bit rows)
        const double M = (double)((1u << b.bits) - 1u);
        const double V = b.bits == 8 ? 128.0 : 16.0, Qmax = plane_qmax(b.mq_planes);
        const double fl = 16.0 * 0x1p-24 * b.mq_qscale * Qmax * V * dim;
        if (b.cosine) return 0.5 * b.mq_qscale * std::sqrt(dim) + fl / std::sqrt(dim) + 0x1p-21;
        return b.mq_qscale * M * dim + 2.0 * fl + 0x1p-21 * (k + b.qnorm2 + M * M * dim) + 1e-30;
    }
    if (b.bits == 8 || b.bits == 4) {
        // integer paths: the per-lane sums are exact.  What is left is (a) the query's
        // quantization, |v_i - qscale*Q_i| <= qscale/2, and (b) the float32 roundings of
        // the row finish: the plane combination and the reduction over the lanes act on
        // terms bounded by sum |Q_i||v'_i| <= Qmax*V*dim (V = 128 resp. 8), i.e. an
        // absolute error <= 16*2^-24 * qscale*Qmax*V*dim in units of sum v n.
        // Two planes on a sketch index (scan_planes; Qmax = 16000, qscale = vmax / 16000 the two-plane step): nothing
        // in (a) or (b) depends on the plane count but through qscale and Qmax.  (a) grows with the step -- cosine:
        // 0.5 qscale sqrt(dim), Euclid: qscale M dim, 62.5 times the three-plane terms.  (b) does not move: qscale*Qmax
        // = vmax whatever Qmax is, and the two-plane key fmaf(128, M, L) rounds once where the three-plane one rounds
        // twice, with |128 M + L| <= Qmax*V*(elements of the lane) as before.
        const double M = (double)((1u << b.bits) - 1u);
        const double V = b.bits == 8 ? 128.0 : 8.0;
        const double Qmax = b.bits == 8 ? plane_qmax(b.planes) : kQmax4;
        const double fl = 16.0 * 0x1p-24 * b.qscale * Qmax * V * dim;
        if (b.cosine)  // divided by |n| >= sqrt(dim) (every n is odd)
            return 0.5 * b.qscale * std::sqrt(dim) + fl / std::sqrt(dim) + 0x1p-21;
        return b.qscale * M * dim + 2.0 * fl + 0x1p-21 * (k + b.qnorm2 + M * M * dim) + 1e-30;
    }
    const double u = b.bits == 64 ? 0x1p-53 : 0x1p-24;
    const double n = dim + 16.0;
    if (b.cosine) return 2.0 * n * u + (b.bits == 64 ? 0x1p-22 : 0.0);
    // Euclid on float rows (RowAcc<16|32|64> in kernels_scan.hip): the key is  k^ = fl sum (fl(g_i) - x_i)^2,  the real-
    // number key  K = |g - x|^2.  Two steps.
    //  (1) The narrowing of the prepared query to the sweep's format, e_i = fl(g_i) - g_i with |e_i| <= u |g_i|, hence
    //      |e| <= u |g|:  K' = |fl(g) - x|^2 = K + 2 e.(g - x) + |e|^2,  so  |K' - K| <= 2 u |g| sqrt(K) + u^2 |g|^2.
    //  (2) The sweep's own roundings, all on non-negative terms: the difference (squared: twice), at most dim fmaf in a
    //      lane, six steps of the reduction over the lanes -- m <= dim + 8 on any path:  |k^ - K'| <= y K'  with
    //      y = (1 + u)^m - 1 <= m u / (1 - m u), and y / (1 - y) <= 2 n u, n = dim + 16, up to the largest dim (2^20).
    // In terms of k^, which is what the caller has:  K' <= k^ / (1 - y)  and  sqrt(K) <= sqrt(K') + |e|, so
    //      |k^ - K|  <=  y K' + 2 u |g| (sqrt(K') + u |g|) + u^2 |g|^2  <=  2 n u k^ + 2.1 u |g| sqrt(k^) + 3 u^2 |g|^2.
    // The first two terms are the formula's of old (with 8 for 2.1).  The third was missing: where the query rounds to
    // the row, k^ = 0 while K = |e|^2 is up to u^2 |g|^2 -- nothing was left of the bound but the constant.  It enters
    // as 4 u^2 |g|^2: 3 from the line above; the fourth unit is for the float64 roundings the derivation leaves out --
    // g_i = maxInt q_i is rounded once before it is narrowed (u becomes u (1 + 2^-29)) and qnorm2 is a float64 sum
    // (off by at most (dim + 2) 2^-53 of itself, 2^-32 at the largest dim) -- which need a 10^-8 of it.  At |g| = 1 the
    // term is 1.4e-14: where a key is of the size of |g|^2 it is seven orders below the spacing of the float32 key, and
    // no threshold at a key of ordinary size moves.
    // 64-bit rows: the query stays float64, u = 2^-53 in (1) (q_i - x_i rounds once); the key is narrowed to float32 on
    // the way out: 2^-24 k^ while it is a normal float32, at most 2^-150 absolute below 2^-126 -- k^ = 0 included, where
    // the float64 sum was below 2^-150 -- which the constant covers.
    // Underflow (float32 sums): subnormals are kept (the kernels are built without flush-to-zero), so an fmaf whose
    // result falls below 2^-126 is off by at most 2^-150 absolute, (dim + 16) 2^-150 < 2^-129 up to dim 2^20; a
    // subnormal fl(g_i) is off by 2^-150 instead of u |g_i|, which moves K' by at most 2^-149 sqrt(dim K) -- below
    // 2 n u K where K >= 2^-250 / dim, below 2^-274 elsewhere.  The constant 1e-37 > 2^-123 covers these.
    return 2.0 * n * u * k + 8.0 * u * b.qnorm * std::sqrt(k) + 4.0 * u * u * b.qnorm2 + (b.bits == 64 ? 0x1p-22 * k : 0.0) +
           1e-37;
}

}  // namespace szg
