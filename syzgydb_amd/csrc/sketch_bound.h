// sketch_bound.h -- the arithmetic every certificate of a call through the 8-bit sketch rests on: slack, the two
// conversions between a bound on a sketch key and a sketch distance, the collect radius, and which queries and radii the
// sketch does not serve.  Plain C++, no HIP and no handle, header only: the three pipelines (SketchCall, scan_sketch.cpp;
// SketchRadiusCall, scan_radius.cpp; SketchTopkCall, scan_sketch_topk.cpp) read the same functions, and
// tests/cpp/test_sketch_bound.cpp holds them to the real formulas on their own.
#pragma once
#include <algorithm>
#include <cmath>

namespace szgi {

// slack: what the triangle inequality adds to or takes from a sketch distance -- the largest d(row, its sketch) that the
// build measured (max_ang), rounded up, + under cosine (gs = 0) the rounding of the build kernel's angles: its float64
// cosine of (row, sketch) is off by at most (dim + 8) u, which acos turns into at most sqrt(2 (dim + 8) u) where c is near
// 1 -- a row that its sketch all but reproduces.  Twice the root (a float64 reference beside it;
// cert_check.sketch_angle_rounding) passes 1e-7 from dim 104 on.
inline double sketch_slack(double max_ang, double gs, int dim)
{
    const double ang_round = gs > 0.0 ? 0.0 : std::max(1e-7, 2.0 * std::sqrt((dim + 8) * 0x1p-52) / M_PI);
    return max_ang * (1.0 + 1e-9) + ang_round;
}

// A bound on the real-number sketch key -> the sketch distance it implies.  Cosine (gs = 0): key = -cos,
// distance acos(cos) / pi; Euclid: key = (255 d)^2 in units of gs.  The key is monotone in the distance, and the two
// directions are mirror images that differ in which way every rounding is pushed:
//   below  a LOWER bound lb of the keys of the rows outside a top-k call's lists -> D_lb, at or below the sketch distance
//          of each of them.  It feeds a certificate (the answer's k-th distance is below D_lb - slack), so it rounds DOWN:
//          the cosine is bounded from above, the quotient scaled by 1 - 1e-12 (1 - 1e-9 under Euclid).
//   above  an UPPER bound U of the keys of k sampled rows -> D_s, at or above the sketch distance of each of them.  It
//          feeds a radius that must contain the answer, so it rounds UP: the cosine is bounded from below, the factors are
//          1 + 1e-12 and 1 + 1e-9.
// Float64 rows: at a scale near the largest double gs * sqrt(key) overflows.  An infinite result bounds nothing -- the
// product it stands for is finite -- so the callers take only a finite one: it settles no query and gives no radius.
inline double sketch_dist_below(double gs, double key_lb)
{
    if (gs > 0.0) return gs * std::sqrt(std::max(key_lb, 0.0)) / 255.0 * (1.0 - 1e-9);
    const double x = -key_lb + 1e-15;  // (an upper bound of the cosine, rounding included)
    return x >= 1.0 ? 0.0 : (x <= -1.0 ? 1.0 : std::acos(x) / M_PI * (1.0 - 1e-12));
}
inline double sketch_dist_above(double gs, double key_ub)
{
    if (gs > 0.0) return gs * std::sqrt(std::max(key_ub, 0.0)) / 255.0 * (1.0 + 1e-9);
    const double x = -key_ub - 1e-15;  // (a lower bound of the cosine, rounding included)
    return x >= 1.0 ? 0.0 : (x <= -1.0 ? 1.0 : std::acos(x) / M_PI * (1.0 + 1e-12));
}
// The certificate of the top-k pre-pass: every row outside the lists is at d(q, row) >= D_lb - slack (the triangle
// inequality), so an answer whose k-th distance kth is below that is final
inline bool sketch_settles(double kth, double D_lb, double slack)
{
    return std::isfinite(D_lb) && kth * (1.0 + 1e-9) < D_lb - slack;
}

// The sketch-distance radius D of a collect sweep that surely holds every row within R of the query:
// d(q, sketch) <= d(q, row) + d(row, sketch) <= R + max_ang <= D; what radius_key_threshold is asked with on the sketch
// handle (Euclid: in units of gs, as the sweep's queries); and the radii no sweep serves: a non-finite D, and under cosine
// a D that covers every angle.
inline double sketch_collect_radius(double R, double slack) { return R * (1.0 + 1e-9) + slack; }
inline double sketch_key_radius(double gs, double D) { return gs > 0.0 ? D / gs : D; }
inline bool sketch_radius_handed(double gs, double D) { return !std::isfinite(D) || (gs <= 0.0 && D >= 1.0); }

// A query the sketch does not serve: a non-finite element or sum of squares; under cosine a query without a direction
inline bool sketch_query_handed(const double *q, int dim, double gs)
{
    double m1 = 0.0;
    for (int i = 0; i < dim; i++) {
        if (!std::isfinite(q[i])) return true;
        m1 += q[i] * q[i];
    }
    return !std::isfinite(m1) || (gs <= 0.0 && m1 == 0.0);
}
// ... and the form the sketch sweeps see of one it serves: q / gs under Euclid
inline void sketch_scale_query(const double *q, int dim, double gs, double *out)
{
    for (int i = 0; i < dim; i++) out[i] = gs > 0.0 ? q[i] / gs : q[i];
}

}  // namespace szgi
