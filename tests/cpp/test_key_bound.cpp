// Stand-alone check of the certification bound on float rows under Euclid (syzgydb_amd/csrc/key_bound.h: key_bound).
// Plain C++, no HIP, its own main; tests/test_coincident_cpu.py builds it with -fsanitize=address,undefined and runs it.
// The one-sweep kernel's float32 key (RowAcc<32> and RowAcc<16> in kernels_scan.hip) is emulated: the prepared query
// g = q (32-bit rows) or 65535 q (16-bit rows, whose elements are the odd integers n = 2 v - 65535) is narrowed to
// float32, the squared float32 differences are summed by fmaf -- in one chain, and in 8 lanes reduced by a tree, the two
// ends of what a lane map does -- and the result is compared with the long double key |g - x|^2 of the UNROUNDED query:
//     |key - real| <= key_bound(key) + the reference's own rounding
// for queries at and near a stored row: P0 the row itself, P1 the row moved by at most a quarter of the float32 spacing
// at each prepared element (the query rounds to the row: key 0, real key > 0), P2 the row moved by 1, 3 and 17 spacings
// in 1, 7 and all coordinates, and an ordinary query; dimensions 1, 3, 17 and 768; magnitudes 1e-3, 1 and 1e3, and 1e-20
// and 1e-24, where the squares fall into and below the float32 subnormals.
// The formula as it stood before it had a term for the narrowing of the query (old_bound below) must FAIL on P1 cases:
// that is counted and required, so the program cannot pass by standing beside the gap.
// Last, it prints the bound of a few fixed inputs of every family as hexadecimal floats ("BOUND ..." lines): the pytest
// asks szg_debug_key_eps the same and compares bit for bit, so the library's hook and this header cannot drift apart.
#include "../../syzgydb_amd/csrc/key_bound.h"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

using namespace szg;

static int g_failures = 0;
static long g_checked = 0, g_zero_keys = 0, g_old_fails = 0, g_old_fails_p1 = 0;

// the float-row Euclidean formula without the 4 u^2 |g|^2 term
static double old_bound(int dim, double key, double qnorm)
{
    const double u = 0x1p-24, n = (double)dim + 16.0, k = std::fabs(key);
    return 2.0 * n * u * k + 8.0 * u * qnorm * std::sqrt(k) + 1e-37;
}

static float key_chain(const std::vector<float> &g, const std::vector<float> &x)
{
    float a = 0.0f;
    for (size_t i = 0; i < g.size(); i++) {
        const float d = g[i] - x[i];
        a = std::fmaf(d, d, a);
    }
    return a;
}

static float key_lanes(const std::vector<float> &g, const std::vector<float> &x)
{
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t i = 0; i < g.size(); i++) {
        const float d = g[i] - x[i];
        a[i % 8] = std::fmaf(d, d, a[i % 8]);
    }
    for (int w = 4; w >= 1; w /= 2)
        for (int l = 0; l < w; l++) a[l] = a[l] + a[l + w];
    return a[0];
}

// q: the caller's query; x: the row's elements in the key's units (float32 values, or the integers n); scale: q -> g
static void check_pair(int bits, const std::vector<double> &q, const std::vector<float> &x, double scale, bool p1, const char *what)
{
    const int dim = (int)q.size();
    std::vector<float> gf(dim);
    double qnorm2 = 0.0;
    long double real = 0.0L;
    for (int i = 0; i < dim; i++) {
        const double g = q[i] * scale;
        qnorm2 += g * g;
        gf[i] = (float)g;
        const long double d = (long double)q[i] * (long double)scale - (long double)x[i];
        real += d * d;
    }
    KeyBoundIn b;
    b.dim = dim;
    b.bits = bits;
    b.qnorm = std::sqrt(qnorm2);
    b.qnorm2 = qnorm2;
    const long double ref_err = (long double)(dim + 8) * LDBL_EPSILON * real;
    const float keys[2] = {key_chain(gf, x), key_lanes(gf, x)};
    for (float key : keys) {
        const long double off = fabsl((long double)key - real);
        const double eps = key_bound(b, (double)key);
        g_checked++;
        if (key == 0.0f && real > 0.0L) g_zero_keys++;
        if (!(off <= (long double)eps + ref_err)) {
            std::fprintf(stderr, "%s: %d-bit dim %d: key %a real %La off %La bound %a\n", what, bits, dim, (double)key, real, off, eps);
            g_failures++;
        }
        if (off > (long double)old_bound(dim, (double)key, b.qnorm) + ref_err) {
            g_old_fails++;
            if (p1) g_old_fails_p1++;
        }
    }
}

static double spacing(float f)  // the float32 spacing at f (the subnormal spacing at and below the smallest normal)
{
    const float a = std::fabs(f);
    return (double)std::nextafterf(a, INFINITY) - (double)a;
}

static void near_row_cases(int bits, const std::vector<float> &x, const std::vector<double> &stored, double scale, std::mt19937_64 &rng)
{
    // stored: the query that decodes to the row (q_i with scale * q_i == x_i up to float64 rounding)
    const int dim = (int)x.size();
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    check_pair(bits, stored, x, scale, false, "P0");
    for (int rep = 0; rep < 4; rep++) {  // P1: |d_i| <= spacing / 4, at the edge of it and inside
        std::vector<double> q(stored);
        for (int i = 0; i < dim; i++) {
            const double s = spacing(x[i]) / scale / 4.0;
            q[i] += rep == 0 ? s : rep == 1 ? -s : unit(rng) * s;
        }
        check_pair(bits, q, x, scale, true, "P1");
    }
    const int moves[] = {1, 3, 17};
    const int coords[] = {1, 7, dim};
    for (int m : moves)
        for (int c : coords) {
            std::vector<double> q(stored);
            for (int j = 0; j < c && j < dim; j++) {
                const int i = (int)(((long)j * 131) % dim);
                q[i] += (j % 2 ? -1.0 : 1.0) * m * spacing(x[i]) / scale;
            }
            check_pair(bits, q, x, scale, false, "P2");
            for (int i = 0; i < dim; i++) q[i] += unit(rng) * spacing(x[i]) / scale / 4.0;  // ... and off the lattice
            check_pair(bits, q, x, scale, false, "P2 off the lattice");
        }
}

static void print_bound(int dim, int bits, int metric, int planes, int family, double key, double qnorm, double qnorm2, double qscale,
                        double mq_qscale)
{
    KeyBoundIn b;
    b.dim = dim;
    b.bits = bits;
    b.cosine = metric;
    b.planes = planes;
    b.mq_planes = family == 1 && bits == 4 ? 3 : 2;  // (both plane counts of the int8 sweep: the hook takes the count)
    b.mq = family >= 2;
    b.mq_bf16 = family == 2;
    b.mq_int = family == 1;
    b.qnorm = qnorm;
    b.qnorm2 = qnorm2;
    b.qscale = qscale;
    b.mq_qscale = mq_qscale;
    std::printf("BOUND %d %d %d %d %d %d %a %a %a %a %a -> %a\n", dim, bits, metric, planes, b.mq_planes, family, key, qnorm, qnorm2, qscale, mq_qscale,
                key_bound(b, key));
}

int main()
{
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    const int dims[] = {1, 3, 17, 768};
    const double mags[] = {1e-3, 1.0, 1e3, 1e-20, 1e-24};
    for (int dim : dims) {
        for (double mag : mags) {  // 32-bit rows: any float32 value
            for (int rep = 0; rep < 3; rep++) {
                std::vector<float> x(dim);
                std::vector<double> stored(dim), other(dim);
                for (int i = 0; i < dim; i++) {
                    x[i] = (float)(unit(rng) * mag + (rep == 2 ? mag * 1000.0 : 0.0));  // (rep 2: far from the origin)
                    stored[i] = (double)x[i];
                    other[i] = unit(rng) * mag + (rep == 2 ? mag * 1000.0 : 0.0);
                }
                near_row_cases(32, x, stored, 1.0, rng);
                check_pair(32, other, x, 1.0, false, "ordinary query");
            }
        }
        for (int rep = 0; rep < 6; rep++) {  // 16-bit rows: n = 2 v - 65535; rep 4 and 5 sit at the ends of the code range
            std::vector<float> x(dim);
            std::vector<double> stored(dim), other(dim);
            for (int i = 0; i < dim; i++) {
                uint32_t v = (uint32_t)(rng() % 65536u);
                if (rep == 4) v = (uint32_t)(rng() % 3u);
                if (rep == 5) v = 65535u - (uint32_t)(rng() % 3u);
                x[i] = (float)(2.0 * v - 65535.0);
                stored[i] = (double)v / 65535.0 * 2.0 - 1.0;  // the reference's decode
                other[i] = unit(rng);
            }
            near_row_cases(16, x, stored, 65535.0, rng);
            check_pair(16, other, x, 65535.0, false, "ordinary query");
        }
    }
    std::printf("checked %ld keys, %ld of them 0 over a positive real key; the formula without the query term fails %ld (%ld under P1)\n",
                g_checked, g_zero_keys, g_old_fails, g_old_fails_p1);
    if (g_zero_keys == 0 || g_old_fails_p1 == 0) {
        std::fprintf(stderr, "no case stands on the gap: P1 gave no zero key over a positive real key that the old formula misses\n");
        g_failures++;
    }
    // 64-bit rows keep the query in float64: the bound at key 0 covers a float64 sum that vanished in the narrowing
    {
        KeyBoundIn b;
        b.dim = 768;
        b.bits = 64;
        b.qnorm = 1e3;
        b.qnorm2 = 1e6;
        if (!(key_bound(b, 0.0) >= 0x1p-149)) {
            std::fprintf(stderr, "64-bit rows: the bound at key 0 is below the smallest float32\n");
            g_failures++;
        }
    }
    // the bound never shrinks as the key grows, and is positive at 0, in every family
    for (int family = 0; family < 4; family++)
        for (int bits : {4, 8, 16, 32, 64})
            for (int metric = 0; metric < 2; metric++) {
                if (family == 1 && bits > 8) continue;  // (the int8 sweep serves 8- and 4-bit rows)
                KeyBoundIn b;
                b.dim = 100;
                b.bits = bits;
                b.cosine = metric;
                b.mq = family >= 2;
                b.mq_bf16 = family == 2;
                b.mq_int = family == 1;
                b.qnorm = metric ? 1.0 : 7.0;
                b.qnorm2 = b.qnorm * b.qnorm;
                b.qscale = b.mq_qscale = 1e-4;
                double last = 0.0;
                for (double key : {0.0, 1e-30, 1e-12, 1e-3, 1.0, 1e4}) {
                    const double e = key_bound(b, key);
                    if (!(e > 0.0) || !(e >= last)) {
                        std::fprintf(stderr, "family %d bits %d metric %d key %g: bound %g after %g\n", family, bits, metric, key, e, last);
                        g_failures++;
                    }
                    last = e;
                }
            }
    // what the pytest compares with the library's hook
    for (double key : {0.0, 0x1p-100, 2.5, 1e6}) {
        print_bound(768, 32, 0, 3, 0, key, 27.7, 27.7 * 27.7, 0.0, 0.0);
        print_bound(17, 16, 0, 3, 0, key, 1.5e5, 2.25e10, 0.0, 0.0);
        print_bound(24, 64, 0, 3, 0, key, 1e3, 1e6, 0.0, 0.0);
        print_bound(100, 8, 0, 3, 0, key, 2e3, 4e6, 2.5e-4, 0.0);
        print_bound(100, 8, 0, 2, 0, key, 2e3, 4e6, 1.5e-2, 0.0);
        print_bound(200, 4, 0, 3, 0, key, 150.0, 22500.0, 5e-4, 0.0);
        print_bound(192, 8, 0, 3, 1, key, 2e3, 4e6, 2.5e-4, 1.5e-2);
        print_bound(40, 32, 0, 3, 2, key, 6.0, 36.0, 0.0, 0.0);
        print_bound(24, 64, 0, 3, 2, key, 6.0, 36.0, 0.0, 0.0);
        print_bound(40, 32, 0, 3, 3, key, 6.0, 36.0, 0.0, 0.0);
    }
    for (double key : {-1.0, -0.25, 0.5}) {
        print_bound(768, 32, 1, 3, 0, key, 1.0, 1.0, 0.0, 0.0);
        print_bound(24, 64, 1, 3, 0, key, 1.0, 1.0, 0.0, 0.0);
        print_bound(100, 8, 1, 3, 0, key, 1.0, 1.0, 1e-6, 0.0);
        print_bound(200, 4, 1, 3, 1, key, 1.0, 1.0, 1e-6, 6e-5);
        print_bound(17, 16, 1, 3, 2, key, 1.0, 1.0, 0.0, 0.0);
        print_bound(17, 32, 1, 3, 3, key, 1.0, 1.0, 0.0, 0.0);
    }
    if (g_failures) {
        std::fprintf(stderr, "%d failure(s)\n", g_failures);
        return 1;
    }
    std::puts("key bound ok");
    return 0;
}
