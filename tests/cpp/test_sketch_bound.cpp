// The arithmetic of the sketch certificates (syzgydb_amd/csrc/sketch_bound.h) on its own: plain g++, no HIP, no library --
// built with -fsanitize=address,undefined by tests/test_sketch_bound_cpu.py.
//
//   test_sketch_bound            (no arguments: the inputs are fixed here, and printed)
// prints every input and result as the doubles' bit patterns (hex), one call per line:
//   slack <max_ang> <gs> <dim, decimal> <result>
//   below <gs> <key> <result>          above <gs> <key> <result>
//   settles <kth> <D_lb> <slack> <0|1>
//   radius <R> <slack> <D>             keyradius <gs> <D> <result>          rhanded <gs> <D> <0|1>
//   query <name> <element> ...         qhanded <name> <gs> <0|1>            scaled <name> <gs> <element> ...
// The Python side restates the rules and compares bit for bit.  What it cannot do in float64 is asserted here, against a
// long double reference of the real formulas -- cosine: acos(-key) / pi, Euclid: gs sqrt(max(key, 0)) / 255 --: at every
// finite key  below <= exact <= above,  neither falls as the key grows, both lie within what their own constants allow,
// and an overflowing gs sqrt(key) yields a non-finite value that settles nothing and gives no radius.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../syzgydb_amd/csrc/sketch_bound.h"

using namespace szgi;

static uint64_t bits_of(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

static int failures = 0;
#define CHECK(cond, ...)                \
    do {                                \
        if (!(cond)) {                  \
            printf("FAIL " __VA_ARGS__); \
            printf("\n");               \
            failures++;                 \
        }                               \
    } while (0)

// the real formulas (a key bound beyond what a cosine can be stands for the nearest one that can)
static long double exact_dist(double gs, double key)
{
    const long double pi = 3.14159265358979323846264338327950288L;
    if (gs > 0.0) return (long double)gs * sqrtl(key > 0.0 ? (long double)key : 0.0L) / 255.0L;
    const long double c = -(long double)key;
    return acosl(c > 1.0L ? 1.0L : (c < -1.0L ? -1.0L : c)) / pi;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ascending, NaN last
    const double keys[] = {-2.0, -1.0 - 1e-15, -1.0, -1.0 + 1e-16, -0.5, -1e-300, -0.0, 0.0, 1e-300, 0.5, 1.0 - 1e-16,
                           1.0,  1.0 + 1e-15,  2.0,  3e38,         inf,  nan};
    const double scales[] = {0.0, 3.7, 1e-150, 1e200};  // 0: cosine
    const int n_keys = (int)(sizeof(keys) / sizeof(keys[0]));

    for (int dim : {1, 222, 223, 768, 4096})
        for (double gs : {0.0, 3.7})
            for (double ang : {0.0, 1e-3, 0.01234, 0.5})
                printf("slack %016" PRIx64 " %016" PRIx64 " %d %016" PRIx64 "\n", bits_of(ang), bits_of(gs), dim,
                       bits_of(sketch_slack(ang, gs, dim)));

    for (double gs : scales) {
        double last_b = -inf, last_a = -inf;
        for (int i = 0; i < n_keys; i++) {
            const double key = keys[i];
            const double b = sketch_dist_below(gs, key), a = sketch_dist_above(gs, key);
            printf("below %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(gs), bits_of(key), bits_of(b));
            printf("above %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(gs), bits_of(key), bits_of(a));
            if (std::isnan(key)) {
                CHECK(std::isnan(b) && std::isnan(a), "gs %g: a NaN key must give NaN, not a bound", gs);
                CHECK(!sketch_settles(0.0, b, 0.0) && sketch_radius_handed(gs, sketch_collect_radius(a, 0.0)), "gs %g: NaN bound used", gs);
                continue;
            }
            CHECK(b >= last_b && a >= last_a, "gs %g key %a: a bound falls as the key grows", gs, key);
            last_b = b, last_a = a;
            if (!std::isfinite(key)) continue;
            const long double x = exact_dist(gs, key);
            CHECK((long double)b <= x && x <= (long double)a, "gs %g key %a: below %a exact %La above %a", gs, key, b, x, a);
            if (gs > 0.0) {  // relative: (1 -+ 1e-9) and three roundings
                CHECK(fabsl((long double)b - x) <= 2e-9L * x && fabsl((long double)a - x) <= 2e-9L * x,
                      "gs %g key %a: beyond 2e-9 of %La: below %a above %a", gs, key, x, b, a);
            } else {  // absolute: 1e-15 on the cosine is at most sqrt(2 * 1e-15) / pi on the angle, + the relative 1e-12
                CHECK(fabsl((long double)b - x) <= 2e-8L && fabsl((long double)a - x) <= 2e-8L,
                      "cosine key %a: beyond 2e-8 of %La: below %a above %a", key, x, b, a);
            }
        }
    }
    // gs sqrt(key) beyond the doubles: not a bound.  It settles nothing and gives no radius
    {
        const double gs = 1e200, key = 1e300;
        const double b = sketch_dist_below(gs, key), a = sketch_dist_above(gs, key);
        printf("below %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(gs), bits_of(key), bits_of(b));
        printf("above %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(gs), bits_of(key), bits_of(a));
        CHECK(!std::isfinite(b) && !std::isfinite(a), "an overflowing gs sqrt(key) gave a finite bound");
        CHECK(!sketch_settles(0.0, b, 0.0), "an infinite D_lb settled a query");
        CHECK(sketch_radius_handed(gs, sketch_collect_radius(a + 0.25, 0.25)), "an infinite D_s gave a radius");
    }

    const double ds[] = {-inf, -1.0, 0.0, 0.25, 0.5, 1.0 - 1e-16, 1.0, 1.5, 1e308, inf, nan};
    for (double kth : {0.0, 0.25, 0.5, inf, nan})
        for (double D : ds)
            for (double slack : {0.0, 1e-3, 0.25})
                printf("settles %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d\n", bits_of(kth), bits_of(D), bits_of(slack),
                       sketch_settles(kth, D, slack) ? 1 : 0);
    for (double R : {0.0, 0.5, 1.0, 1e308, inf, -inf, nan})
        for (double slack : {0.0, 1e-3, 0.25}) {
            const double D = sketch_collect_radius(R, slack);
            printf("radius %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(R), bits_of(slack), bits_of(D));
            CHECK(std::isnan(R) || D >= R + slack, "the collect radius of %a, slack %a is below their sum", R, slack);
            for (double gs : scales)
                printf("rhanded %016" PRIx64 " %016" PRIx64 " %d\n", bits_of(gs), bits_of(D), sketch_radius_handed(gs, D) ? 1 : 0);
        }
    for (double gs : scales)
        for (double D : ds) {
            printf("keyradius %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(gs), bits_of(D), bits_of(sketch_key_radius(gs, D)));
            printf("rhanded %016" PRIx64 " %016" PRIx64 " %d\n", bits_of(gs), bits_of(D), sketch_radius_handed(gs, D) ? 1 : 0);
        }

    // queries: a vector of exactly dim doubles on the heap each (a read beyond it is the sanitizer's to find)
    const int dim = 7;
    struct Named {
        const char *name;
        std::vector<double> q;
    };
    std::vector<Named> qs;
    auto base = [&] {
        std::vector<double> q(dim);
        for (int i = 0; i < dim; i++) q[i] = (i % 2 ? -1.0 : 1.0) * (0.5 + i) / 3.0;
        return q;
    };
    auto with = [&](const char *name, int at, double v) {
        Named x{name, base()};
        x.q[at] = v;
        qs.push_back(x);
    };
    qs.push_back(Named{"plain", base()});
    with("nan_first", 0, nan);
    with("nan_last", dim - 1, nan);
    with("inf_first", 0, inf);
    with("inf_last", dim - 1, -inf);
    qs.push_back(Named{"zero", std::vector<double>(dim, 0.0)});
    qs.push_back(Named{"negative_zero", std::vector<double>(dim, -0.0)});
    qs.push_back(Named{"squares_overflow", std::vector<double>(dim, 1e200)});
    with("one_square_overflows", dim - 1, -1.5e154);
    qs.push_back(Named{"squares_underflow", std::vector<double>(dim, 1e-200)});  // (a zero sum of a query with a direction)
    for (const Named &x : qs)
        for (double gs : scales) {
            printf("qhanded %s %016" PRIx64 " %d\n", x.name, bits_of(gs), sketch_query_handed(x.q.data(), dim, gs) ? 1 : 0);
            std::vector<double> out(dim, 12345.0);
            sketch_scale_query(x.q.data(), dim, gs, out.data());
            printf("scaled %s %016" PRIx64, x.name, bits_of(gs));
            for (int i = 0; i < dim; i++) printf(" %016" PRIx64, bits_of(out[i]));
            printf("\n");
        }
    for (const Named &x : qs) {
        printf("query %s", x.name);
        for (int i = 0; i < dim; i++) printf(" %016" PRIx64, bits_of(x.q[i]));
        printf("\n");
    }
    if (failures) return 1;
    printf("sketch bound ok\n");
    return 0;
}
