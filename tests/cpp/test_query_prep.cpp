// The 8-bit query rule (syzgydb_amd/csrc/query_prep.h) and the batch rule of option query_prep (sketch_plan.h) on their
// own: plain g++, no HIP, no library -- built with -fsanitize=address,undefined by tests/test_query_prep_cpu.py.
//
//   test_query_prep <file> <dim> <n> <cosine> <planes> <gs>
// reads n queries of dim little-endian doubles from <file>, prepares each as an 8-bit index's host form does (divided by
// gs first where gs > 0, as a Euclidean sketch call does) and prints per query
//   image <hex of the 48 * ceil(dim / 16) bytes>
//   meta <qnorm> <m1> <qscale> <qconst> <qnorm2>      (the doubles' bit patterns, hex)
// then the batch rule:  min <kQueryPrepMin>  and  serves <option> <batch> <0|1>  for options -1 .. 3, batches 0 .. 70.
// The Python side restates the rule and compares.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../syzgydb_amd/csrc/query_prep.h"
#include "../../syzgydb_amd/csrc/sketch_plan.h"

static uint64_t bits_of(double x)
{
    uint64_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

int main(int argc, char **argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: %s file dim n cosine planes gs\n", argv[0]);
        return 2;
    }
    const int dim = atoi(argv[2]), n = atoi(argv[3]), cosine = atoi(argv[4]), planes = atoi(argv[5]);
    const double gs = atof(argv[6]);
    if (dim < 1 || n < 0 || (planes != 2 && planes != 3)) return 2;
    std::vector<double> q((size_t)n * dim);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(q.data(), sizeof(double), q.size(), f) != q.size()) {
        fprintf(stderr, "cannot read %zu doubles from %s\n", q.size(), argv[1]);
        return 2;
    }
    fclose(f);
    const int r16 = (dim + 15) / 16;
    // (exactly the image's bytes on the heap: a write beyond them is the sanitizer's to find)
    std::vector<uint8_t> image(szg::qp_image_bytes(r16));
    std::vector<double> scaled(dim);
    for (int j = 0; j < n; j++) {
        const double *qj = q.data() + (size_t)j * dim;
        if (gs > 0.0) {
            for (int e = 0; e < dim; e++) scaled[e] = qj[e] / gs;
            qj = scaled.data();
        }
        memset(image.data(), 0xAB, image.size());  // (the rule zeroes what no element reaches)
        szg::QueryPrepConsts c;
        szg::query_prep8(qj, dim, cosine, planes, r16, image.data(), &c);
        printf("image ");
        for (uint8_t b : image) printf("%02x", b);
        printf("\nmeta %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits_of(c.qnorm), bits_of(c.m1),
               bits_of(c.qscale), bits_of(c.qconst), bits_of(c.qnorm2));
        // the pieces agree with the whole: every element's digits recombine to its Q, and the Qs sum to qconst
        long long sum = 0;
        const double scale = szg::qp_scale(cosine, 8, c.m1);
        for (int e = 0; e < dim; e++) {
            const long long Q = szg::qp_quantize(qj[e], scale, c.qscale, szg::qp_qmax8(planes));
            long long back = 0;
            for (int x = 3 - planes; x <= 2; x++)
                back = back * 128 + (int8_t)image[szg::qp_word(x, r16, e) * 4 + szg::qp_byte(e)];
            if (back != Q) {
                printf("FAIL query %d element %d: digits give %lld, Q is %lld\n", j, e, back, Q);
                return 1;
            }
            sum += Q;
        }
        if ((double)sum != c.qconst) {
            printf("FAIL query %d: qconst\n", j);
            return 1;
        }
    }
    printf("min %d\n", szgi::kQueryPrepMin);
    for (int o = -1; o <= 3; o++)
        for (int b = 0; b <= 70; b++) printf("serves %d %d %d\n", o, b, szgi::query_prep_serves(o, b) ? 1 : 0);
    printf("query prep ok\n");
    return 0;
}
