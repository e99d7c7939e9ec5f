// Stand-alone host program over csrc/icp_math.h's robust losses (tests/test_icp_robust_oracle.py compiles it with AddressSanitizer and
// UndefinedBehaviorSanitizer).  argv[1]: a file of float64 rows (r, k, q, epsilon), 4 numbers each.  Per row it prints the bit patterns (hex)
// of robust_weight(kind, r, k) for kind = none, huber, cauchy, gm, tukey and of gicp_residual(q, epsilon).  The last line is the number of rows.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_math.h"

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s table\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> t;
    double buf[4];
    while (fread(buf, sizeof(double), 4, f) == 4) t.insert(t.end(), buf, buf + 4);
    fclose(f);
    const size_t rows = t.size() / 4;
    const int kinds[5] = {icp_math::LOSS_NONE, icp_math::LOSS_HUBER, icp_math::LOSS_CAUCHY, icp_math::LOSS_GM, icp_math::LOSS_TUKEY};
    for (size_t r = 0; r < rows; ++r) {
        const double *x = &t[r * 4];
        for (int q = 0; q < 5; ++q) printf("%016" PRIx64 " ", bits(icp_math::robust_weight(kinds[q], x[0], x[1])));
        printf("%016" PRIx64 "\n", bits(icp_math::gicp_residual(x[2], x[3])));
    }
    printf("%zu\n", rows);
    return 0;
}
