// Stand-alone host program over csrc/fpfh_math.h (tests/test_fpfh_oracle.py compiles it with AddressSanitizer and UndefinedBehaviorSanitizer).
// argv[1]: a file of float64 rows (x_i, n_i, x_j, n_j, c), 15 numbers each.  Per row it prints
//   flip_i flip_j skip b1 b2 b3
// the two orientation flags against the viewpoint c, then, on the ORIENTED normals, whether the pair (i, j) is skipped (d2 == 0 or no
// frame; the bins are then -1) and its three bins.  The last line is the number of rows.
#include <cstdio>
#include <vector>

#include "fpfh_math.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s table\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> t;
    double buf[15];
    while (fread(buf, sizeof(double), 15, f) == 15) t.insert(t.end(), buf, buf + 15);
    fclose(f);
    const size_t rows = t.size() / 15;
    for (size_t r = 0; r < rows; ++r) {
        const double *xi = &t[r * 15], *ni0 = xi + 3, *xj = xi + 6, *nj0 = xi + 9, *c = xi + 12;
        const bool fi = fpfh_math::orient_flip(ni0, xi, c), fj = fpfh_math::orient_flip(nj0, xj, c);
        double ni[3], nj[3], dp[3];
        for (int q = 0; q < 3; ++q) { ni[q] = fi ? -ni0[q] : ni0[q]; nj[q] = fj ? -nj0[q] : nj0[q]; dp[q] = xj[q] - xi[q]; }
        const double d2 = fpfh_math::dot3(dp[0], dp[1], dp[2], dp[0], dp[1], dp[2]);
        fpfh_math::Pair p;
        const bool ok = d2 > 0.0 && fpfh_math::pair_feature(dp, d2, ni, nj, p);
        if (ok)
            printf("%d %d 0 %d %d %d\n", (int)fi, (int)fj, fpfh_math::bin_angle(p.y, p.x), fpfh_math::bin_linear(p.f2), fpfh_math::bin_linear(p.f3));
        else
            printf("%d %d 1 -1 -1 -1\n", (int)fi, (int)fj);
    }
    printf("%zu\n", rows);
    return 0;
}
