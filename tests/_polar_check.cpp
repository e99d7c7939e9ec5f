// Stand-alone host program over csrc/polar.h (tests/test_polar_oracle.py compiles it with AddressSanitizer and UndefinedBehaviorSanitizer).
// argv[1]: a file of float64 3x3 matrices, row-major, 9 numbers each.  Per matrix it prints the bit patterns (hex) of polar_uvt's nine
// values, then of polar_proper's nine.  The last line is the number of matrices.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "polar.h"

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s matrices\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<double> t;
    double buf[9];
    while (fread(buf, sizeof(double), 9, f) == 9) t.insert(t.end(), buf, buf + 9);
    fclose(f);
    const size_t rows = t.size() / 9;
    for (size_t r = 0; r < rows; ++r) {
        double R[9], P[9];
        polar_uvt(&t[r * 9], R);
        polar_proper(&t[r * 9], P);
        for (int q = 0; q < 9; ++q) printf("%016" PRIx64 " ", bits(R[q]));
        for (int q = 0; q < 9; ++q) printf("%016" PRIx64 "%c", bits(P[q]), q == 8 ? '\n' : ' ');
    }
    printf("%zu\n", rows);
    return 0;
}
