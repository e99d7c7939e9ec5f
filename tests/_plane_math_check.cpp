// Stand-alone host program over csrc/plane_math.h (tests/test_plane_oracle.py compiles it with AddressSanitizer and UndefinedBehaviorSanitizer).
// argv[1]: a file of int64 n, H, R, uint64 seed, float64 dist, then n rows of three float32.  The live rows are the rows with finite coordinates,
// in ascending order, in every round (nothing is labelled here).  Per round r < R and hypothesis h < H it prints
//   r h i0 i1 i2 valid nx ny nz d count
// the three draws, whether the hypothesis is valid, the raw plane as the bits of its four float64 words in hexadecimal (0 when invalid) and its
// count (-1 when invalid).  The last line is the number of live rows.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "plane_math.h"

static uint64_t bits(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s table\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t head[3];
    uint64_t seed;
    double dist;
    if (fread(head, sizeof(int64_t), 3, f) != 3 || fread(&seed, sizeof seed, 1, f) != 1 || fread(&dist, sizeof dist, 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int64_t n = head[0], H = head[1], R = head[2];
    if (n < 0 || n > (1 << 20) || H < 0 || H > (1 << 20) || R < 0 || R > 64) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> p((size_t)n * 3);
    if (n && fread(p.data(), sizeof(float), p.size(), f) != p.size()) { fprintf(stderr, "short table\n"); return 2; }
    fclose(f);
    std::vector<double> X;
    for (int64_t i = 0; i < n; ++i)
        if (isfinite(p[3 * i]) && isfinite(p[3 * i + 1]) && isfinite(p[3 * i + 2]))
            for (int k = 0; k < 3; ++k) X.push_back((double)p[3 * i + k]);
    const uint32_t L = (uint32_t)(X.size() / 3);
    for (int r = 0; r < R && L >= 3; ++r) {
        const uint64_t base = plane_math::round_base(seed, r);
        for (int64_t h = 0; h < H; ++h) {
            const uint32_t i0 = plane_math::draw(base, (uint32_t)h, 0, L), i1 = plane_math::draw(base, (uint32_t)h, 1, L), i2 = plane_math::draw(base, (uint32_t)h, 2, L);
            plane_math::Plane pl{0.0, 0.0, 0.0, 0.0};
            const double *a = &X[3 * (size_t)i0];
            const bool valid = i0 != i1 && i0 != i2 && i1 != i2 && plane_math::plane_of(a, &X[3 * (size_t)i1], &X[3 * (size_t)i2], pl);
            long count = -1;
            double d = 0.0;
            if (valid) {
                const double thr = plane_math::threshold(dist, pl.q);
                d = plane_math::offset(pl, a);
                count = 0;
                for (uint32_t i = 0; i < L; ++i)
                    count += plane_math::inlier(pl.nx, pl.ny, pl.nz, a[0], a[1], a[2], thr, X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]);
            } else {
                pl = plane_math::Plane{0.0, 0.0, 0.0, 0.0};
            }
            printf("%d %" PRId64 " %u %u %u %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %ld\n", r, h, i0, i1, i2, (int)valid, bits(pl.nx), bits(pl.ny),
                   bits(pl.nz), bits(d), count);
        }
    }
    printf("%u\n", L);
    return 0;
}
