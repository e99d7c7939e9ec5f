// Stand-alone host check of the plane-to-plane weight in roreg_amd/csrc/icp_math.h (tests/test_icp_gicp_oracle.py compiles it with
// -fsanitize=address,undefined and runs it): S S^-1 = I for S = 2 I - kappa (n n^T + m m^T) on seeded unit-normal pairs, on m = +n and
// m = -n (the worst conditioned: eigenvalues 2, 2, 2 eps), with one or both normals zero, at eps = 1e-3 and 1e-6.  Prints "ok" when all hold.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "icp_math.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {                               // xorshift64*: (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return ((rng_state * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-17;
}
static void unit(double *v) {
    double n2;
    do {
        for (int i = 0; i < 3; ++i) v[i] = 2.0 * uniform() - 1.0;
        n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    } while (n2 < 1e-2 || n2 > 1.0);
    const double n = sqrt(n2);
    for (int i = 0; i < 3; ++i) v[i] /= n;
}

// max |S M - I| for the pair (n, m) at kappa, and whether M is finite
static double residual(const double *n, const double *m, double kappa, bool &finite) {
    double M6[6];
    icp_math::gicp_weight(n[0], n[1], n[2], m[0], m[1], m[2], kappa, M6);
    const int ix[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    double S[3][3], worst = 0.0;
    finite = true;
    for (int q = 0; q < 6; ++q) finite = finite && std::isfinite(M6[q]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[r][c] = (r == c ? 2.0 : 0.0) - kappa * (n[r] * n[c] + m[r] * m[c]);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double v = 0.0;
            for (int k = 0; k < 3; ++k) v += S[r][k] * M6[ix[k][c]];
            worst = fmax(worst, fabs(v - (r == c ? 1.0 : 0.0)));
        }
    return worst;
}

int main() {
    int bad = 0;
    const double zero[3] = {0.0, 0.0, 0.0};
    for (double eps : {1e-3, 1e-6, 1.0}) {
        const double kappa = 1.0 - eps;
        // the entries of S are at most 2, so every cofactor carries an absolute error of a few 4 u (u = 2^-53) and the determinant
        // (>= 8 eps) a few 8 u: dM is a few u / eps in absolute terms plus a relative u / eps of M itself, and |S M - I| <= |S| |dM| + u / eps
        // = a few tens of u / eps.  Bound: 64 u / eps.
        const double bound = 64.0 * ldexp(1.0, -53) / eps;
        double worst = 0.0;
        for (int k = 0; k < 20000; ++k) {
            double n[3], m[3], neg[3];
            unit(n); unit(m);
            for (int i = 0; i < 3; ++i) neg[i] = -n[i];
            const double *pairs[6][2] = {{n, m}, {n, n}, {n, neg}, {n, zero}, {zero, m}, {zero, zero}};
            for (auto &p : pairs) {
                bool finite;
                const double r = residual(p[0], p[1], kappa, finite);
                worst = fmax(worst, r);
                if (!finite || !(r <= bound)) { if (bad < 5) printf("eps %g: residual %.3e over %.3e (finite %d)\n", eps, r, bound, (int)finite); ++bad; }
            }
            if (k < 2000) {                              // nearly agreeing normals: m = n turned by 1e-4 .. 1e-8 rad
                double near[3];
                const double th = pow(10.0, -4.0 - 4.0 * uniform());
                double nn = 0.0;
                for (int i = 0; i < 3; ++i) { near[i] = n[i] + th * m[i]; nn += near[i] * near[i]; }
                for (int i = 0; i < 3; ++i) near[i] /= sqrt(nn);
                bool finite;
                const double r = residual(n, near, kappa, finite);
                worst = fmax(worst, r);
                if (!finite || !(r <= bound)) { if (bad < 5) printf("eps %g, near pair: residual %.3e over %.3e\n", eps, r, bound); ++bad; }
            }
        }
        printf("eps %g: worst |S M - I| = %.3e (bound %.3e)\n", eps, worst, bound);
    }
    // the zero pair and eps = 1 give M = I / 2 exactly
    double M6[6];
    icp_math::gicp_weight(0, 0, 0, 0, 0, 0, 0.999, M6);
    if (!(M6[0] == 0.5 && M6[3] == 0.5 && M6[5] == 0.5 && M6[1] == 0.0 && M6[2] == 0.0 && M6[4] == 0.0)) { printf("zero normals: M is not I / 2\n"); ++bad; }
    icp_math::gicp_weight(0.6, 0.8, 0.0, 0.0, 0.6, -0.8, 0.0, M6);
    if (!(M6[0] == 0.5 && M6[3] == 0.5 && M6[5] == 0.5 && M6[1] == 0.0 && M6[2] == 0.0 && M6[4] == 0.0)) { printf("eps = 1: M is not I / 2\n"); ++bad; }
    if (bad) { printf("%d failures\n", bad); return 1; }
    printf("ok\n");
    return 0;
}
