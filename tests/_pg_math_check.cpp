// Stand-alone host check of roreg_amd/csrc/pg_math.h (tests/test_pose_graph_oracle.py compiles it with -fsanitize=address,undefined and runs
// it): the Cholesky block factorisation and the two triangular solves against A = L L^T and A x = b, a refused pivot, and the structured
// Jacobians of the edge residual against central differences of the residual routine itself.  Prints the worst figures; exit status 0 = all
// within their bounds.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pg_math.h"

static unsigned long long state = 0x9e3779b97f4a7c15ull;
static double uniform() {                                   // xorshift64*, (-1, 1)
    state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
    return (double)((state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

static void random_pose(double angle_scale, double *P) {
    double w[3] = {uniform() * angle_scale, uniform() * angle_scale, uniform() * angle_scale}, R[9];
    icp_math::rodrigues(w, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[r * 4 + c] = R[r * 3 + c];
        P[r * 4 + 3] = 2.0 * uniform();
    }
    P[12] = P[13] = P[14] = 0.0; P[15] = 1.0;
}

static void residual(const double *Pi, const double *Pj, const double *T, double *e) {
    double Rm[9], tm[3], RE[9], q[4];
    pg_math::edge_error(Pi, Pj, T, Rm, tm, RE, e, q);
}

int main() {
    int bad = 0;
    // Cholesky and the solves, every block size the device can meet, in a buffer of exactly the size used (the sanitizer sees any overrun)
    double worst_llt = 0.0, worst_solve = 0.0;
    for (int n = 1; n <= 32; ++n) {
        const int ld = 33;
        std::vector<double> B((size_t)n * n), A((size_t)(n - 1) * ld + n), L((size_t)(n - 1) * ld + n), x(n), b(n);
        for (double &v : B) v = uniform();
        double scale = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) {
                double s = (i == j) ? 0.5 : 0.0;
                for (int k = 0; k < n; ++k) s += B[(size_t)i * n + k] * B[(size_t)j * n + k];
                A[(size_t)i * ld + j] = s; L[(size_t)i * ld + j] = s;
                scale = fmax(scale, fabs(s));
            }
        if (!pg_math::chol_lower(L.data(), n, ld, 0, 1, pg_math::NoSync())) { printf("n=%d: pivot refused\n", n); bad = 1; continue; }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) {
                double s = 0.0;
                for (int k = 0; k <= j; ++k) s += L[(size_t)i * ld + k] * L[(size_t)j * ld + k];
                worst_llt = fmax(worst_llt, fabs(s - A[(size_t)i * ld + j]) / scale);
            }
        for (int i = 0; i < n; ++i) { b[i] = uniform(); x[i] = b[i]; }
        pg_math::trsv_lower(L.data(), n, ld, x.data());
        pg_math::trsv_lower_t(L.data(), n, ld, x.data());
        double xs = 0.0;
        for (int i = 0; i < n; ++i) xs = fmax(xs, fabs(x[i]));
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int k = 0; k < n; ++k) s += A[(size_t)(i > k ? i : k) * ld + (i > k ? k : i)] * x[k];
            worst_solve = fmax(worst_solve, fabs(s - b[i]) / (scale * xs * n));
        }
    }
    // backward errors: |L L^T - A| <= (n + 1) u |L||L|^T and the residual of the solve likewise, u = 1.1e-16, |L||L|^T <= n scale
    if (!(worst_llt <= 33.0 * 32.0 * 1.2e-16) || !(worst_solve <= 3.0 * 33.0 * 1.2e-16 * 32.0)) bad = 1;
    double Z[4] = {1.0, 0.0, 2.0, 1.0};                      // [[1, .], [2, 1]]: the second pivot is 1 - 4 < 0
    if (pg_math::chol_lower(Z, 2, 2, 0, 1, pg_math::NoSync())) { printf("a negative pivot was accepted\n"); bad = 1; }
    double N1[1] = {NAN};
    if (pg_math::chol_lower(N1, 1, 1, 0, 1, pg_math::NoSync())) { printf("a NaN pivot was accepted\n"); bad = 1; }

    // the structured Jacobians against central differences, h = 1e-6: truncation h^2 |e'''| / 6 ~ 1e-12, rounding 2^-53 |e| / h ~ 1e-9 at most
    double worst_jac = 0.0, worst_q = 0.0;
    for (int trial = 0; trial < 200; ++trial) {
        double Pi[16], Pj[16], T[16], N[16], Tt[16];
        random_pose(2.0, Pi); random_pose(2.0, Pj);
        random_pose(0.3, N);                                  // T = inv(Pi) Pj N: the residual's rotation stays well below 180 degrees
        double PiI[16], I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        pg_math::pose_compose(I4, Pi, true, PiI);
        pg_math::pose_compose(PiI, Pj, false, Tt);
        pg_math::pose_compose(Tt, N, false, T);
        double Rm[9], tm[3], RE[9], e[6], q[4], Q[9], A[9], Bm[9], D[9];
        pg_math::edge_error(Pi, Pj, T, Rm, tm, RE, e, q);
        pg_math::edge_jacobians(Rm, tm, RE, q, Q, A, Bm, D);
        worst_q = fmax(worst_q, fabs(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3] - 1.0));
        if (q[0] < 0.0) bad = 1;
        const double h = 1e-6;
        for (int c = 0; c < 6; ++c) {
            double dp[6] = {0, 0, 0, 0, 0, 0}, dm[6] = {0, 0, 0, 0, 0, 0}, Pp[16], Pm[16], ep[6], em[6];
            dp[c] = h; dm[c] = -h;
            pg_math::pose_update(Pj, dp, Pp); pg_math::pose_update(Pj, dm, Pm);
            residual(Pi, Pp, T, ep); residual(Pi, Pm, T, em);
            for (int r = 0; r < 6; ++r)
                worst_jac = fmax(worst_jac, fabs((ep[r] - em[r]) / (2 * h) - pg_math::dense_J(RE, Q, A, Bm, D, true, r, c)));
            pg_math::pose_update(Pi, dp, Pp); pg_math::pose_update(Pi, dm, Pm);
            residual(Pp, Pj, T, ep); residual(Pm, Pj, T, em);
            for (int r = 0; r < 6; ++r)
                worst_jac = fmax(worst_jac, fabs((ep[r] - em[r]) / (2 * h) - pg_math::dense_J(RE, Q, A, Bm, D, false, r, c)));
        }
    }
    if (!(worst_jac <= 5e-9) || !(worst_q <= 1e-15)) bad = 1;
    // the robust kernel's limits
    double rho, w;
    pg_math::robust(3.0, 0.0, 0.1, rho, w); if (rho != 0.0 || w != 0.0) bad = 1;
    pg_math::robust(3.0, 100.0, 0.0, rho, w); if (rho != 3.0 || w != 1.0) bad = 1;
    pg_math::robust(1.0, 4.0, 0.5, rho, w); if (rho != 0.5 || w != 0.25) bad = 1;
    printf("LLt %.3e solve %.3e jacobian %.3e quat %.3e %s\n", worst_llt, worst_solve, worst_jac, worst_q, bad ? "FAILED" : "ok");
    return bad;
}
