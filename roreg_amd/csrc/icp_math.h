// Small float64 linear algebra of the point-to-plane and plane-to-plane ICP (csrc/icp.hip, "v6d", "v6i", "v6p"): symmetric eigen-decompositions by
// cyclic Jacobi, the rigid update, the plane-to-plane weight matrix and the robust losses' weights.  Plain C++ so that a host program can include it and
// check it without a device.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ICP_HD __host__ __device__ __forceinline__
#else
#define ICP_HD inline
#endif

namespace icp_math {

// One Jacobi rotation of the symmetric pair (app, aqq, apq) -> (c, s) with t = s / c the smaller root: a'_pq = 0.
ICP_HD void jacobi_cs(double app, double aqq, double apq, double &c, double &s) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

// Symmetric 3x3 C (xx, xy, xz, yy, yz, zz) -> eigenvalues lam[3] (unsorted) and eigenvectors as the COLUMNS of V (row-major [3][3]).
// Every index is a compile-time constant once unrolled: the matrices live in registers.
ICP_HD void jacobi3(const double *C6, double *lam, double *V) {
    double a00 = C6[0], a01 = C6[1], a02 = C6[2], a11 = C6[3], a12 = C6[4], a22 = C6[5];
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
    const double scale = fmax(fmax(fabs(a00), fabs(a11)), fmax(fabs(a22), fmax(fabs(a01), fmax(fabs(a02), fabs(a12)))));
    const double tiny = 1e-22 * scale;
    for (int sweep = 0; sweep < 24; ++sweep) {
        if (!(fmax(fabs(a01), fmax(fabs(a02), fabs(a12))) > tiny)) break;
        double c, s, x, y;
        if (fabs(a01) > tiny) {                      // (p, q) = (0, 1); the third index is 2
            jacobi_cs(a00, a11, a01, c, s);
            const double t = s / c;
            a00 -= t * a01; a11 += t * a01; a01 = 0.0;
            x = a02; y = a12; a02 = c * x - s * y; a12 = s * x + c * y;
            x = v00; y = v01; v00 = c * x - s * y; v01 = s * x + c * y;
            x = v10; y = v11; v10 = c * x - s * y; v11 = s * x + c * y;
            x = v20; y = v21; v20 = c * x - s * y; v21 = s * x + c * y;
        }
        if (fabs(a02) > tiny) {                      // (0, 2); third index 1
            jacobi_cs(a00, a22, a02, c, s);
            const double t = s / c;
            a00 -= t * a02; a22 += t * a02; a02 = 0.0;
            x = a01; y = a12; a01 = c * x - s * y; a12 = s * x + c * y;
            x = v00; y = v02; v00 = c * x - s * y; v02 = s * x + c * y;
            x = v10; y = v12; v10 = c * x - s * y; v12 = s * x + c * y;
            x = v20; y = v22; v20 = c * x - s * y; v22 = s * x + c * y;
        }
        if (fabs(a12) > tiny) {                      // (1, 2); third index 0
            jacobi_cs(a11, a22, a12, c, s);
            const double t = s / c;
            a11 -= t * a12; a22 += t * a12; a12 = 0.0;
            x = a01; y = a02; a01 = c * x - s * y; a02 = s * x + c * y;
            x = v01; y = v02; v01 = c * x - s * y; v02 = s * x + c * y;
            x = v11; y = v12; v11 = c * x - s * y; v12 = s * x + c * y;
            x = v21; y = v22; v21 = c * x - s * y; v22 = s * x + c * y;
        }
    }
    lam[0] = a00; lam[1] = a11; lam[2] = a22;
    V[0] = v00; V[1] = v01; V[2] = v02; V[3] = v10; V[4] = v11; V[5] = v12; V[6] = v20; V[7] = v21; V[8] = v22;
}

// Symmetric n x n A (row-major, full; overwritten: its diagonal ends as the eigenvalues) and V (out: eigenvectors as columns).  Indexed at
// run time: the caller keeps A and V in memory that allows it (LDS on the device).
ICP_HD void jacobi_sym(double *A, double *V, int n) {
    double scale = 0.0;
    for (int i = 0; i < n * n; ++i) { V[i] = (i % (n + 1) == 0) ? 1.0 : 0.0; scale = fmax(scale, fabs(A[i])); }
    const double tiny = 1e-22 * scale;
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) off = fmax(off, fabs(A[p * n + q]));
        if (!(off > tiny)) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (!(fabs(apq) > tiny)) continue;
                double c, s;
                jacobi_cs(A[p * n + p], A[q * n + q], apq, c, s);
                for (int k = 0; k < n; ++k) {
                    const double x = A[k * n + p], y = A[k * n + q];
                    A[k * n + p] = c * x - s * y; A[k * n + q] = s * x + c * y;
                }
                for (int k = 0; k < n; ++k) {
                    const double x = A[p * n + k], y = A[q * n + k];
                    A[p * n + k] = c * x - s * y; A[q * n + k] = s * x + c * y;
                }
                A[p * n + q] = 0.0; A[q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double x = V[k * n + p], y = V[k * n + q];
                    V[k * n + p] = c * x - s * y; V[k * n + q] = s * x + c * y;
                }
            }
    }
}

// dR = exp([w]x) (Rodrigues; the series below |w| = 1e-8), row-major.
ICP_HD void rodrigues(const double *w, double *dR) {
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(th2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double k2 = (K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c]) + K[r * 3 + 2] * K[6 + c];
            dR[r * 3 + c] = ((r == c ? 1.0 : 0.0) + a * K[r * 3 + c]) + b * k2;
        }
}

// Symmetric 3x3 S (xx, xy, xz, yy, yz, zz) -> M = S^-1 in the same layout, by the adjugate over the determinant.  No pivoting: meant for a
// well-conditioned S (gicp_weight's has its eigenvalues in [2 eps, 2]); the error of M is a few cond(S) roundings of its largest entry.
ICP_HD void inverse_sym3(const double *S, double *M) {
    const double s00 = S[0], s01 = S[1], s02 = S[2], s11 = S[3], s12 = S[4], s22 = S[5];
    const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
    const double inv = 1.0 / ((s00 * c00 + s01 * c01) + s02 * c02);
    M[0] = c00 * inv; M[1] = c01 * inv; M[2] = c02 * inv; M[3] = c11 * inv; M[4] = c12 * inv; M[5] = c22 * inv;
}

// The plane-to-plane weight of one correspondence: with the surface-aligned covariances C = V diag(1, 1, eps) V^T = I - kappa n n^T
// (kappa = 1 - eps, n the unit normal) of the target point (normal n) and of the source point moved by R (normal m = R n_p),
// S = C_q + R C_p R^T = 2 I - kappa (n n^T + m m^T) and M = S^-1.  A zero n or m (no valid normal) leaves that point the identity.
ICP_HD void gicp_weight(double nx, double ny, double nz, double mx, double my, double mz, double kappa, double *M) {
    const double S[6] = {2.0 - kappa * (nx * nx + mx * mx), 0.0 - kappa * (nx * ny + mx * my), 0.0 - kappa * (nx * nz + mx * mz),
                         2.0 - kappa * (ny * ny + my * my), 0.0 - kappa * (ny * nz + my * mz), 2.0 - kappa * (nz * nz + mz * mz)};
    inverse_sym3(S, M);
}

// The robust losses of the weighted second passes ("v6p"; the values of roreg_icp_loss in include/roreg_hip.h).
enum { LOSS_NONE = 0, LOSS_HUBER = 1, LOSS_CAUCHY = 2, LOSS_GM = 3, LOSS_TUKEY = 4 };

// The IRLS weight of a residual r at scale k > 0, with u = r / k: huber 1 (|u| <= 1) or 1 / |u|; cauchy 1 / (1 + u^2); gm (Geman-McClure)
// 1 / (1 + u^2)^2; tukey (1 - u^2)^2 (|u| <= 1) or 0; LOSS_NONE (and any other kind) 1.  All continuous in r.  Selects only, and ONE division
// beside u's: the three losses that divide do so by a denominator chosen first (|u| outside huber's unit interval, 1 + u^2 for cauchy and gm,
// else 1).  An overflowing u^2 gives 1 / inf = 0 (cauchy, gm), the branch |u| > 1 (tukey: 0) or 1 / |u| (huber): never NaN for a finite or
// infinite r.
ICP_HD double robust_weight(int kind, double r, double k) {
    const double u = r / k;
    const double a = fabs(u), u2 = u * u;
    const bool in = a <= 1.0;
    const double den = kind == LOSS_HUBER ? (in ? 1.0 : a) : ((kind == LOSS_CAUCHY || kind == LOSS_GM) ? 1.0 + u2 : 1.0);
    const double inv = 1.0 / den;
    const double t = 1.0 - u2;
    const double tukey = in ? t * t : 0.0;
    return kind == LOSS_TUKEY ? tukey : (kind == LOSS_GM ? inv * inv : inv);
}

// The residual the plane-to-plane method hands to robust_weight: q = d^T M d -> sqrt(2 eps q).  Where both normals agree M has 1 / (2 eps)
// along the normal and 1 / 2 in the surface, so this is the point-to-plane distance in metres plus eps times the tangential one: one scale
// means the same under both methods.  (q is a positive-definite form; the clamp only keeps a rounding below zero from becoming NaN.)
ICP_HD double gicp_residual(double q, double epsilon) { return sqrt((2.0 * epsilon) * fmax(q, 0.0)); }

}  // namespace icp_math
