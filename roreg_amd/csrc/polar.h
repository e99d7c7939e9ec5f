// 3x3 polar factors in fp64 for the Kabsch fits: polar_uvt is the refinements' R = U V^T (csrc/ransac.hip, the reference's value: no
// determinant fix), polar_proper the rotation of the spatial-compatibility hypotheses (csrc/sc2.hip).  Include after the translation unit's
// `#pragma clang fp contract(off)`; internal linkage, one copy per translation unit.  Plain C++ so that a host program can include it and
// check it without a device (tests/_polar_check.cpp).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define POLAR_HD __host__ __device__
#define POLAR_HD_INLINE __host__ __device__ __forceinline__
#else
#include <math.h>
#define POLAR_HD inline
#define POLAR_HD_INLINE inline
#endif

namespace {

// ---- 3x3 SVD polar factor R = U V^T by one-sided Jacobi (fp64) ----------------------------------------
POLAR_HD void polar_uvt(const double *Hm, double *R) {
    // A (columns a0,a1,a2) = H ; rotate column pairs until orthogonal: A = U S, accumulated V gives H = U S V^T
    double A[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) { A[i] = Hm[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    double scale = 0.0, sum = 0.0;
    for (int i = 0; i < 9; ++i) { scale = fmax(scale, fabs(A[i])); sum += A[i]; }
    if (sum != sum || scale > 1.7976931348623157e308) {   // a NaN or an infinite entry (fmax drops a NaN; inf - inf and NaN make the sum NaN):
        for (int i = 0; i < 9; ++i) R[i] = sum - sum;     // NaN in all nine, like the reference
        return;
    }
    if (!(scale > 0.0)) {     // H == 0 (single inlier): LAPACK returns U=V=I  -> R = I
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    // A polar factor does not depend on the scale of H, the convergence measure below does (its 1e-300, and alpha * beta overflows from
    // |H| ~ 1e77): divide by the power of two at the largest entry's exponent first.  Exact, so every value below is the unscaled run's times
    // that power of two, and R is the same bits at any scale.
    int ex;
    frexp(scale, &ex);
    for (int i = 0; i < 9; ++i) A[i] = ldexp(A[i], -ex);
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int r = 0; r < 3; ++r) {
                    alpha += A[r * 3 + p] * A[r * 3 + p];
                    beta += A[r * 3 + q] * A[r * 3 + q];
                    gamma += A[r * 3 + p] * A[r * 3 + q];
                }
                if (gamma == 0.0) continue;
                off = fmax(off, fabs(gamma) / sqrt(alpha * beta + 1e-300));
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; ++r) {
                    const double ap = A[r * 3 + p], aq = A[r * 3 + q];
                    A[r * 3 + p] = c * ap - s * aq;
                    A[r * 3 + q] = s * ap + c * aq;
                    const double vp = V[r * 3 + p], vq = V[r * 3 + q];
                    V[r * 3 + p] = c * vp - s * vq;
                    V[r * 3 + q] = s * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    double U[9], nrm[3];
    for (int c = 0; c < 3; ++c) {
        nrm[c] = sqrt(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
    }
    const double tol = 1e-13 * fmax(nrm[0], fmax(nrm[1], nrm[2]));
    int good[3], ngood = 0;
    for (int c = 0; c < 3; ++c) {
        good[c] = nrm[c] > tol;
        ngood += good[c];
        for (int r = 0; r < 3; ++r) U[r * 3 + c] = good[c] ? A[r * 3 + c] / nrm[c] : 0.0;
    }
    if (ngood == 2) {        // complete the basis so that U V^T is a proper rotation
        int z = !good[0] ? 0 : (!good[1] ? 1 : 2);
        int a = (z + 1) % 3, b = (z + 2) % 3;
        double cx = U[3 + a] * U[6 + b] - U[6 + a] * U[3 + b];
        double cy = U[6 + a] * U[0 + b] - U[0 + a] * U[6 + b];
        double cz = U[0 + a] * U[3 + b] - U[3 + a] * U[0 + b];
        // det(V) sign decides the orientation of the completed column
        const double detV = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
        const double sg = detV >= 0 ? 1.0 : -1.0;
        U[0 + z] = sg * cx; U[3 + z] = sg * cy; U[6 + z] = sg * cz;
    } else if (ngood < 2) {  // rank <= 1: no unique answer; fall back to identity like the H==0 case
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = U[r * 3] * V[c * 3] + U[r * 3 + 1] * V[c * 3 + 1] + U[r * 3 + 2] * V[c * 3 + 2];
}

POLAR_HD_INLINE double det3(const double *R) {
    return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

// The proper rotation nearest H: U diag(1, 1, det(U V^T)) V^T with the sign on the SMALLEST singular direction.  polar_uvt gives R0 = U V^T;
// where that is a reflection, R0^T H = V S V^T is symmetric with the singular values as eigenvalues, v3 = its eigenvector of the smallest one
// (cyclic Jacobi on the symmetric part), and U diag(1, 1, -1) V^T = R0 - 2 (R0 v3) v3^T.
POLAR_HD void polar_proper(const double *Hm, double *R) {
    polar_uvt(Hm, R);
    if (!(det3(R) < 0.0)) return;
    double B[9], E[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) B[r * 3 + c] = R[0 + r] * Hm[0 + c] + R[3 + r] * Hm[3 + c] + R[6 + r] * Hm[6 + c];
    for (int r = 0; r < 3; ++r)
        for (int c = r + 1; c < 3; ++c) { const double m = 0.5 * (B[r * 3 + c] + B[c * 3 + r]); B[r * 3 + c] = m; B[c * 3 + r] = m; }
    for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = fabs(B[1]) + fabs(B[2]) + fabs(B[5]);
        if (off <= 1e-17 * (fabs(B[0]) + fabs(B[4]) + fabs(B[8]))) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = B[p * 3 + q];
                if (apq == 0.0) continue;
                const double theta = (B[q * 3 + q] - B[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < 3; ++k) {                       // B <- B J
                    const double bp = B[k * 3 + p], bq = B[k * 3 + q];
                    B[k * 3 + p] = c * bp - s * bq; B[k * 3 + q] = s * bp + c * bq;
                }
                for (int k = 0; k < 3; ++k) {                       // B <- J^T B
                    const double bp = B[p * 3 + k], bq = B[q * 3 + k];
                    B[p * 3 + k] = c * bp - s * bq; B[q * 3 + k] = s * bp + c * bq;
                }
                for (int k = 0; k < 3; ++k) {                       // E <- E J (columns = eigenvectors)
                    const double ep = E[k * 3 + p], eq = E[k * 3 + q];
                    E[k * 3 + p] = c * ep - s * eq; E[k * 3 + q] = s * ep + c * eq;
                }
            }
    }
    int z = 0;
    if (B[4] < B[z * 4]) z = 1;
    if (B[8] < B[z * 4]) z = 2;
    const double v[3] = {E[0 + z], E[3 + z], E[6 + z]};
    for (int r = 0; r < 3; ++r) {
        const double u = R[r * 3] * v[0] + R[r * 3 + 1] * v[1] + R[r * 3 + 2] * v[2];
        for (int c = 0; c < 3; ++c) R[r * 3 + c] -= 2.0 * u * v[c];
    }
}

}  // namespace
