// Small float64 linear algebra of the pose-graph optimiser (csrc/pose_graph.hip, "v6h"): the edge residual with its structured Jacobians,
// Shepperd's quaternion, the robust weight, the pose update and an in-place Cholesky factorisation of a small block that takes the calling
// thread's rank, so that the device runs it with a workgroup and a host program with one thread.  Plain C++ as icp_math.h is: a host program
// includes it and checks it without a device.
#pragma once
#include <math.h>
#include "icp_math.h"

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ __forceinline__
#else
#define PG_HD inline
#endif

namespace pg_math {

// c = a b, 3x3 row-major; every entry (a0 b0 + a1 b1) + a2 b2
PG_HD void mul33(const double *a, const double *b, double *c) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) c[r * 3 + k] = (a[r * 3] * b[k] + a[r * 3 + 1] * b[3 + k]) + a[r * 3 + 2] * b[6 + k];
}
// c = a^T b
PG_HD void mulT33(const double *a, const double *b, double *c) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) c[r * 3 + k] = (a[r] * b[k] + a[3 + r] * b[3 + k]) + a[6 + r] * b[6 + k];
}
// y = a^T x
PG_HD void mulT3(const double *a, const double *x, double *y) {
    for (int r = 0; r < 3; ++r) y[r] = (a[r] * x[0] + a[3 + r] * x[1]) + a[6 + r] * x[2];
}
PG_HD void skew(const double *v, double *K) {
    K[0] = 0.0; K[1] = -v[2]; K[2] = v[1]; K[3] = v[2]; K[4] = 0.0; K[5] = -v[0]; K[6] = -v[1]; K[7] = v[0]; K[8] = 0.0;
}
// rotation and translation of a row-major [4,4] pose
PG_HD void split_pose(const double *P, double *R, double *t) {
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) R[r * 3 + k] = P[r * 4 + k];
        t[r] = P[r * 4 + 3];
    }
}

// Unit quaternion q = (w, x, y, z), w >= 0, of a rotation by Shepperd's rule: the largest of w, x, y, z (tr >= R_kk <=> w^2 >= that axis'
// square) is taken from the square root, the others from the off-diagonal sums; then normalised, then the sign.
PG_HD void rot_to_quat(const double *R, double *q) {
    const double tr = (R[0] + R[4]) + R[8];
    double w, x, y, z;
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        w = 0.5 * sqrt(1.0 + tr);
        const double s = 0.25 / w;
        x = (R[7] - R[5]) * s; y = (R[2] - R[6]) * s; z = (R[3] - R[1]) * s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        x = 0.5 * sqrt(((1.0 + R[0]) - R[4]) - R[8]);
        const double s = 0.25 / x;
        w = (R[7] - R[5]) * s; y = (R[1] + R[3]) * s; z = (R[2] + R[6]) * s;
    } else if (R[4] >= R[8]) {
        y = 0.5 * sqrt(((1.0 - R[0]) + R[4]) - R[8]);
        const double s = 0.25 / y;
        w = (R[2] - R[6]) * s; x = (R[1] + R[3]) * s; z = (R[5] + R[7]) * s;
    } else {
        z = 0.5 * sqrt(((1.0 - R[0]) - R[4]) + R[8]);
        const double s = 0.25 / z;
        w = (R[3] - R[1]) * s; x = (R[2] + R[6]) * s; y = (R[5] + R[7]) * s;
    }
    const double nrm = sqrt(((w * w + x * x) + y * y) + z * z);
    const double sg = (w < 0.0 ? -1.0 : 1.0) / nrm;
    q[0] = w * sg; q[1] = x * sg; q[2] = y * sg; q[3] = z * sg;
}

// M = P_i^-1 P_j and E = T^-1 M, every inverse by transposition (the upper-left blocks are taken to be rotations):
// Rm = Ri^T Rj, tm = Ri^T (tj - ti), RE = Rt^T Rm, tE = Rt^T (tm - tt); e = (tE, vector part of the quaternion of RE), q the quaternion.
PG_HD void edge_error(const double *Pi, const double *Pj, const double *T, double *Rm, double *tm, double *RE, double *e, double *q) {
    double Ri[9], ti[3], Rj[9], tj[3], Rt[9], tt[3], d[3];
    split_pose(Pi, Ri, ti); split_pose(Pj, Rj, tj); split_pose(T, Rt, tt);
    mulT33(Ri, Rj, Rm);
    for (int r = 0; r < 3; ++r) d[r] = tj[r] - ti[r];
    mulT3(Ri, d, tm);
    mulT33(Rt, Rm, RE);
    for (int r = 0; r < 3; ++r) d[r] = tm[r] - tt[r];
    mulT3(Rt, d, e);
    rot_to_quat(RE, q);
    e[3] = q[1]; e[4] = q[2]; e[5] = q[3];
}

// chi2 = e^T Lambda e: Le_r = sum_c Lambda[r][c] e_c and the outer sum, both in ascending index starting from the first term
PG_HD double chi2_of(const double *e, const double *Lam) {
    double s = 0.0;
    for (int r = 0; r < 6; ++r) {
        double le = Lam[r * 6] * e[0];
        for (int c = 1; c < 6; ++c) le += Lam[r * 6 + c] * e[c];
        s = (r == 0) ? e[0] * le : s + e[r] * le;
    }
    return s;
}

// rho and the IRLS weight of an edge: tau <= 0 = no robust kernel.  Lambda[0,0] = 0 (no correspondences): the edge contributes nothing.
PG_HD void robust(double chi2, double lam00, double tau, double &rho, double &w) {
    if (!(lam00 > 0.0) && !(lam00 < 0.0)) { rho = 0.0; w = 0.0; return; }
    if (tau > 0.0) {
        const double mu = (tau * tau) * lam00;
        const double r = mu / (mu + chi2);
        rho = (mu * chi2) / (mu + chi2);
        w = r * r;
    } else { rho = chi2; w = 1.0; }
}

// The structured Jacobians of e under P <- P [Exp(omega), v; 0, 1], delta = (v, omega):
//   J_j = blockdiag(RE, Q), Q = (w I + [qv]x) / 2;   J_i = -J_j Ad(M^-1) = -[[A, B], [0, D]],
//   A = RE Rmi, B = RE [tmi]x Rmi, D = Q Rmi with M^-1 = (Rmi, tmi) = (Rm^T, -Rm^T tm).
PG_HD void edge_jacobians(const double *Rm, const double *tm, const double *RE, const double *q, double *Q, double *A, double *B, double *D) {
    double K[9], Rmi[9], tmi[3], KR[9];
    skew(q + 1, K);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Q[r * 3 + c] = 0.5 * ((r == c ? q[0] : 0.0) + K[r * 3 + c]);
            Rmi[r * 3 + c] = Rm[c * 3 + r];
        }
    mulT3(Rm, tm, tmi);
    for (int r = 0; r < 3; ++r) tmi[r] = -tmi[r];
    mul33(RE, Rmi, A);
    skew(tmi, K);
    mul33(K, Rmi, KR);
    mul33(RE, KR, B);
    mul33(Q, Rmi, D);
}

// entry (r, c) of the dense 6x6 Jacobian from the record (RE, Q, A, B, D), for the edge's j side or i side
PG_HD double dense_J(const double *RE, const double *Q, const double *A, const double *B, const double *D, bool j_side, int r, int c) {
    const int rr = r % 3, cc = c % 3;
    if (j_side) return (r < 3) == (c < 3) ? (r < 3 ? RE[rr * 3 + cc] : Q[rr * 3 + cc]) : 0.0;
    if (r < 3) return c < 3 ? -A[rr * 3 + cc] : -B[rr * 3 + cc];
    return c < 3 ? 0.0 : -D[rr * 3 + cc];
}

// P' = P [Exp(omega), v; 0, 1], delta = (v, omega): R' = R dR, t' = R v + t; the last row is copied
PG_HD void pose_update(const double *P, const double *delta, double *Pn) {
    double R[9], t[3], dR[9], Rn[9];
    split_pose(P, R, t);
    icp_math::rodrigues(delta + 3, dR);
    mul33(R, dR, Rn);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Pn[r * 4 + c] = Rn[r * 3 + c];
        Pn[r * 4 + 3] = ((R[r * 3] * delta[0] + R[r * 3 + 1] * delta[1]) + R[r * 3 + 2] * delta[2]) + t[r];
    }
    for (int c = 0; c < 4; ++c) Pn[12 + c] = P[12 + c];
}

// P_child = P_parent T (forward) or P_parent T^-1 (inverse by transposition); the last row is (0, 0, 0, 1)
PG_HD void pose_compose(const double *Pp, const double *T, bool inverse, double *Pc) {
    double R[9], t[3], Rt[9], tt[3], Rn[9], u[3];
    split_pose(Pp, R, t); split_pose(T, Rt, tt);
    if (inverse) {
        double Ri[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) Ri[r * 3 + c] = Rt[c * 3 + r];
        mulT3(Rt, tt, u);
        for (int r = 0; r < 3; ++r) { tt[r] = -u[r]; }
        for (int k = 0; k < 9; ++k) Rt[k] = Ri[k];
    }
    mul33(R, Rt, Rn);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Pc[r * 4 + c] = Rn[r * 3 + c];
        Pc[r * 4 + 3] = ((R[r * 3] * tt[0] + R[r * 3 + 1] * tt[1]) + R[r * 3 + 2] * tt[2]) + t[r];
    }
    Pc[12] = 0.0; Pc[13] = 0.0; Pc[14] = 0.0; Pc[15] = 1.0;
}

struct NoSync { PG_HD void operator()() const {} };

// In-place Cholesky factorisation A = L L^T of the lower triangle of a small n x n block (row-major, leading dimension ld), right-looking
// and unblocked, by `nt` threads of which the caller is number `tid`; sync() is a barrier over them that also orders their writes to A.
// A host program calls it with (0, 1, NoSync()).  Returns false at the first pivot that is not positive and finite; every thread reads the
// same pivot, so all of them return together.
template <class Sync>
PG_HD bool chol_lower(double *A, int n, int ld, int tid, int nt, Sync sync) {
    for (int j = 0; j < n; ++j) {
        const double d = A[j * ld + j];
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return false;
        const double s = sqrt(d);
        sync();
        if (tid == 0) A[j * ld + j] = s;
        for (int i = j + 1 + tid; i < n; i += nt) A[i * ld + j] = A[i * ld + j] / s;
        sync();
        const int m = n - j - 1;
        for (int idx = tid; idx < m * m; idx += nt) {
            const int i = j + 1 + idx / m, k = j + 1 + idx % m;
            if (k <= i) A[i * ld + k] = A[i * ld + k] - A[i * ld + j] * A[k * ld + j];
        }
        sync();
    }
    return true;
}

// x <- L^-1 x and x <- L^-T x for the lower-triangular n x n block L (row-major, ld), one thread
PG_HD void trsv_lower(const double *L, int n, int ld, double *x) {
    for (int j = 0; j < n; ++j) {
        double s = x[j];
        for (int p = 0; p < j; ++p) s -= L[j * ld + p] * x[p];
        x[j] = s / L[j * ld + j];
    }
}
PG_HD void trsv_lower_t(const double *L, int n, int ld, double *x) {
    for (int j = n - 1; j >= 0; --j) {
        double s = x[j];
        for (int p = j + 1; p < n; ++p) s -= L[p * ld + j] * x[p];
        x[j] = s / L[j * ld + j];
    }
}

}  // namespace pg_math
