// The float64 arithmetic of the FPFH descriptor (csrc/fpfh.hip, "v6n"): the viewpoint orientation test, the Darboux-frame
// pair feature and the three bin functions.  Every value is a function of + - * / sqrt alone, in the operation order written here, so that the
// device, a host program and the numpy restatement (tests/_fpfh_oracle.py) agree bit for bit (-ffp-contract=off everywhere).  Plain C++ so
// that a host program can include it and check it without a device.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FPFH_HD __host__ __device__ __forceinline__
#else
#define FPFH_HD inline
#endif

namespace fpfh_math {

constexpr int BINS = 11;               // per feature
constexpr int WIDTH = 3 * BINS;        // the descriptor: bins of atan2(y, x), then of f2, then of f3

FPFH_HD double dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// true: the normal n at x points away from the viewpoint c and is to be negated.  A dot product of exactly 0 keeps the sign.
FPFH_HD bool orient_flip(const double *n, const double *x, const double *c) { return dot3(n[0], n[1], n[2], c[0] - x[0], c[1] - x[1], c[2] - x[2]) < 0.0; }

struct Pair { double y, x, f2, f3; };          // the first feature is the angle atan2(y, x); f2 = v . nb; f3 = na . dp / |dp|

// The pair feature of (i, j): dp = x_j - x_i with d2 = |dp|^2 > 0, ni and nj the oriented unit normals.  The frame's origin is the point
// whose normal makes the smaller angle with the connecting line (|a1| < |a2|, strict: swap).  false: dp is parallel to that normal, there
// is no frame and the pair is skipped.
FPFH_HD bool pair_feature(const double *dp_in, double d2, const double *ni, const double *nj, Pair &out) {
    const double d = sqrt(d2);
    const double a1 = dot3(ni[0], ni[1], ni[2], dp_in[0], dp_in[1], dp_in[2]) / d;
    const double a2 = dot3(nj[0], nj[1], nj[2], dp_in[0], dp_in[1], dp_in[2]) / d;
    const bool swap = fabs(a1) < fabs(a2);
    const double na0 = swap ? nj[0] : ni[0], na1 = swap ? nj[1] : ni[1], na2 = swap ? nj[2] : ni[2];
    const double nb0 = swap ? ni[0] : nj[0], nb1 = swap ? ni[1] : nj[1], nb2 = swap ? ni[2] : nj[2];
    const double p0 = swap ? -dp_in[0] : dp_in[0], p1 = swap ? -dp_in[1] : dp_in[1], p2 = swap ? -dp_in[2] : dp_in[2];
    out.f3 = swap ? -a2 : a1;
    double v0 = p1 * na2 - p2 * na1, v1 = p2 * na0 - p0 * na2, v2 = p0 * na1 - p1 * na0;          // v = dp x na
    const double vn = sqrt(dot3(v0, v1, v2, v0, v1, v2));
    if (vn == 0.0) return false;
    v0 /= vn; v1 /= vn; v2 /= vn;
    const double w0 = na1 * v2 - na2 * v1, w1 = na2 * v0 - na0 * v2, w2 = na0 * v1 - na1 * v0;    // w = na x v
    out.f2 = dot3(v0, v1, v2, nb0, nb1, nb2);
    out.y = dot3(w0, w1, w2, nb0, nb1, nb2);
    out.x = dot3(na0, na1, na2, nb0, nb1, nb2);
    return true;
}

// bin of f in [-1, 1]: clamp(floor((11 (f + 1)) 0.5), 0, 10)
FPFH_HD int bin_linear(double f) { return (int)fmin(fmax(floor((11.0 * (f + 1.0)) * 0.5), 0.0), 10.0); }

// bin of atan2(y, x) over (-pi, pi] without the arc tangent: bin edge k = 6..10 lies at theta_k = pi (2 k - 11) / 11, and the angle is at or past
// it iff cos(theta_k) y - sin(theta_k) x >= 0.  The lower half plane mirrors the upper one.  (Same digits as tests/_fpfh_oracle.py EDGE_C, EDGE_S.)
FPFH_HD int bin_angle(double y, double x) {
    constexpr double C6 = 0.9594929736144974, S6 = 0.28173255684142967;
    constexpr double C7 = 0.6548607339452851, S7 = 0.7557495743542583;
    constexpr double C8 = 0.14231483827328512, S8 = 0.9898214418809327;
    constexpr double C9 = -0.4154150130018863, S9 = 0.9096319953545184;
    constexpr double C10 = -0.8412535328311811, S10 = 0.5406408174555978;
    if (x == 0.0 && y == 0.0) return 5;
    if (y >= 0.0)
        return 5 + (int)(C6 * y - S6 * x >= 0.0) + (int)(C7 * y - S7 * x >= 0.0) + (int)(C8 * y - S8 * x >= 0.0) + (int)(C9 * y - S9 * x >= 0.0) +
               (int)(C10 * y - S10 * x >= 0.0);
    const double z = -y;
    return 5 - (int)(C6 * z - S6 * x > 0.0) - (int)(C7 * z - S7 * x > 0.0) - (int)(C8 * z - S8 * x > 0.0) - (int)(C9 * z - S9 * x > 0.0) -
           (int)(C10 * z - S10 * x > 0.0);
}

}  // namespace fpfh_math
