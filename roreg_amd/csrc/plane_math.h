// The scalar arithmetic of the RANSAC plane segmentation (csrc/plane.hip, "v6t"): the counter-based draws, the plane of three
// points and the inlier test.  Integers and + - * alone, in the operation order written here (no square root, no division), so that the device, a
// host program and the numpy restatement (tests/_plane_oracle.py) agree bit for bit (-ffp-contract=off everywhere).  Plain C++ so that a host
// program can include it and check it without a device.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLANE_HD __host__ __device__ __forceinline__
#else
#define PLANE_HD inline
#endif

namespace plane_math {

// the splitmix64 finaliser
PLANE_HD uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

PLANE_HD uint64_t round_base(uint64_t seed, int r) { return mix(seed ^ ((uint64_t)r << 32)); }

// slot j (0..2) of hypothesis h among L live rows (1 <= L < 2^32) -> a number in [0, L)
PLANE_HD uint32_t draw(uint64_t base, uint32_t h, int j, uint32_t L) {
    const uint64_t w = mix(base + 3ull * h + (uint64_t)j);
    return (uint32_t)(((w >> 32) * (uint64_t)L) >> 32);
}

struct Plane { double nx, ny, nz, q; };

// the plane through a, b, c -> false (invalid) when q is 0 or not finite
PLANE_HD bool plane_of(const double *a, const double *b, const double *c, Plane &p) {
    const double e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
    const double e2x = c[0] - a[0], e2y = c[1] - a[1], e2z = c[2] - a[2];
    p.nx = e1y * e2z - e1z * e2y;
    p.ny = e1z * e2x - e1x * e2z;
    p.nz = e1x * e2y - e1y * e2x;
    p.q = (p.nx * p.nx + p.ny * p.ny) + p.nz * p.nz;
    return p.q != 0.0 && isfinite(p.q);
}

// the inlier threshold of a plane: (dist dist) q, each product once
PLANE_HD double threshold(double dist, double q) {
    const double d2 = dist * dist;
    return d2 * q;
}

// the fourth word of the raw plane: -((nx ax + ny ay) + nz az)
PLANE_HD double offset(const Plane &p, const double *a) { return -((p.nx * a[0] + p.ny * a[1]) + p.nz * a[2]); }

// s s <= thr with s = (nx (px - ax) + ny (py - ay)) + nz (pz - az): inclusive; false for a NaN on either side
PLANE_HD bool inlier(double nx, double ny, double nz, double ax, double ay, double az, double thr, double px, double py, double pz) {
    const double s = (nx * (px - ax) + ny * (py - ay)) + nz * (pz - az);
    return s * s <= thr;
}

}  // namespace plane_math
