// RANSAC plane segmentation of dense clouds ("v6t").  No reference counterpart; tests/_plane_oracle.py is the numpy
// restatement, include/roreg_hip.h states the definition and plane_math.h holds its scalar arithmetic.  Every decision is an integer function
// of the input: the draws are counter based, the inlier test is a comparison of exactly rounded float64 values, the counts are integer sums
// and the winner is a total order, so the outputs are the same bytes on every run.
//
// A round is twelve launches and no host synchronisation: flag the live rows, scan (scan.h), compact them into the live list, draw the
// hypotheses, score them, select the winner, label its inliers and sum their moments, fit, sum the squared distances to the fit, close.  Whether
// a round runs is a function of two device words that earlier launches of the same stream wrote: n_planes[0] == r (every earlier round found a
// plane) and the live count L >= 3.  A round that does not run leaves every output alone.  No workgroup waits for another.
//
// The scoring pass (plane_score_kernel).  A workgroup owns a tile of PS_TILE live points, four per lane as float64 in registers, and a strided
// share of the hypothesis chunks.  Per chunk the first PS_CHUNK lanes build the records (normal, anchor, dist^2 q) from the triples into LDS;
// every wave then walks the records (all lanes read the same words: a broadcast), tests its 256 points with one ballot per register point and
// adds the population counts, a wave-uniform integer, to the chunk's LDS counters; the workgroup adds one integer per hypothesis to the global
// count.  Integer adds are order free.  Register arrays are indexed by unrolled loop counters only (the Makefile fails the build on scratch).
#include "common.h"
#include <algorithm>
#include <cmath>
#include <climits>

#include "icp_math.h"
#include "plane_math.h"

#pragma clang fp contract(off)

namespace {

#include "scan.h"

constexpr int PLANE_MAX_N = 1 << 30;
constexpr int PS_THREADS = ROREG_PLANE_THREADS;
constexpr int PS_PTS = ROREG_PLANE_TILE / ROREG_PLANE_THREADS;       // points a lane keeps
constexpr int PS_TILE = ROREG_PLANE_TILE;
constexpr int PS_CHUNK = ROREG_PLANE_HYP_CHUNK;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_TARGET_BLOCKS = 2048;                                // the hypothesis chunks are spread over grid.y until the launch has about this many workgroups
constexpr int MOM_W = 10;                                             // count, sum d (3), sum d d^T (xx, xy, xz, yy, yz, zz) with d = p - a
constexpr int FLAT_BLOCKS = 2048;                                     // grid-stride launches over rows
constexpr int SEL_THREADS = 1024;
static_assert(PS_THREADS == 256 && PS_PTS == 4 && PS_CHUNK <= PS_THREADS && PS_WAVES == 4, "the scoring kernel's shape");

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

struct Record { double nx, ny, nz, ax, ay, az, thr; bool valid; };

// The record of the hypothesis through the original rows (t0, t1, t2): invalid (thr = NaN: no point passes) for a row outside [0, n), a
// repeated row, a dead row or a degenerate plane.
__device__ __forceinline__ Record make_record(const float *__restrict__ pts, int n, int t0, int t1, int t2, double dist) {
    Record R{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, (double)NAN, false};
    if (t0 < 0 || t1 < 0 || t2 < 0 || t0 >= n || t1 >= n || t2 >= n || t0 == t1 || t0 == t2 || t1 == t2) return R;
    const float *pa = pts + (size_t)t0 * 3, *pb = pts + (size_t)t1 * 3, *pc = pts + (size_t)t2 * 3;
    const float a0 = pa[0], a1 = pa[1], a2 = pa[2], b0 = pb[0], b1 = pb[1], b2 = pb[2], c0 = pc[0], c1 = pc[1], c2 = pc[2];
    if (!finite3(a0, a1, a2) || !finite3(b0, b1, b2) || !finite3(c0, c1, c2)) return R;
    const double a[3] = {(double)a0, (double)a1, (double)a2}, b[3] = {(double)b0, (double)b1, (double)b2}, c[3] = {(double)c0, (double)c1, (double)c2};
    plane_math::Plane p;
    if (!plane_math::plane_of(a, b, c, p)) return R;
    R.nx = p.nx; R.ny = p.ny; R.nz = p.nz;
    R.ax = a[0]; R.ay = a[1]; R.az = a[2];
    R.thr = plane_math::threshold(dist, p.q);
    R.valid = true;
    return R;
}

// everything the outputs hold when no plane is found
__global__ __launch_bounds__(256) void plane_init_kernel(int n, int K, int32_t *__restrict__ labels, int32_t *__restrict__ n_planes, int32_t *__restrict__ counts,
                                                         int32_t *__restrict__ triples, double *__restrict__ raw, double *__restrict__ fit, double *__restrict__ rms) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) labels[i] = -1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < 4 * (int64_t)K; i += stride) {
        if (i < K) { counts[i] = 0; rms[i] = 0.0; }
        if (i < 3 * (int64_t)K) triples[i] = -1;
        raw[i] = 0.0;
        fit[i] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) n_planes[0] = 0;
}

// S[i] = 1 for a live row (finite, not yet labelled), S[n] = 0: the scan then leaves the row's number in the live list and L in S[n].  A round
// that does not run scans zeros.
__global__ __launch_bounds__(256) void plane_flag_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ labels, const int32_t *__restrict__ n_planes,
                                                         int r, int32_t *__restrict__ S) {
    const bool go = n_planes[0] == r;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += stride) {
        int f = 0;
        if (go && i < n) {
            const float *p = pts + (size_t)i * 3;
            f = finite3(p[0], p[1], p[2]) && labels[i] < 0;
        }
        S[i] = f;
    }
}

__global__ __launch_bounds__(256) void plane_compact_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ labels, const int32_t *__restrict__ n_planes,
                                                            int r, const int32_t *__restrict__ S, int32_t *__restrict__ live) {
    if (n_planes[0] != r) return;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float *p = pts + (size_t)i * 3;
        if (finite3(p[0], p[1], p[2]) && labels[i] < 0) {
            const int at = S[i];
            if (at >= 0 && at < n) live[at] = (int32_t)i;
        }
    }
}

// the round's triples (original rows; -1 for an invalid hypothesis) and the counts' start: 0, or -1 for an invalid hypothesis
__global__ __launch_bounds__(256) void plane_draw_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ live, const int32_t *__restrict__ S,
                                                         const int32_t *__restrict__ n_planes, int r, uint64_t base, int H, double dist, int32_t *__restrict__ trip,
                                                         int32_t *__restrict__ cnt) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    const int L = S[n];
    int t0 = -1, t1 = -1, t2 = -1;
    if (n_planes[0] == r && L >= 3 && L <= n) {
        const uint32_t i0 = plane_math::draw(base, (uint32_t)h, 0, (uint32_t)L), i1 = plane_math::draw(base, (uint32_t)h, 1, (uint32_t)L),
                       i2 = plane_math::draw(base, (uint32_t)h, 2, (uint32_t)L);
        if (i0 != i1 && i0 != i2 && i1 != i2) { t0 = live[i0]; t1 = live[i1]; t2 = live[i2]; }
    }
    const bool valid = make_record(pts, n, t0, t1, t2, dist).valid;
    trip[3 * h] = valid ? t0 : -1;
    trip[3 * h + 1] = valid ? t1 : -1;
    trip[3 * h + 2] = valid ? t2 : -1;
    cnt[h] = valid ? 0 : -1;
}

// roreg_plane_score: the counts' start for caller-given triples
__global__ __launch_bounds__(256) void plane_check_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ trip, int H, double dist, int32_t *__restrict__ cnt) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    cnt[h] = make_record(pts, n, trip[3 * h], trip[3 * h + 1], trip[3 * h + 2], dist).valid ? 0 : -1;
}

// live == nullptr: every row of the cloud is a candidate (dead rows fail every test); otherwise the first S[n] entries of the live list, and the
// round runs only if n_planes[0] == r.  cnt[h] starts at 0 (valid) or -1 (invalid: nothing is added).
__global__ __launch_bounds__(PS_THREADS) void plane_score_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ live, const int32_t *__restrict__ S,
                                                                 const int32_t *__restrict__ n_planes, int r, const int32_t *__restrict__ trip, int H, double dist,
                                                                 int32_t *__restrict__ cnt) {
    __shared__ double rec[PS_CHUNK][8];
    __shared__ int wsum[PS_CHUNK];
    if (live && n_planes[0] != r) return;
    const int L = live ? S[n] : n;
    if (L > n || (live && L < 3)) return;
    const int64_t tile0 = (int64_t)blockIdx.x * PS_TILE;
    if (tile0 >= L) return;                                           // (the same for every lane)
    const int tid = threadIdx.x, lane = tid & 63;
    double px[PS_PTS], py[PS_PTS], pz[PS_PTS];
#pragma unroll
    for (int q = 0; q < PS_PTS; ++q) {
        const int64_t idx = tile0 + q * PS_THREADS + tid;
        px[q] = py[q] = pz[q] = (double)NAN;                          // past the end or dead: no test passes
        if (idx < L) {
            const int row = live ? live[idx] : (int)idx;
            if (row >= 0 && row < n) {
                const float *p = pts + (size_t)row * 3;
                const float x = p[0], y = p[1], z = p[2];
                if (finite3(x, y, z)) { px[q] = (double)x; py[q] = (double)y; pz[q] = (double)z; }
            }
        }
    }
    const int chunks = (H + PS_CHUNK - 1) / PS_CHUNK;
    for (int c = blockIdx.y; c < chunks; c += gridDim.y) {
        const int h0 = c * PS_CHUNK, hc = min(PS_CHUNK, H - h0);
        __syncthreads();                                              // the previous chunk's records and counters have been read
        if (tid < PS_CHUNK) {
            double thr = (double)NAN;
            Record R{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, thr, false};
            if (tid < hc) R = make_record(pts, n, trip[3 * (h0 + tid)], trip[3 * (h0 + tid) + 1], trip[3 * (h0 + tid) + 2], dist);
            rec[tid][0] = R.nx; rec[tid][1] = R.ny; rec[tid][2] = R.nz; rec[tid][3] = R.ax; rec[tid][4] = R.ay; rec[tid][5] = R.az; rec[tid][6] = R.thr;
            wsum[tid] = 0;
        }
        __syncthreads();
        for (int j = 0; j < hc; ++j) {
            const double nx = rec[j][0], ny = rec[j][1], nz = rec[j][2], ax = rec[j][3], ay = rec[j][4], az = rec[j][5], thr = rec[j][6];
            int in = 0;
#pragma unroll
            for (int q = 0; q < PS_PTS; ++q) in += __popcll(__ballot(plane_math::inlier(nx, ny, nz, ax, ay, az, thr, px[q], py[q], pz[q])));
            if (lane == 0 && in) atomicAdd(&wsum[j], in);
        }
        __syncthreads();
        if (tid < hc && wsum[tid] > 0) atomicAdd(&cnt[h0 + tid], wsum[tid]);
    }
}

struct Cand { int cnt, h; };
// (count descending, h ascending): a total order; an invalid hypothesis (count -1) is below every valid one
__device__ __forceinline__ void take(Cand &b, int cnt, int h) {
    if (cnt > b.cnt || (cnt == b.cnt && h < b.h)) { b.cnt = cnt; b.h = h; }
}

// One workgroup.  The winner's outputs, its record for the launches behind, and n_planes[0] = r + 1; or nothing: the segmentation has ended.
__global__ __launch_bounds__(SEL_THREADS) void plane_select_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ S, int32_t *__restrict__ n_planes, int r,
                                                                   const int32_t *__restrict__ trip, const int32_t *__restrict__ cnt, int H, double dist, int min_inliers,
                                                                   int32_t *__restrict__ counts, int32_t *__restrict__ triples, double *__restrict__ raw,
                                                                   double *__restrict__ win) {
    __shared__ int wc[SEL_THREADS / 64], wh[SEL_THREADS / 64];
    const int L = S[n];
    if (n_planes[0] != r || L < 3) return;                            // (the same for every lane; only this kernel's lane 0 writes n_planes, below)
    Cand b{-1, INT_MAX};
    for (int h = threadIdx.x; h < H; h += SEL_THREADS) take(b, cnt[h], h);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) take(b, __shfl_xor(b.cnt, off), __shfl_xor(b.h, off));
    if ((threadIdx.x & 63) == 0) { wc[threadIdx.x >> 6] = b.cnt; wh[threadIdx.x >> 6] = b.h; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < SEL_THREADS / 64; ++w) take(b, wc[w], wh[w]);
    if (b.cnt < 0 || b.cnt < min_inliers || b.h >= H) return;
    const int t0 = trip[3 * b.h], t1 = trip[3 * b.h + 1], t2 = trip[3 * b.h + 2];
    const Record R = make_record(pts, n, t0, t1, t2, dist);
    if (!R.valid) return;
    counts[r] = b.cnt;
    triples[3 * r] = t0; triples[3 * r + 1] = t1; triples[3 * r + 2] = t2;
    const plane_math::Plane p{R.nx, R.ny, R.nz, 0.0};
    const double a[3] = {R.ax, R.ay, R.az};
    raw[4 * r] = R.nx; raw[4 * r + 1] = R.ny; raw[4 * r + 2] = R.nz; raw[4 * r + 3] = plane_math::offset(p, a);
    win[0] = R.nx; win[1] = R.ny; win[2] = R.nz; win[3] = R.ax; win[4] = R.ay; win[5] = R.az; win[6] = R.thr; win[7] = (double)b.cnt;
    n_planes[0] = r + 1;
}

// the wave's sum in every lane (a + b == b + a: every lane adds the same pairs), then ((w0 + w1) + w2) + w3 by the first W lanes
template <int W>
__device__ __forceinline__ void slot_write(double *acc, double (*red)[W], double *__restrict__ slot) {
#pragma unroll
    for (int q = 0; q < W; ++q) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[q] += __shfl_xor(acc[q], off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < W; ++q) red[wave][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < W) slot[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the winner's inliers get label r; the moments of (p - a) over them, one fixed slot per tile of the live list
__global__ __launch_bounds__(PS_THREADS) void plane_label_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ live, const int32_t *__restrict__ S,
                                                                 const int32_t *__restrict__ n_planes, int r, const double *__restrict__ win, int32_t *__restrict__ labels,
                                                                 double *__restrict__ mom) {
    __shared__ double red[PS_WAVES][MOM_W];
    if (n_planes[0] != r + 1) return;
    const int L = S[n];
    const int64_t tile0 = (int64_t)blockIdx.x * PS_TILE;
    if (L > n || tile0 >= L) return;
    const double nx = win[0], ny = win[1], nz = win[2], ax = win[3], ay = win[4], az = win[5], thr = win[6];
    double acc[MOM_W];
#pragma unroll
    for (int q = 0; q < MOM_W; ++q) acc[q] = 0.0;
#pragma unroll
    for (int q = 0; q < PS_PTS; ++q) {
        const int64_t idx = tile0 + q * PS_THREADS + threadIdx.x;
        if (idx >= L) continue;
        const int row = live[idx];
        if (row < 0 || row >= n) continue;
        const float *p = pts + (size_t)row * 3;
        const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
        if (!plane_math::inlier(nx, ny, nz, ax, ay, az, thr, x, y, z)) continue;
        labels[row] = r;
        const double dx = x - ax, dy = y - ay, dz = z - az;
        acc[0] += 1.0; acc[1] += dx; acc[2] += dy; acc[3] += dz;
        acc[4] += dx * dx; acc[5] += dx * dy; acc[6] += dx * dz; acc[7] += dy * dy; acc[8] += dy * dz; acc[9] += dz * dz;
    }
    slot_write<MOM_W>(acc, red, mom + (size_t)blockIdx.x * MOM_W);
}

// One workgroup: the slots in ascending order, the covariance about the centroid, the eigenvector of its smallest eigenvalue (icp_math::jacobi3),
// signed like the raw normal.  fitrec = (unit normal, centroid) for the distance pass.
__global__ __launch_bounds__(64) void plane_fit_kernel(int n, const int32_t *__restrict__ S, const int32_t *__restrict__ n_planes, int r, const double *__restrict__ win,
                                                       const double *__restrict__ mom, double *__restrict__ fit, double *__restrict__ fitrec) {
    __shared__ double M[MOM_W];
    if (n_planes[0] != r + 1) return;
    const int L = S[n];
    const int slots = (int)(((int64_t)L + PS_TILE - 1) / PS_TILE);
    if (threadIdx.x < MOM_W) {
        double s = 0.0;
        for (int i = 0; i < slots; ++i) s += mom[(size_t)i * MOM_W + threadIdx.x];
        M[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double c = M[0];
    const double mx = M[1] / c, my = M[2] / c, mz = M[3] / c;
    const double C6[6] = {M[4] / c - mx * mx, M[5] / c - mx * my, M[6] / c - mx * mz, M[7] / c - my * my, M[8] / c - my * mz, M[9] / c - mz * mz};
    double lam[3], V[9];
    icp_math::jacobi3(C6, lam, V);
    const int imin = (lam[0] <= lam[1] && lam[0] <= lam[2]) ? 0 : (lam[1] <= lam[2] ? 1 : 2);
    double fx = imin == 0 ? V[0] : (imin == 1 ? V[1] : V[2]);
    double fy = imin == 0 ? V[3] : (imin == 1 ? V[4] : V[5]);
    double fz = imin == 0 ? V[6] : (imin == 1 ? V[7] : V[8]);
    const double nn = sqrt((fx * fx + fy * fy) + fz * fz);
    fx /= nn; fy /= nn; fz /= nn;
    if ((fx * win[0] + fy * win[1]) + fz * win[2] < 0.0) { fx = -fx; fy = -fy; fz = -fz; }
    const double cx = win[3] + mx, cy = win[4] + my, cz = win[5] + mz;
    fit[4 * r] = fx; fit[4 * r + 1] = fy; fit[4 * r + 2] = fz; fit[4 * r + 3] = -((fx * cx + fy * cy) + fz * cz);
    fitrec[0] = fx; fitrec[1] = fy; fitrec[2] = fz; fitrec[3] = cx; fitrec[4] = cy; fitrec[5] = cz;
}

// the squared distances of plane r's rows to the fit, through the same slots
__global__ __launch_bounds__(PS_THREADS) void plane_dist_kernel(const float *__restrict__ pts, int n, const int32_t *__restrict__ live, const int32_t *__restrict__ S,
                                                                const int32_t *__restrict__ n_planes, int r, const double *__restrict__ fitrec,
                                                                const int32_t *__restrict__ labels, double *__restrict__ dsl) {
    __shared__ double red[PS_WAVES][1];
    if (n_planes[0] != r + 1) return;
    const int L = S[n];
    const int64_t tile0 = (int64_t)blockIdx.x * PS_TILE;
    if (L > n || tile0 >= L) return;
    const double fx = fitrec[0], fy = fitrec[1], fz = fitrec[2], cx = fitrec[3], cy = fitrec[4], cz = fitrec[5];
    double acc[1] = {0.0};
#pragma unroll
    for (int q = 0; q < PS_PTS; ++q) {
        const int64_t idx = tile0 + q * PS_THREADS + threadIdx.x;
        if (idx >= L) continue;
        const int row = live[idx];
        if (row < 0 || row >= n || labels[row] != r) continue;
        const float *p = pts + (size_t)row * 3;
        const double d = (fx * ((double)p[0] - cx) + fy * ((double)p[1] - cy)) + fz * ((double)p[2] - cz);
        acc[0] += d * d;
    }
    slot_write<1>(acc, red, dsl + blockIdx.x);
}

__global__ __launch_bounds__(64) void plane_rms_kernel(int n, const int32_t *__restrict__ S, const int32_t *__restrict__ n_planes, int r, const double *__restrict__ win,
                                                       const double *__restrict__ dsl, double *__restrict__ rms) {
    if (n_planes[0] != r + 1 || threadIdx.x != 0) return;
    const int slots = (int)(((int64_t)S[n] + PS_TILE - 1) / PS_TILE);
    double s = 0.0;
    for (int i = 0; i < slots; ++i) s += dsl[i];
    rms[r] = sqrt(s / win[7]);
}

void launch_scan(int32_t *S, int64_t m, int32_t *bsum, hipStream_t s) {
    const int64_t nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
    hipLaunchKernelGGL(icp_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const int32_t *)S, m, bsum);
    hipLaunchKernelGGL(icp_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, (int)nb);
    hipLaunchKernelGGL(icp_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, S, m, (const int32_t *)bsum);
}

int tiles_of(int n) { return (int)(((int64_t)n + PS_TILE - 1) / PS_TILE); }

dim3 score_grid(int n, int H) {
    const int tiles = std::max(tiles_of(n), 1), chunks = (H + PS_CHUNK - 1) / PS_CHUNK;
    return dim3((unsigned)tiles, (unsigned)std::min(chunks, std::max(1, PS_TARGET_BLOCKS / tiles)));
}

struct Layout {
    size_t S, bsum, live, trip, cnt, win, fitrec, mom, dsl, bytes;
};

Layout layout(int n, int H) {
    Layout L;
    size_t o = 0;
    const size_t m = (size_t)n + 1, nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK, slots = (size_t)std::max(tiles_of(n), 1);
    L.S = o; o += align_up(m * 4, 256);
    L.bsum = o; o += align_up(nb * 4, 256);
    L.live = o; o += align_up(std::max<size_t>((size_t)n, 1) * 4, 256);
    L.trip = o; o += align_up((size_t)H * 12, 256);
    L.cnt = o; o += align_up((size_t)H * 4, 256);
    L.win = o; o += 256;
    L.fitrec = o; o += 256;
    L.mom = o; o += align_up(slots * MOM_W * 8, 256);
    L.dsl = o; o += align_up(slots * 8, 256);
    L.bytes = o;
    return L;
}

bool sizes_ok(int n, int H) { return n >= 0 && n <= PLANE_MAX_N && H >= 1 && H <= ROREG_PLANE_MAX_HYP; }

}  // namespace

extern "C" size_t roreg_plane_workspace(int n, int n_hyp) {
    if (!sizes_ok(n, n_hyp)) return 0;
    return layout(n, n_hyp).bytes;
}

extern "C" int roreg_plane_segment(const float *points, int n, double dist, int n_hyp, int max_planes, int min_inliers, uint64_t seed, int32_t *labels,
                                   int32_t *n_planes, int32_t *counts, int32_t *triples, double *raw, double *fit, double *rms, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(sizes_ok(n, n_hyp) && max_planes >= 0 && max_planes <= ROREG_PLANE_MAX_PLANES && min_inliers >= 3, "roreg_plane_segment: bad sizes");
    ROREG_REQUIRE(dist > 0.0 && std::isfinite(dist), "roreg_plane_segment: dist must be positive and finite");
    ROREG_REQUIRE(n_planes && (n == 0 || (points && labels)) && (max_planes == 0 || (counts && triples && raw && fit && rms)), "roreg_plane_segment: bad arguments");
    hipStream_t s = roreg::as_stream(stream);
    const int flat = (int)std::min<int64_t>(std::max<int64_t>(((int64_t)std::max(n + 1, 4 * max_planes) + 255) / 256, 1), FLAT_BLOCKS);
    hipLaunchKernelGGL(plane_init_kernel, dim3((unsigned)flat), dim3(256), 0, s, n, max_planes, labels, n_planes, counts, triples, raw, fit, rms);
    ROREG_CHECK_LAUNCH("roreg_plane_segment");
    if (n < 3 || max_planes == 0) return 0;
    const Layout L = layout(n, n_hyp);
    ROREG_REQUIRE(workspace && workspace_bytes >= L.bytes, "roreg_plane_segment: workspace too small");
    char *w = reinterpret_cast<char *>(workspace);
    int32_t *S = reinterpret_cast<int32_t *>(w + L.S), *bsum = reinterpret_cast<int32_t *>(w + L.bsum), *live = reinterpret_cast<int32_t *>(w + L.live);
    int32_t *trip = reinterpret_cast<int32_t *>(w + L.trip), *cnt = reinterpret_cast<int32_t *>(w + L.cnt);
    double *win = reinterpret_cast<double *>(w + L.win), *fitrec = reinterpret_cast<double *>(w + L.fitrec), *mom = reinterpret_cast<double *>(w + L.mom),
           *dsl = reinterpret_cast<double *>(w + L.dsl);
    const dim3 tiles((unsigned)tiles_of(n)), hyp_blocks((unsigned)((n_hyp + 255) / 256)), sg = score_grid(n, n_hyp);
    for (int r = 0; r < max_planes; ++r) {
        hipLaunchKernelGGL(plane_flag_kernel, dim3((unsigned)flat), dim3(256), 0, s, points, n, (const int32_t *)labels, (const int32_t *)n_planes, r, S);
        launch_scan(S, (int64_t)n + 1, bsum, s);
        hipLaunchKernelGGL(plane_compact_kernel, dim3((unsigned)flat), dim3(256), 0, s, points, n, (const int32_t *)labels, (const int32_t *)n_planes, r,
                           (const int32_t *)S, live);
        hipLaunchKernelGGL(plane_draw_kernel, hyp_blocks, dim3(256), 0, s, points, n, (const int32_t *)live, (const int32_t *)S, (const int32_t *)n_planes, r,
                           plane_math::round_base(seed, r), n_hyp, dist, trip, cnt);
        hipLaunchKernelGGL(plane_score_kernel, sg, dim3(PS_THREADS), 0, s, points, n, (const int32_t *)live, (const int32_t *)S, (const int32_t *)n_planes, r,
                           (const int32_t *)trip, n_hyp, dist, cnt);
        hipLaunchKernelGGL(plane_select_kernel, dim3(1), dim3(SEL_THREADS), 0, s, points, n, (const int32_t *)S, n_planes, r, (const int32_t *)trip,
                           (const int32_t *)cnt, n_hyp, dist, min_inliers, counts, triples, raw, win);
        hipLaunchKernelGGL(plane_label_kernel, tiles, dim3(PS_THREADS), 0, s, points, n, (const int32_t *)live, (const int32_t *)S, (const int32_t *)n_planes, r,
                           (const double *)win, labels, mom);
        hipLaunchKernelGGL(plane_fit_kernel, dim3(1), dim3(64), 0, s, n, (const int32_t *)S, (const int32_t *)n_planes, r, (const double *)win, (const double *)mom,
                           fit, fitrec);
        hipLaunchKernelGGL(plane_dist_kernel, tiles, dim3(PS_THREADS), 0, s, points, n, (const int32_t *)live, (const int32_t *)S, (const int32_t *)n_planes, r,
                           (const double *)fitrec, (const int32_t *)labels, dsl);
        hipLaunchKernelGGL(plane_rms_kernel, dim3(1), dim3(64), 0, s, n, (const int32_t *)S, (const int32_t *)n_planes, r, (const double *)win, (const double *)dsl,
                           rms);
    }
    ROREG_CHECK_LAUNCH("roreg_plane_segment");
    return 0;
}

extern "C" int roreg_plane_score(const float *points, int n, const int32_t *triples, int n_hyp, double dist, int32_t *counts_out, void *stream) {
    ROREG_REQUIRE(n >= 0 && n <= PLANE_MAX_N && n_hyp >= 0 && n_hyp <= ROREG_PLANE_MAX_HYP, "roreg_plane_score: bad sizes");
    ROREG_REQUIRE(dist > 0.0 && std::isfinite(dist), "roreg_plane_score: dist must be positive and finite");
    if (n_hyp == 0) return 0;
    ROREG_REQUIRE(triples && counts_out && (points || n == 0), "roreg_plane_score: bad arguments");
    hipStream_t s = roreg::as_stream(stream);
    hipLaunchKernelGGL(plane_check_kernel, dim3((unsigned)((n_hyp + 255) / 256)), dim3(256), 0, s, points, n, triples, n_hyp, dist, counts_out);
    if (n > 0)
        hipLaunchKernelGGL(plane_score_kernel, score_grid(n, n_hyp), dim3(PS_THREADS), 0, s, points, n, (const int32_t *)nullptr, (const int32_t *)nullptr,
                           (const int32_t *)nullptr, 0, triples, n_hyp, dist, counts_out);
    ROREG_CHECK_LAUNCH("roreg_plane_score");
    return 0;
}
