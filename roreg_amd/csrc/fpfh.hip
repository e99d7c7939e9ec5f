// FPFH descriptors of a dense cloud ("v6n"): 33 numbers per point from the point's neighbours and their normals, all
// float64 arithmetic on float32 coordinates in the operation order of csrc/fpfh_math.h.  No reference counterpart: the reference's
// descriptors are learned; tests/_fpfh_oracle.py is the numpy restatement.
//
// Three entries, every public table in ORIGINAL row order, every kernel one lane per record of the cloud's grid in CELL order (csrc/icp_grid.h:
// a wave's lanes walk the same cells, so the records, normals and histograms of the neighbours are shared cache lines):
//   orient   : n_i <- -n_i iff n_i . (c - x_i) < 0.
//   spfh     : a permutation pass copies the oriented normals into cell order (the walk then reads a neighbour's normal where it reads its
//              record); the walk bins the pair feature of every neighbour within the radius.  A lane's 33 counters are indexed at run time:
//              they live in LDS as [bin][lane], the lane the fast axis, so that a wave's 64 increments fall into 64 different banks whatever
//              the bins are (33 x 256 x 4 bytes = 33 KB per workgroup, four workgroups per CU).  Counters are 32 bits wide: a count is at most
//              n - 1 < 2^31.
//   features : a scaling pass writes S = count (100 / m) and m in cell order (264 bytes per record: what the walk streams from L2); the walk
//              adds S_j / d2 into 33 accumulators held in registers (every index a compile-time constant), then normalises each third.
// The counts are integers and do not depend on the order of the walk: any grid of the cloud gives the same bytes.  The float64 sums of the
// second pass do (ascending cell, ascending row inside a cell).
#include "common.h"
#include "fpfh_math.h"
#include "icp_grid.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int FPFH_THREADS = 256;
constexpr int FPFH_W = fpfh_math::WIDTH;
constexpr int FPFH_MAX_N = 1 << 30;

__device__ __forceinline__ bool normal_valid(const double4 &v) { return v.x != 0.0 || v.y != 0.0 || v.z != 0.0; }

// record i of the grid and its original row -> false: past the cloud, or a row the cloud does not have (a damaged grid writes nothing)
__device__ __forceinline__ bool own_record(const float4 *__restrict__ rec, int n, int i, float4 &p, int &row) {
    if (i >= n) return false;
    p = rec[i];
    row = __float_as_int(p.w);
    return row >= 0 && row < n;
}

__global__ __launch_bounds__(FPFH_THREADS) void fpfh_orient_kernel(const void *__restrict__ grid, int n, const double4 *__restrict__ normals, double cx, double cy,
                                                                   double cz, double4 *__restrict__ out) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    float4 p; int row;
    if (!own_record(grid_recs(grid), n, blockIdx.x * FPFH_THREADS + threadIdx.x, p, row)) return;
    double4 v = normals[row];
    const double nrm[3] = {v.x, v.y, v.z}, x[3] = {(double)p.x, (double)p.y, (double)p.z}, c[3] = {cx, cy, cz};
    if (fpfh_math::orient_flip(nrm, x, c)) { v.x = -v.x; v.y = -v.y; v.z = -v.z; }
    out[row] = v;
}

// oriented normals, original row order -> cell order; w = 1 for a valid normal, 0 for the zero vector
__global__ __launch_bounds__(FPFH_THREADS) void fpfh_permute_kernel(const void *__restrict__ grid, int n, const double4 *__restrict__ normals, double4 *__restrict__ ncell) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const int i = blockIdx.x * FPFH_THREADS + threadIdx.x;
    if (i >= n) return;
    float4 p; int row;
    double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
    if (own_record(grid_recs(grid), n, i, p, row)) { v = normals[row]; v.w = normal_valid(v) ? 1.0 : 0.0; }
    ncell[i] = v;
}

__global__ __launch_bounds__(FPFH_THREADS) void fpfh_spfh_kernel(const void *__restrict__ grid, int n, const double4 *__restrict__ ncell, double thr2, double reach,
                                                                 int32_t *__restrict__ counts, int32_t *__restrict__ m_out) {
    __shared__ uint32_t cnt[FPFH_W][FPFH_THREADS];          // [bin][lane]: bank = lane % 64 whatever the bin
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    const int tid = threadIdx.x, i = blockIdx.x * FPFH_THREADS + tid;
    float4 p; int row;
    if (!own_record(rec, n, i, p, row)) return;          // (no barrier below: a lane touches its own column of cnt alone)
#pragma unroll
    for (int b = 0; b < FPFH_W; ++b) cnt[b][tid] = 0;
    int m = 0;
    const double4 own = ncell[i];
    if (own.w != 0.0) {
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        const double ni[3] = {own.x, own.y, own.z};
        // (the walk hands over the record where it lies: its place in the table is the neighbour's place in every cell-ordered table)
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 &q) {
            const int k = (int)(&q - rec);
            const double dp[3] = {(double)q.x - px, (double)q.y - py, (double)q.z - pz};        // exact: both are float32 values
            const double d2 = fpfh_math::dot3(dp[0], dp[1], dp[2], dp[0], dp[1], dp[2]);
            if (k == i || !(d2 <= thr2) || !(d2 > 0.0)) return;
            const double4 nb = ncell[k];
            if (nb.w == 0.0) return;
            const double nj[3] = {nb.x, nb.y, nb.z};
            fpfh_math::Pair f;
            if (!fpfh_math::pair_feature(dp, d2, ni, nj, f)) return;
            ++m;
            cnt[fpfh_math::bin_angle(f.y, f.x)][tid] += 1;
            cnt[fpfh_math::BINS + fpfh_math::bin_linear(f.f2)][tid] += 1;
            cnt[2 * fpfh_math::BINS + fpfh_math::bin_linear(f.f3)][tid] += 1;
        });
    }
    int32_t *o = counts + (size_t)row * FPFH_W;
#pragma unroll
    for (int b = 0; b < FPFH_W; ++b) o[b] = (int32_t)cnt[b][tid];
    m_out[row] = m;
}

// S = count (100 / m) (0 where m <= 0) and m, original row order -> cell order
__global__ __launch_bounds__(FPFH_THREADS) void fpfh_scale_kernel(const void *__restrict__ grid, int n, const int32_t *__restrict__ counts, const int32_t *__restrict__ m,
                                                                  double *__restrict__ scell, int32_t *__restrict__ mcell) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const int i = blockIdx.x * FPFH_THREADS + threadIdx.x;
    if (i >= n) return;
    float4 p; int row;
    const bool ok = own_record(grid_recs(grid), n, i, p, row);
    const int mi = ok ? m[row] : 0;
    const double scale = mi > 0 ? 100.0 / (double)mi : 0.0;
    for (int b = 0; b < FPFH_W; ++b) scell[(size_t)i * FPFH_W + b] = mi > 0 ? (double)counts[(size_t)row * FPFH_W + b] * scale : 0.0;
    mcell[i] = mi;
}

__global__ __launch_bounds__(FPFH_THREADS) void fpfh_features_kernel(const void *__restrict__ grid, int n, const double *__restrict__ scell,
                                                                     const int32_t *__restrict__ mcell, double thr2, double reach, float *__restrict__ out,
                                                                     uint8_t *__restrict__ valid_out) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    const int i = blockIdx.x * FPFH_THREADS + threadIdx.x;
    float4 p; int row;
    if (!own_record(rec, n, i, p, row)) return;
    const bool valid = mcell[i] > 0;
    float *o = out + (size_t)row * FPFH_W;
    valid_out[row] = valid ? 1 : 0;
    if (!valid) {
#pragma unroll
        for (int b = 0; b < FPFH_W; ++b) o[b] = 0.0f;
        return;
    }
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    double W[FPFH_W];
#pragma unroll
    for (int b = 0; b < FPFH_W; ++b) W[b] = 0.0;
    walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 &q) {
        const int k = (int)(&q - rec);
        const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
        const double d2 = fpfh_math::dot3(dx, dy, dz, dx, dy, dz);
        if (k == i || !(d2 <= thr2) || !(d2 > 0.0) || mcell[k] <= 0) return;
        const double *__restrict__ s = scell + (size_t)k * FPFH_W;
#pragma unroll
        for (int b = 0; b < FPFH_W; ++b) W[b] += s[b] / d2;
    });
    const double *__restrict__ own = scell + (size_t)i * FPFH_W;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        double sg = 0.0;
#pragma unroll
        for (int b = 0; b < fpfh_math::BINS; ++b) sg += W[t * fpfh_math::BINS + b];
#pragma unroll
        for (int b = 0; b < fpfh_math::BINS; ++b) {
            const int q = t * fpfh_math::BINS + b;
            o[q] = (float)((sg > 0.0 ? (100.0 * W[q]) / sg : 0.0) + own[q]);
        }
    }
}

bool fpfh_radius_ok(double radius) { return radius > 0.0 && std::isfinite(radius); }
int fpfh_blocks(int n) { return (n + FPFH_THREADS - 1) / FPFH_THREADS; }

}  // namespace

extern "C" size_t roreg_fpfh_spfh_workspace(int n) { return n < 0 || n > FPFH_MAX_N ? 0 : align_up((size_t)n * sizeof(double4), 256) + 256; }

extern "C" size_t roreg_fpfh_features_workspace(int n) {
    return n < 0 || n > FPFH_MAX_N ? 0 : align_up((size_t)n * FPFH_W * sizeof(double), 256) + align_up((size_t)n * sizeof(int32_t), 256) + 256;
}

extern "C" int roreg_fpfh_orient(const void *grid, int n, const double *normals, const double *viewpoint, double *out, void *stream) {
    if (n == 0) return 0;
    ROREG_REQUIRE(grid && n > 0 && n <= FPFH_MAX_N && normals && viewpoint && out, "roreg_fpfh_orient: bad arguments");
    ROREG_REQUIRE(((uintptr_t)normals % 32) == 0 && ((uintptr_t)out % 32) == 0, "roreg_fpfh_orient: the normal tables must be 32-byte aligned");
    ROREG_REQUIRE(std::isfinite(viewpoint[0]) && std::isfinite(viewpoint[1]) && std::isfinite(viewpoint[2]), "roreg_fpfh_orient: the viewpoint must be finite");
    hipLaunchKernelGGL(fpfh_orient_kernel, dim3(fpfh_blocks(n)), dim3(FPFH_THREADS), 0, roreg::as_stream(stream), grid, n,
                       reinterpret_cast<const double4 *>(normals), viewpoint[0], viewpoint[1], viewpoint[2], reinterpret_cast<double4 *>(out));
    ROREG_CHECK_LAUNCH("roreg_fpfh_orient");
    return 0;
}

extern "C" int roreg_fpfh_spfh(const void *grid, int n, const double *oriented, double radius, int32_t *counts_out, int32_t *m_out, void *workspace,
                               size_t workspace_bytes, void *stream) {
    if (n == 0) return 0;
    ROREG_REQUIRE(grid && n > 0 && n <= FPFH_MAX_N && oriented && counts_out && m_out && workspace, "roreg_fpfh_spfh: bad arguments");
    ROREG_REQUIRE(fpfh_radius_ok(radius), "roreg_fpfh_spfh: radius must be positive and finite");
    ROREG_REQUIRE(((uintptr_t)oriented % 32) == 0 && ((uintptr_t)workspace % 32) == 0, "roreg_fpfh_spfh: the normal table and the workspace must be 32-byte aligned");
    ROREG_REQUIRE(workspace_bytes >= roreg_fpfh_spfh_workspace(n), "roreg_fpfh_spfh: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    double4 *ncell = reinterpret_cast<double4 *>(workspace);
    hipLaunchKernelGGL(fpfh_permute_kernel, dim3(fpfh_blocks(n)), dim3(FPFH_THREADS), 0, s, grid, n, reinterpret_cast<const double4 *>(oriented), ncell);
    hipLaunchKernelGGL(fpfh_spfh_kernel, dim3(fpfh_blocks(n)), dim3(FPFH_THREADS), 0, s, grid, n, (const double4 *)ncell, radius * radius,
                       radius * (1.0 + 1e-9), counts_out, m_out);
    ROREG_CHECK_LAUNCH("roreg_fpfh_spfh");
    return 0;
}

extern "C" int roreg_fpfh_features(const void *grid, int n, const int32_t *counts, const int32_t *m, double radius, float *out, uint8_t *valid_out,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    if (n == 0) return 0;
    ROREG_REQUIRE(grid && n > 0 && n <= FPFH_MAX_N && counts && m && out && valid_out && workspace, "roreg_fpfh_features: bad arguments");
    ROREG_REQUIRE(fpfh_radius_ok(radius), "roreg_fpfh_features: radius must be positive and finite");
    ROREG_REQUIRE(((uintptr_t)workspace % 8) == 0, "roreg_fpfh_features: the workspace must be 8-byte aligned");
    ROREG_REQUIRE(workspace_bytes >= roreg_fpfh_features_workspace(n), "roreg_fpfh_features: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    double *scell = reinterpret_cast<double *>(workspace);
    int32_t *mcell = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(workspace) + align_up((size_t)n * FPFH_W * sizeof(double), 256));
    hipLaunchKernelGGL(fpfh_scale_kernel, dim3(fpfh_blocks(n)), dim3(FPFH_THREADS), 0, s, grid, n, counts, m, scell, mcell);
    hipLaunchKernelGGL(fpfh_features_kernel, dim3(fpfh_blocks(n)), dim3(FPFH_THREADS), 0, s, grid, n, (const double *)scell, (const int32_t *)mcell,
                       radius * radius, radius * (1.0 + 1e-9), out, valid_out);
    ROREG_CHECK_LAUNCH("roreg_fpfh_features");
    return 0;
}
