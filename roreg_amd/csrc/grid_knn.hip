// The k nearest neighbours within a radius of every query, from a cloud's grid ("v6q").  No reference counterpart;
// tests/_grid_knn_oracle.py is the numpy restatement.  Coordinates are float32 values widened to float64, d2 = (dx dx + dy dy) + dz dz with no
// FMA, a row is a candidate iff it is not the query's excluded row and d2 <= radius^2, candidates are ordered by (d2, row): every output is a
// function of + - * / sqrt and comparisons in a stated order, so any grid of the cloud gives the same bytes.
//
// One lane per query.  Own-cloud mode: the queries are the grid's records in CELL order (csrc/icp_grid.h), so a wave's lanes walk the same
// cells; a query's results go to its original row.  Query mode: lane q takes queries[q] and writes row q.  A lane's list is indexed at run
// time, so it lives in LDS as [slot][lane], the lane the fast axis: wherever the 64 lanes of a wave stand in their lists, their accesses fall
// into distinct banks (a slot is KNN_THREADS * 8 bytes, a whole number of bank rounds).  12 bytes per entry: K = 32 x 128 lanes = 48 KiB per
// workgroup, three workgroups per CU.  The list's fill and its worst (d2, row) stay in registers (csrc/knn_list.h): once the list is full most
// candidates are rejected by two comparisons without touching LDS.
#include "common.h"
#include "icp_grid.h"
#include "knn_list.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int KNN_THREADS = 128;
constexpr int KNN_MAX_K = 32;
constexpr int KNN_MAX_N = 1 << 30;

template <int K>
struct LdsList {
    double (*d)[KNN_THREADS];
    int32_t (*r)[KNN_THREADS];
    int lane;
    __device__ __forceinline__ double d2(int s) const { return d[s][lane]; }
    __device__ __forceinline__ int row(int s) const { return r[s][lane]; }
    __device__ __forceinline__ void set(int s, double v, int j) { d[s][lane] = v; r[s][lane] = j; }
};

// K: the list's length in LDS (k rounded up to 8 / 16 / 32); OWN: the queries are the grid's own records.
template <int K, bool OWN>
__global__ __launch_bounds__(KNN_THREADS) void grid_knn_kernel(const void *__restrict__ grid, int n, int k, double thr2, double reach, const float *__restrict__ queries,
                                                               const int32_t *__restrict__ self_rows, int m, int32_t *__restrict__ idx_out,
                                                               double *__restrict__ d2_out, int32_t *__restrict__ count_out, double *__restrict__ mean_out) {
    __shared__ double ld[K][KNN_THREADS];                // [slot][lane]
    __shared__ int32_t lr[K][KNN_THREADS];
    const GridDesc g = *grid_desc(grid);
    if (g.n != n || k < 1 || k > K) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    const int tid = threadIdx.x, i = blockIdx.x * KNN_THREADS + tid;
    if (i >= m) return;                                  // (no barrier below: a lane touches its own column of the list alone)
    double px, py, pz;
    int excl, out;
    if (OWN) {
        const float4 p = rec[i];
        excl = out = __float_as_int(p.w);
        if (out < 0 || out >= n) return;                 // a row the cloud does not have: a damaged grid writes nothing
        px = (double)p.x; py = (double)p.y; pz = (double)p.z;
    } else {
        px = (double)queries[(size_t)i * 3]; py = (double)queries[(size_t)i * 3 + 1]; pz = (double)queries[(size_t)i * 3 + 2];
        excl = self_rows ? self_rows[i] : -1;
        out = i;
    }
    LdsList<K> list{ld, lr, tid};
    knn_list::State s = knn_list::empty();
    int count = 0;
    walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
        const int j = __float_as_int(q.w);
        if (j < 0 || j >= n || j == excl) return;
        const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;        // exact: both are float32 values
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (!(d2 <= thr2)) return;
        ++count;
        knn_list::offer(list, k, s, d2, j);
    });
    int32_t *oi = idx_out + (size_t)out * k;
    double *od = d2_out + (size_t)out * k;
    double sum = 0.0;
    for (int t = 0; t < k; ++t) {
        const bool held = t < s.fill;
        const double v = held ? list.d2(t) : (double)INFINITY;
        oi[t] = held ? list.row(t) : -1;
        od[t] = v;
        if (held) sum = t == 0 ? sqrt(v) : sum + sqrt(v);
    }
    count_out[out] = count;
    if (mean_out) mean_out[out] = s.fill > 0 ? sum / (double)s.fill : (double)INFINITY;
}

template <int K>
void launch(bool own, hipStream_t s, const void *grid, int n, int k, double radius, const float *queries, const int32_t *self_rows, int m, int32_t *idx_out,
            double *d2_out, int32_t *count_out, double *mean_out) {
    const dim3 blocks((m + KNN_THREADS - 1) / KNN_THREADS), threads(KNN_THREADS);
    const double thr2 = radius * radius, reach = radius * (1.0 + 1e-9);
    if (own)
        hipLaunchKernelGGL((grid_knn_kernel<K, true>), blocks, threads, 0, s, grid, n, k, thr2, reach, queries, self_rows, m, idx_out, d2_out, count_out, mean_out);
    else
        hipLaunchKernelGGL((grid_knn_kernel<K, false>), blocks, threads, 0, s, grid, n, k, thr2, reach, queries, self_rows, m, idx_out, d2_out, count_out, mean_out);
}

}  // namespace

extern "C" int roreg_grid_knn(const void *grid, int n, int k, double radius, const float *queries, const int32_t *self_rows, int m, int32_t *idx_out,
                              double *d2_out, int32_t *count_out, double *mean_dist_out, void *stream) {
    ROREG_REQUIRE(k >= 1 && k <= KNN_MAX_K, "roreg_grid_knn: k must be in 1..32");
    ROREG_REQUIRE(radius > 0.0 && std::isfinite(radius), "roreg_grid_knn: radius must be positive and finite");
    ROREG_REQUIRE(queries || !self_rows, "roreg_grid_knn: self_rows without queries");
    ROREG_REQUIRE(n >= 0 && n <= KNN_MAX_N && m >= 0 && m <= KNN_MAX_N && (queries || m == n), "roreg_grid_knn: bad sizes (own-cloud mode: m == n)");
    if (m == 0) return 0;
    ROREG_REQUIRE(grid && n > 0 && idx_out && d2_out && count_out, "roreg_grid_knn: bad arguments");
    hipStream_t s = roreg::as_stream(stream);
    const bool own = queries == nullptr;
    if (k <= 8) launch<8>(own, s, grid, n, k, radius, queries, self_rows, m, idx_out, d2_out, count_out, mean_dist_out);
    else if (k <= 16) launch<16>(own, s, grid, n, k, radius, queries, self_rows, m, idx_out, d2_out, count_out, mean_dist_out);
    else launch<32>(own, s, grid, n, k, radius, queries, self_rows, m, idx_out, d2_out, count_out, mean_dist_out);
    ROREG_CHECK_LAUNCH("roreg_grid_knn");
    return 0;
}
