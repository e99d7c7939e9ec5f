// Dense ICP of registered pairs, point-to-point ("v6c"), point-to-plane ("v6d") and plane-to-plane ("v6i"), and the read-only pair evaluation
// ("v6g"): all float64 arithmetic on float32 coordinates (include/roreg_hip.h).  No reference counterpart: the reference ends at the keypoint
// transform; tests/_icp_oracle.py, tests/_icp_plane_oracle.py, tests/_icp_gicp_oracle.py and tests/_dense_eval_oracle.py are the numpy restatements.
//
// Grid (once per cloud and cell edge): a uniform 3-D table over the bounding box padded by one cell; counting sort = cell id, integer
// histogram, exclusive scan, fill, and then every cell's records put in ascending original row, so that nothing downstream depends on the
// order the fill's atomics were served in.  Records are 16 bytes (x, y, z, original row as bits): one dwordx4 load per candidate.
//
// Iteration (icp_run: one driver for every method; three launches, no host synchronisation, max_iter times):
//   search : one source point per lane (four per thread, 1024 per workgroup), source points in THEIR OWN cell order so that a wave's
//            queries walk neighbouring target cells; the cells that can hold a point within max_dist are a box of at most 3 (rarely 4)
//            cells per axis, x-contiguous cells are one run of records.  First-pass sums (n, sum q, sum p, sum d2) by wave reduction into
//            the workgroup's fixed slot.
//   second pass over the stored assignments, into fixed slots again --
//     point (icp_cov_kernel)  : centroids rebuilt from the pair's slots in slot order, the 9 entries of H;
//     plane (icp_plane_kernel): the 29 words of the 6x6 normal equations against the target's normals;
//     gicp  (icp_gicp_kernel) : the same 29 words, every residual weighted by M = (C_q + R C_p R^T)^-1 from both clouds' normals;
//     plane and gicp under a robust loss ("v6p": the same two kernels over the robust task records): A and b with every correspondence
//                               weighted by its residual (icp_math.h robust_weight); count and squared-residual sum unweighted;
//   solve  : one workgroup per pair reduces the slots in slot order; lane 0 solves (point: 3x3 one-sided Jacobi SVD with the determinant
//            fix; plane and gicp: 6x6 Jacobi, exp of the rotation part) and hands (R+, t+, support) to the one tail every method shares
//            (solve_tail): step sizes, convergence test, the pair's state and `done` word, the outputs.
// init, search, export and the 6x6 solve are templates over the task record (IcpTask, IcpPlaneTask, IcpGicpTask: the fields they read are in
// each), so every entry's table is read where it lies.  The work list is ragged (pair, chunk) rows; a slot belongs to (pair, chunk) alone, so a pair's
// sums -- and its result -- are the same bits in every batch.  No floating-point atomics anywhere.  What fixes the bits is defined once:
// work_row (which workgroups run), transform_point, slot_write (wave sums, then ((w0 + w1) + w2) + w3), slot_sum (ascending slot).
#include "common.h"
#include "icp_grid.h"
#include "icp_math.h"
#include "primitives.h"
#include <cmath>
#include <cstddef>

#pragma clang fp contract(off)

namespace {

constexpr int ICP_CHUNK = 1024;        // source points per workgroup and per slot
constexpr int ICP_THREADS = 256;
constexpr int ICP_PER_THREAD = ICP_CHUNK / ICP_THREADS;
constexpr int SUM_W = 8;               // first-pass slot: n, sum q (3), sum p (3), sum d2
constexpr int COV_W = 9;               // second-pass slot, point method: H
constexpr int PLANE_W = 29;            // second-pass slot, plane method: n_valid, the 21 upper entries of A = sum J J^T, the 6 of b = -sum J e, sum e^2
                                       // (gicp, the same layout: n, A = sum J^T M J, b = -sum J^T M d, sum d^T M d)
constexpr int PLANE_STATS_W = 32;      // plane and gicp stats_out row: n_valid, c (3), A upper (21), b (6), sum e^2
constexpr int EVAL_W = 12;             // evaluation slot: n, sum x (3), the 6 upper entries of sum x x^T, sum d2 and its error word
constexpr int64_t MAX_CELLS = (int64_t)1 << 24;

// The task records.  init, search and export read tgt, src, T0, n_src and slot0 of any.  The two robust records ("v6p") are the plane and
// gicp records followed by the loss's scale and kind; `robust` (a static member: no byte of the record) tells the second pass which it has.
struct IcpTask { const void *tgt, *src; const double *T0; int32_t n_src, slot0; };
struct IcpPlaneTask {
    static constexpr bool robust = false;
    const void *tgt, *src; const double *normals; const double *T0; int32_t n_src, slot0;
};
struct IcpGicpTask {
    static constexpr bool robust = false;
    const void *tgt, *src; const double *tgt_normals, *src_normals; const double *T0; double epsilon; int32_t n_src, slot0;
};
struct IcpPlaneRobustTask {
    static constexpr bool robust = true;
    const void *tgt, *src; const double *normals; const double *T0; int32_t n_src, slot0; double scale; int32_t loss, reserved;
};
struct IcpGicpRobustTask {
    static constexpr bool robust = true;
    const void *tgt, *src; const double *tgt_normals, *src_normals; const double *T0; double epsilon; int32_t n_src, slot0; double scale; int32_t loss, reserved;
};
static_assert(sizeof(IcpTask) == sizeof(roreg_icp_task), "IcpTask mirrors roreg_icp_task");
static_assert(sizeof(IcpPlaneTask) == sizeof(roreg_icp_plane_task), "IcpPlaneTask mirrors roreg_icp_plane_task");
static_assert(sizeof(IcpGicpTask) == sizeof(roreg_icp_gicp_task) && sizeof(IcpGicpTask) == 56, "IcpGicpTask mirrors roreg_icp_gicp_task");
static_assert(sizeof(IcpPlaneRobustTask) == sizeof(roreg_icp_plane_robust_task) && sizeof(IcpPlaneRobustTask) == 56 &&
              offsetof(IcpPlaneRobustTask, scale) == sizeof(IcpPlaneTask), "IcpPlaneRobustTask mirrors roreg_icp_plane_robust_task");
static_assert(sizeof(IcpGicpRobustTask) == sizeof(roreg_icp_gicp_robust_task) && sizeof(IcpGicpRobustTask) == 72 &&
              offsetof(IcpGicpRobustTask, scale) == sizeof(IcpGicpTask), "IcpGicpRobustTask mirrors roreg_icp_gicp_robust_task");
static_assert(icp_math::LOSS_HUBER == ROREG_ICP_LOSS_HUBER && icp_math::LOSS_CAUCHY == ROREG_ICP_LOSS_CAUCHY && icp_math::LOSS_GM == ROREG_ICP_LOSS_GM &&
              icp_math::LOSS_TUKEY == ROREG_ICP_LOSS_TUKEY, "icp_math's loss kinds are roreg_icp_loss's");

struct PairState {
    double R[9], t[3];
    double rmse;
    int32_t done, iters, inliers, status;
    double pad_;
};
static_assert(sizeof(PairState) == 128, "PairState is 128 bytes");

enum { ST_CONVERGED = 0, ST_MAX_ITER = 1, ST_NO_SUPPORT = 2, ST_NONFINITE = 3 };

struct IcpOut { double *T; int32_t *iters, *inliers; double *rmse; int32_t *status; };          // the five per-pair outputs of a batch entry

// ---- grid build -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void icp_hist_kernel(const float *__restrict__ pts, GridDesc d, int32_t *__restrict__ S, GridDesc *__restrict__ hdr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *hdr = d;
    if (i >= d.n) return;
    atomicAdd(&S[cell_of(d, 1.0 / d.edge, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2])], 1);
}

__global__ __launch_bounds__(256) void icp_header_kernel(GridDesc d, GridDesc *__restrict__ hdr) { *hdr = d; }

#include "scan.h"          // icp_scan_{sums,top,apply}_kernel: the three-launch exclusive scan, shared with csrc/voxel.hip

// S[c] is cell c's cursor: afterwards it is the cell's END, i.e. the word before S holds the table of starts (starts = S - 1, starts[0] = 0)
__global__ __launch_bounds__(256) void icp_fill_kernel(const float *__restrict__ pts, GridDesc d, int32_t *__restrict__ S, float4 *__restrict__ tmp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    const int pos = atomicAdd(&S[cell_of(d, 1.0 / d.edge, x, y, z)], 1);
    if (pos >= 0 && pos < d.n) tmp[pos] = make_float4(x, y, z, __int_as_float(i));
}

// canonical order inside a cell: a record's place is the number of records of its cell with a lower original row
__global__ __launch_bounds__(256) void icp_rank_kernel(const float4 *__restrict__ tmp, GridDesc d, const int32_t *__restrict__ starts, float4 *__restrict__ recs) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d.n) return;
    const float4 r = tmp[j];
    const int c = cell_of(d, 1.0 / d.edge, r.x, r.y, r.z);
    const int b = starts[c], e = starts[c + 1];
    const int row = __float_as_int(r.w);
    int rank = 0;
    for (int k = b; k < e; ++k) rank += __float_as_int(tmp[k].w) < row;
    if (b + rank < d.n) recs[b + rank] = r;
}

// ---- iteration ------------------------------------------------------------------------------------------------------------------------
// The v6c search of one query (tx, ty, tz): the nearest record of the target grid by d2 = (dx dx + dy dy) + dz dz, an exact tie going to the
// lowest original row -> (its d2, its original row, its record; record -1: no cell in reach).  Shared by the iteration's search and the pair
// evaluation.
struct Nearest { double d2; int row, k; };
__device__ __forceinline__ Nearest nearest_record(const GridDesc &g, const float4 *__restrict__ trec, const int32_t *__restrict__ tst, double inv, double tx,
                                                  double ty, double tz, double reach) {
    // every target point within max_dist lies in cells [lo, hi] per axis: `reach` exceeds max_dist by more than the roundings of d2
    const double lx = cell_coord(tx - reach, g.origin[0], inv), hx = cell_coord(tx + reach, g.origin[0], inv);
    const double ly = cell_coord(ty - reach, g.origin[1], inv), hy = cell_coord(ty + reach, g.origin[1], inv);
    const double lz = cell_coord(tz - reach, g.origin[2], inv), hz = cell_coord(tz + reach, g.origin[2], inv);
    double best = __builtin_inf();
    int brow = 0x7fffffff, bk = -1;
    // (written so that a NaN or infinite coordinate selects no cell)
    if (hx >= 0.0 && lx <= (double)(g.dims[0] - 1) && hy >= 0.0 && ly <= (double)(g.dims[1] - 1) && hz >= 0.0 && lz <= (double)(g.dims[2] - 1)) {
        const int x0 = cell_clamp(lx, g.dims[0]), x1 = cell_clamp(hx, g.dims[0]);
        const int y0 = cell_clamp(ly, g.dims[1]), y1 = cell_clamp(hy, g.dims[1]);
        const int z0 = cell_clamp(lz, g.dims[2]), z1 = cell_clamp(hz, g.dims[2]);
        for (int cz = z0; cz <= z1; ++cz)
            for (int cy = y0; cy <= y1; ++cy) {
                const size_t c = ((size_t)cz * g.dims[1] + cy) * g.dims[0];
                const int b = tst[c + x0], e = tst[c + x1 + 1];          // cells x0..x1 of this row are one run of records
                for (int k = b; k < e; ++k) {
                    const float4 q = trec[k];
                    const double dx = (double)q.x - tx, dy = (double)q.y - ty, dz = (double)q.z - tz;
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const int row = __float_as_int(q.w);
                    if (d2 < best || (d2 == best && row < brow)) { best = d2; brow = row; bk = k; }
                }
            }
    }
    return {best, brow, bk};
}

// ---- what the chunked kernels share: each fixes bits or slot ownership, so each is defined once ------------------------------------------
// This workgroup's row (task, chunk) of the ragged work list -> false: a padding row, a task that is done (where DONE asks for the word), or a
// chunk past the task's points.  (The caller reads its task record itself: handing it back from here costs the search an instruction per point.)
template <bool DONE, class Task>
__device__ __forceinline__ bool work_row(const Task *__restrict__ tasks, int n_tasks, const int32_t *__restrict__ work, const PairState *__restrict__ state,
                                         int &task, int &chunk) {
    task = work[2 * blockIdx.x]; chunk = work[2 * blockIdx.x + 1];
    if (task < 0 || task >= n_tasks || chunk < 0) return false;
    if (DONE && state[task].done) return false;
    return (int64_t)chunk * ICP_CHUNK < tasks[task].n_src;
}

// p' = ((R0 x + R1 y) + R2 z) + t, row by row
__device__ __forceinline__ void transform_point(const double *R, const double *t, double x, double y, double z, double &tx, double &ty, double &tz) {
    tx = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
    ty = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
    tz = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
}

// The workgroup's words 0..W-1 into its slot: every wave's sum by butterfly, then ((w0 + w1) + w2) + w3.  (Holds the workgroup's barrier.)
template <int W, int N>
__device__ __forceinline__ void slot_write(const double (&acc)[N], double (&red)[ICP_THREADS / 64][N], double *__restrict__ slot) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < W; ++q) {
        const double v = wave_sum(acc[q]);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < W) slot[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// word w of a task's n_slots slots of W words, summed in slot order: the same in every workgroup that asks
__device__ __forceinline__ double slot_sum(const double *__restrict__ slots, int slot0, int n_slots, int W, int w) {
    double s = 0.0;
    for (int k = 0; k < n_slots; ++k) s += slots[((size_t)slot0 + k) * W + w];
    return s;
}
__device__ __forceinline__ int slots_of(int n_src) { return (n_src + ICP_CHUNK - 1) / ICP_CHUNK; }

template <class Task>
__global__ __launch_bounds__(64) void icp_init_kernel(const Task *__restrict__ tasks, int n_tasks, PairState *__restrict__ state, IcpOut out) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_tasks) return;
    const double *T0 = tasks[p].T0;
    bool finite = true;
    PairState st;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) { st.R[r * 3 + c] = T0[r * 4 + c]; finite = finite && isfinite(T0[r * 4 + c]); }
        st.t[r] = T0[r * 4 + 3]; finite = finite && isfinite(T0[r * 4 + 3]);
    }
    st.rmse = __builtin_nan("");
    st.done = finite ? 0 : 1; st.iters = 0; st.inliers = 0; st.status = finite ? ST_MAX_ITER : ST_NONFINITE; st.pad_ = 0;
    state[p] = st;
    for (int q = 0; q < 16; ++q) out.T[(size_t)p * 16 + q] = T0[q];
    out.iters[p] = 0; out.inliers[p] = 0; out.rmse[p] = st.rmse; out.status[p] = st.status;
}

template <class Task>
__global__ __launch_bounds__(ICP_THREADS) void icp_search_kernel(const Task *__restrict__ tasks, int n_tasks, const int32_t *__restrict__ work,
                                                                 const PairState *__restrict__ state, double *__restrict__ sums,
                                                                 int32_t *__restrict__ assign, double thr2, double reach) {
    __shared__ double red[ICP_THREADS / 64][SUM_W];
    int pair, chunk;
    if (!work_row<true>(tasks, n_tasks, work, state, pair, chunk)) return;
    const Task tk = tasks[pair];
    const PairState &st = state[pair];
    const int n1 = tk.n_src;
    const GridDesc g = *grid_desc(tk.tgt);
    const float4 *__restrict__ trec = grid_recs(tk.tgt);
    const int32_t *__restrict__ tst = grid_starts(tk.tgt, g.n);
    const float4 *__restrict__ srec = grid_recs(tk.src);
    const double inv = 1.0 / g.edge;
    const int tid = threadIdx.x;
    const size_t off = (size_t)tk.slot0 * ICP_CHUNK;
    double R[9], t[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = st.R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) t[q] = st.t[q];
    double acc[SUM_W] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int it = 0; it < ICP_PER_THREAD; ++it) {
        const int j = chunk * ICP_CHUNK + it * ICP_THREADS + tid;
        if (j >= n1) continue;
        const float4 p = srec[j];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        double tx, ty, tz;
        transform_point(R, t, px, py, pz, tx, ty, tz);
        const Nearest nn = nearest_record(g, trec, tst, inv, tx, ty, tz, reach);
        const double best = nn.d2;
        const int bk = nn.k;
        const bool in = bk >= 0 && best <= thr2;
        assign[off + j] = in ? bk : -1;
        if (in) {
            const float4 q = trec[bk];
            acc[0] += 1.0;
            acc[1] += (double)q.x; acc[2] += (double)q.y; acc[3] += (double)q.z;
            acc[4] += px; acc[5] += py; acc[6] += pz;
            acc[7] += best;
        }
    }
    slot_write<SUM_W>(acc, red, sums + ((size_t)tk.slot0 + chunk) * SUM_W);
}

__global__ __launch_bounds__(ICP_THREADS) void icp_cov_kernel(const IcpTask *__restrict__ tasks, int n_tasks, const int32_t *__restrict__ work,
                                                              const PairState *__restrict__ state, const double *__restrict__ sums,
                                                              double *__restrict__ hs, const int32_t *__restrict__ assign) {
    __shared__ double red[ICP_THREADS / 64][COV_W];
    __shared__ double cen[SUM_W];
    int pair, chunk;
    if (!work_row<true>(tasks, n_tasks, work, state, pair, chunk)) return;
    const IcpTask tk = tasks[pair];
    const int n1 = tk.n_src;
    const float4 *__restrict__ trec = grid_recs(tk.tgt);
    const float4 *__restrict__ srec = grid_recs(tk.src);
    const int tid = threadIdx.x;
    if (tid < 7) cen[tid] = slot_sum(sums, tk.slot0, slots_of(n1), SUM_W, tid);          // the pair's centroids: the same in every workgroup of the pair
    __syncthreads();
    const double n = cen[0];
    double h[COV_W] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n > 0.0) {
        const double cqx = cen[1] / n, cqy = cen[2] / n, cqz = cen[3] / n, cpx = cen[4] / n, cpy = cen[5] / n, cpz = cen[6] / n;
        const size_t off = (size_t)tk.slot0 * ICP_CHUNK;
        for (int it = 0; it < ICP_PER_THREAD; ++it) {
            const int j = chunk * ICP_CHUNK + it * ICP_THREADS + tid;
            if (j >= n1) continue;
            const int a = assign[off + j];
            if (a < 0) continue;
            const float4 q = trec[a], p = srec[j];
            const double ax = (double)q.x - cqx, ay = (double)q.y - cqy, az = (double)q.z - cqz;
            const double bx = (double)p.x - cpx, by = (double)p.y - cpy, bz = (double)p.z - cpz;
            h[0] += ax * bx; h[1] += ax * by; h[2] += ax * bz;
            h[3] += ay * bx; h[4] += ay * by; h[5] += ay * bz;
            h[6] += az * bx; h[7] += az * by; h[8] += az * bz;
        }
    }
    slot_write<COV_W>(h, red, hs + ((size_t)tk.slot0 + chunk) * COV_W);
}

// H = U S V^T by one-sided Jacobi (the scheme of csrc/ransac.hip polar_uvt); R = U diag(1, 1, det(U V^T)) V^T.  With (u1, v1), (u2, v2) the
// two leading pairs that product is u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T whatever signs the third pair carries, so the third pair is
// never formed: a coplanar inlier set (rank 2) takes the same path as a full-rank one.  false: rank(H) <= 1.
__device__ bool kabsch_rotation(const double *Hm, double *R) {
    double A[9], V[9];
    double scale = 0.0;
    for (int i = 0; i < 9; ++i) { A[i] = Hm[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; scale = fmax(scale, fabs(Hm[i])); }
    if (!(scale > 0.0) || !isfinite(scale)) return false;
    int ex;                                                        // scale out the largest entry's power of two (exact): see polar_uvt
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
                const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
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
    double nrm[3];
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt(A[c] * A[c] + A[3 + c] * A[3 + c] + A[6 + c] * A[6 + c]);
    int i1 = 0;
    if (nrm[1] > nrm[i1]) i1 = 1;
    if (nrm[2] > nrm[i1]) i1 = 2;
    int i2 = (i1 + 1) % 3;
    const int i3 = (i1 + 2) % 3;
    if (nrm[i3] > nrm[i2]) i2 = i3;
    if (!(nrm[i2] > 1e-10 * nrm[i1])) return false;
    double u1[3], u2[3], v1[3], v2[3];
    for (int r = 0; r < 3; ++r) {
        u1[r] = A[r * 3 + i1] / nrm[i1]; u2[r] = A[r * 3 + i2] / nrm[i2];
        v1[r] = V[r * 3 + i1]; v2[r] = V[r * 3 + i2];
    }
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = (u1[r] * v1[c] + u2[r] * v2[c]) + u3[r] * v3[c];
    return true;
}

// The end of either method's solve, on lane 0 of the pair's workgroup: from the method's step (R+, t+) -- or support == false: nothing could be
// solved and the pair ends with its transform kept -- to the step sizes, the convergence test, the pair's state with its `done` word, its
// row of T_out and its four other outputs.  n_in, rmse: what the method counts as inliers and their residual.
__device__ __forceinline__ void solve_tail(PairState &st, int pair, bool support, const double *Rn, const double *tn, double n_in, double rmse, int it,
                                           int max_iter, double tol_deg, double tol_t, const IcpOut &out) {
    int status = ST_MAX_ITER, done = it + 1 >= max_iter;
    if (!support) {
        status = ST_NO_SUPPORT; done = 1;
    } else {
        double fro = 0.0, dt = 0.0;
        for (int r = 0; r < 3; ++r) { const double e = tn[r] - st.t[r]; dt += e * e; }
        for (int q = 0; q < 9; ++q) { const double e = Rn[q] - st.R[q]; fro += e * e; }
        // |R+ - R|_F = 2 sqrt(2) sin(angle / 2): well conditioned at the small angles the test is about, unlike acos((trace - 1) / 2)
        const double ang = 2.0 * asin(fmin(1.0, sqrt(fro) / (2.0 * sqrt(2.0)))) * (180.0 / 3.14159265358979323846);
        for (int q = 0; q < 9; ++q) st.R[q] = Rn[q];
        for (int q = 0; q < 3; ++q) st.t[q] = tn[q];
        if (ang < tol_deg && sqrt(dt) < tol_t) { status = ST_CONVERGED; done = 1; }
        double *T = out.T + (size_t)pair * 16;
        for (int r = 0; r < 3; ++r) { T[r * 4] = Rn[r * 3]; T[r * 4 + 1] = Rn[r * 3 + 1]; T[r * 4 + 2] = Rn[r * 3 + 2]; T[r * 4 + 3] = tn[r]; }
        T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
    }
    st.iters = it + 1; st.inliers = (int)n_in; st.rmse = rmse; st.status = status; st.done = done;
    out.iters[pair] = it + 1; out.inliers[pair] = (int)n_in; out.rmse[pair] = rmse; out.status[pair] = status;
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const IcpTask *__restrict__ tasks, PairState *__restrict__ state, const double *__restrict__ sums,
                                                       const double *__restrict__ hs, int it, int max_iter, double tol_deg, double tol_t, IcpOut out,
                                                       double *__restrict__ stats_out) {
    __shared__ double S[SUM_W + COV_W];
    const int pair = blockIdx.x, tid = threadIdx.x;
    PairState &st = state[pair];
    if (st.done) return;
    const IcpTask tk = tasks[pair];
    if (tid < SUM_W) S[tid] = slot_sum(sums, tk.slot0, slots_of(tk.n_src), SUM_W, tid);
    else if (tid < SUM_W + COV_W) S[tid] = slot_sum(hs, tk.slot0, slots_of(tk.n_src), COV_W, tid - SUM_W);
    __syncthreads();
    if (tid != 0) return;
    const double n = S[0];
    const double rmse = sqrt(S[7] / n);          // n == 0: NaN
    double cq[3] = {0, 0, 0}, cp[3] = {0, 0, 0}, Rn[9], tn[3];
    bool support = n >= 3.0;
    if (n > 0.0)
        for (int q = 0; q < 3; ++q) { cq[q] = S[1 + q] / n; cp[q] = S[4 + q] / n; }
    if (support) support = kabsch_rotation(S + SUM_W, Rn);
    if (support)
        for (int r = 0; r < 3; ++r) tn[r] = cq[r] - ((Rn[r * 3] * cp[0] + Rn[r * 3 + 1] * cp[1]) + Rn[r * 3 + 2] * cp[2]);
    solve_tail(st, pair, support, Rn, tn, n, rmse, it, max_iter, tol_deg, tol_t, out);
    if (stats_out) {
        double *o = stats_out + (size_t)pair * 16;
        o[0] = n;
        for (int q = 0; q < 3; ++q) { o[1 + q] = cq[q]; o[4 + q] = cp[q]; }
        for (int q = 0; q < 9; ++q) o[7 + q] = S[SUM_W + q];
    }
}

// the assignments of the last executed search in ORIGINAL rows (tests, callers that want the correspondences)
template <class Task>
__global__ __launch_bounds__(ICP_THREADS) void icp_export_kernel(const Task *__restrict__ tasks, int n_tasks, const int32_t *__restrict__ work,
                                                                 const PairState *__restrict__ state, const int32_t *__restrict__ assign,
                                                                 int32_t *__restrict__ out) {
    int pair, chunk;
    if (!work_row<false>(tasks, n_tasks, work, state, pair, chunk)) return;          // (a pair that is done has assignments too)
    const Task tk = tasks[pair];
    const int n1 = tk.n_src, n0 = grid_desc(tk.tgt)->n;
    const bool ran = state[pair].iters > 0;          // no search ran (non-finite T0): the stored assignments are not defined
    const float4 *__restrict__ trec = grid_recs(tk.tgt);
    const float4 *__restrict__ srec = grid_recs(tk.src);
    const size_t off = (size_t)tk.slot0 * ICP_CHUNK;
    for (int it = 0; it < ICP_PER_THREAD; ++it) {
        const int j = chunk * ICP_CHUNK + it * ICP_THREADS + threadIdx.x;
        if (j >= n1) continue;
        const int row = __float_as_int(srec[j].w);
        if (row < 0 || row >= n1) continue;
        const int a = ran ? assign[off + j] : -1;
        out[off + row] = (a >= 0 && a < n0) ? __float_as_int(trec[a].w) : -1;
    }
}

// ---- v6d: surface normals and the point-to-plane iteration (tests/_icp_plane_oracle.py is the numpy restatement) -----------------------
constexpr int NORMALS_BLOCKS = 2048;    // 256 CUs x 8 workgroups of 256: every SIMD holds waves to hide the walk's loads

// s += x with the rounding error of the addition kept in e (Knuth's two-sum): hi + lo carries the sum to about twice the working precision,
// so its rounded value does not depend on the order of the terms -- which is what makes a cloud's table the same whichever grid was walked.
__device__ __forceinline__ void dd_add(double &s, double &e, double x) {
    const double t = s + x;
    const double bb = t - s;
    e += (s - (t - bb)) + (x - bb);
    s = t;
}
__device__ __forceinline__ void dd_add_prod(double &s, double &e, double a, double b) {
    const double p = a * b;
    e += fma(a, b, -p);                // the product's own rounding error, exactly
    dd_add(s, e, p);
}

// One record per lane in cell order: a wave's lanes walk the same cells.  out[original row] = (nx, ny, nz, m).
__global__ __launch_bounds__(256) void icp_normals_kernel(const void *__restrict__ grid, double thr2, double reach, int min_neighbors, double *__restrict__ out) {
    const GridDesc g = *grid_desc(grid);
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, g.n);
    const double inv = 1.0 / g.edge;
    // (the host does not know n: a fixed launch strides over the records)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < g.n; i += gridDim.x * 256) {
        const float4 p = rec[i];
        const int row = __float_as_int(p.w);
        if (row < 0 || row >= g.n) continue;
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        int m = 0;
        double s[3] = {0, 0, 0}, se[3] = {0, 0, 0};
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;        // exact: both are float32 values
            if ((dx * dx + dy * dy) + dz * dz <= thr2) {
                ++m;
                dd_add(s[0], se[0], dx); dd_add(s[1], se[1], dy); dd_add(s[2], se[2], dz);
            }
        });
        const double mx = (s[0] + se[0]) / (double)m, my = (s[1] + se[1]) / (double)m, mz = (s[2] + se[2]) / (double)m;       // m >= 1: the point itself
        double c[6] = {0, 0, 0, 0, 0, 0}, ce[6] = {0, 0, 0, 0, 0, 0};
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
            if ((dx * dx + dy * dy) + dz * dz <= thr2) {
                const double ax = dx - mx, ay = dy - my, az = dz - mz;
                dd_add_prod(c[0], ce[0], ax, ax); dd_add_prod(c[1], ce[1], ax, ay); dd_add_prod(c[2], ce[2], ax, az);
                dd_add_prod(c[3], ce[3], ay, ay); dd_add_prod(c[4], ce[4], ay, az); dd_add_prod(c[5], ce[5], az, az);
            }
        });
#pragma unroll
        for (int q = 0; q < 6; ++q) c[q] += ce[q];
        double lam[3], V[9];
        icp_math::jacobi3(c, lam, V);
        // the smallest eigenvalue's column, by selects (no run-time index into registers)
        const int imin = (lam[0] <= lam[1] && lam[0] <= lam[2]) ? 0 : (lam[1] <= lam[2] ? 1 : 2);
        const double lmax = fmax(lam[0], fmax(lam[1], lam[2]));
        const double lmid = imin == 0 ? fmin(lam[1], lam[2]) : (imin == 1 ? fmin(lam[0], lam[2]) : fmin(lam[0], lam[1]));
        double nx = imin == 0 ? V[0] : (imin == 1 ? V[1] : V[2]);
        double ny = imin == 0 ? V[3] : (imin == 1 ? V[4] : V[5]);
        double nz = imin == 0 ? V[6] : (imin == 1 ? V[7] : V[8]);
        const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
        const bool valid = m >= min_neighbors && lmid > 1e-8 * lmax && nn > 0.0;
        if (valid) { nx /= nn; ny /= nn; nz /= nn; } else { nx = 0.0; ny = 0.0; nz = 0.0; }
        double4 *o = reinterpret_cast<double4 *>(out) + row;
        *o = make_double4(nx, ny, nz, (double)m);
    }
}

// Same ragged work list and slot ownership as icp_cov_kernel.  c = R c_p + t with c_p rebuilt from the pair's first-pass slots in slot order.
// Task = IcpPlaneTask: the v6d pass.  Task = IcpPlaneRobustTask ("v6p"): every correspondence's J J^T and J e enter with the weight of its
// residual e (icp_math::robust_weight; the task's kind and scale are wave-uniform, the weight is selects); the count and sum e^2 stay
// unweighted.  The unweighted instantiation has none of the weighted one's operations: its arithmetic is what it was.
template <class Task>
__global__ __launch_bounds__(ICP_THREADS) void icp_plane_kernel(const Task *__restrict__ tasks, int n_tasks, const int32_t *__restrict__ work,
                                                                const PairState *__restrict__ state, const double *__restrict__ sums,
                                                                double *__restrict__ ps, const int32_t *__restrict__ assign) {
    __shared__ double red[ICP_THREADS / 64][PLANE_W];
    __shared__ double cen[SUM_W];
    int pair, chunk;
    if (!work_row<true>(tasks, n_tasks, work, state, pair, chunk)) return;
    const Task tk = tasks[pair];
    const PairState &st = state[pair];
    const int n1 = tk.n_src;
    const int n0 = grid_desc(tk.tgt)->n;
    const float4 *__restrict__ trec = grid_recs(tk.tgt);
    const float4 *__restrict__ srec = grid_recs(tk.src);
    const double4 *__restrict__ nrm = reinterpret_cast<const double4 *>(tk.normals);
    const int tid = threadIdx.x;
    if (tid < 7) cen[tid] = slot_sum(sums, tk.slot0, slots_of(n1), SUM_W, tid);
    __syncthreads();
    const double n = cen[0];
    double acc[PLANE_W];
#pragma unroll
    for (int q = 0; q < PLANE_W; ++q) acc[q] = 0.0;
    if (n > 0.0) {
        double R[9], t[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = st.R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) t[q] = st.t[q];
        double cx, cy, cz;
        transform_point(R, t, cen[4] / n, cen[5] / n, cen[6] / n, cx, cy, cz);
        const size_t off = (size_t)tk.slot0 * ICP_CHUNK;
        for (int it = 0; it < ICP_PER_THREAD; ++it) {
            const int j = chunk * ICP_CHUNK + it * ICP_THREADS + tid;
            if (j >= n1) continue;
            const int a = assign[off + j];
            if (a < 0 || a >= n0) continue;
            const float4 q = trec[a], p = srec[j];
            const int row = __float_as_int(q.w);
            if (row < 0 || row >= n0) continue;
            const double4 nv = nrm[row];
            if (nv.x == 0.0 && nv.y == 0.0 && nv.z == 0.0) continue;          // no valid normal at this target point
            double tx, ty, tz;
            transform_point(R, t, (double)p.x, (double)p.y, (double)p.z, tx, ty, tz);
            const double ax = tx - cx, ay = ty - cy, az = tz - cz;
            const double dx = tx - (double)q.x, dy = ty - (double)q.y, dz = tz - (double)q.z;
            const double e = (nv.x * dx + nv.y * dy) + nv.z * dz;
            const double J[6] = {ay * nv.z - az * nv.y, az * nv.x - ax * nv.z, ax * nv.y - ay * nv.x, nv.x, nv.y, nv.z};
            double JL[6];                                   // the left factor of every product: J, or w J under a loss
#pragma unroll
            for (int r = 0; r < 6; ++r) JL[r] = J[r];
            if constexpr (Task::robust) {
                const double wt = icp_math::robust_weight(tk.loss, e, tk.scale);
#pragma unroll
                for (int r = 0; r < 6; ++r) JL[r] = wt * J[r];
            }
            acc[0] += 1.0;
            int w = 1;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = r; c < 6; ++c) acc[w++] += JL[r] * J[c];
#pragma unroll
            for (int r = 0; r < 6; ++r) acc[22 + r] -= JL[r] * e;
            acc[28] += e * e;
        }
    }
    slot_write<PLANE_W>(acc, red, ps + ((size_t)tk.slot0 + chunk) * PLANE_W);
}

// One workgroup per pair: the slots reduced in slot order over the lanes, then lane 0: 6x6 Jacobi (A and V in LDS, indexed at run time),
// x = V diag(1 / lambda) V^T b = (w, v), dR = exp([w]x), R+ = dR R, t+ = dR (t - c) + c + v, then solve_tail.  The solve of every method
// whose second pass fills the 29-word slot (plane, gicp): of the task record it reads n_src and slot0.
template <class Task>
__global__ __launch_bounds__(64) void icp_plane_solve_kernel(const Task *__restrict__ tasks, PairState *__restrict__ state, const double *__restrict__ sums,
                                                             const double *__restrict__ ps, int it, int max_iter, double tol_deg, double tol_t, IcpOut out,
                                                             double *__restrict__ stats_out) {
    __shared__ double S[SUM_W + PLANE_W];
    __shared__ double A[36], V[36];
    const int pair = blockIdx.x, tid = threadIdx.x;
    PairState &st = state[pair];
    if (st.done) return;
    const Task tk = tasks[pair];
    if (tid < SUM_W) S[tid] = slot_sum(sums, tk.slot0, slots_of(tk.n_src), SUM_W, tid);
    else if (tid < SUM_W + PLANE_W) S[tid] = slot_sum(ps, tk.slot0, slots_of(tk.n_src), PLANE_W, tid - SUM_W);
    __syncthreads();
    if (tid != 0) return;
    const double n = S[0];
    const double *P = S + SUM_W;
    const double nv = n > 0.0 ? P[0] : 0.0;          // no distance inlier: the plane pass wrote zeros
    const double rmse = sqrt(P[28] / nv);            // nv == 0: NaN
    double c[3] = {0, 0, 0}, b[6];
    if (n > 0.0) transform_point(st.R, st.t, S[4] / n, S[5] / n, S[6] / n, c[0], c[1], c[2]);
    {
        int w = 1;
        for (int r = 0; r < 6; ++r)
            for (int q = r; q < 6; ++q) { A[r * 6 + q] = P[w]; A[q * 6 + r] = P[w]; ++w; }
        for (int r = 0; r < 6; ++r) b[r] = P[22 + r];
    }
    bool support = nv >= 6.0;
    double x[6] = {0, 0, 0, 0, 0, 0};
    if (support) {
        bool finite = true;
        for (int q = 0; q < 36; ++q) finite = finite && isfinite(A[q]);
        for (int q = 0; q < 6; ++q) finite = finite && isfinite(b[q]);
        support = finite;
    }
    if (support) {
        icp_math::jacobi_sym(A, V, 6);
        double lmin = A[0], lmax = A[0];
        for (int q = 1; q < 6; ++q) { lmin = fmin(lmin, A[q * 7]); lmax = fmax(lmax, A[q * 7]); }
        support = lmax > 0.0 && lmin > 1e-10 * lmax;
        if (support)
            for (int k = 0; k < 6; ++k) {
                double d = 0.0;
                for (int r = 0; r < 6; ++r) d += V[r * 6 + k] * b[r];
                d /= A[k * 7];
                for (int r = 0; r < 6; ++r) x[r] += V[r * 6 + k] * d;
            }
    }
    double Rn[9], tn[3];
    if (support) {
        double dR[9];
        icp_math::rodrigues(x, dR);
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) Rn[r * 3 + q] = (dR[r * 3] * st.R[q] + dR[r * 3 + 1] * st.R[3 + q]) + dR[r * 3 + 2] * st.R[6 + q];
            tn[r] = (((dR[r * 3] * (st.t[0] - c[0]) + dR[r * 3 + 1] * (st.t[1] - c[1])) + dR[r * 3 + 2] * (st.t[2] - c[2])) + c[r]) + x[3 + r];
        }
    }
    solve_tail(st, pair, support, Rn, tn, nv, rmse, it, max_iter, tol_deg, tol_t, out);
    if (stats_out) {
        double *o = stats_out + (size_t)pair * PLANE_STATS_W;
        o[0] = nv;
        for (int q = 0; q < 3; ++q) o[1 + q] = c[q];
        for (int q = 0; q < 27; ++q) o[4 + q] = n > 0.0 ? P[1 + q] : 0.0;
        o[31] = n > 0.0 ? P[28] : 0.0;
    }
}

// ---- v6i: the plane-to-plane (generalized) iteration (tests/_icp_gicp_oracle.py is the numpy restatement) --------------------------------
// icp_plane_kernel's skeleton with every residual d = p' - q weighted by M = S^-1, S = C_q + R C_p R^T.  A surface-aligned covariance
// V diag(1, 1, eps) V^T with n the eigenvector of eps is I - (1 - eps) n n^T, so S = 2 I - kappa (n_q n_q^T + m m^T), m = R n_p, comes from the
// two normal tables alone; a zero row (no valid normal) leaves the identity, and nothing is branched on.  With J = [-[a]x, I] the blocks of
// J^T M J are [a]x M [a]x^T, G = [a]x M and M, so no 3x6 matrix is formed: G's column j is a x (column j of M), the rotation block's row i is
// a x (row i of G).  M by the adjugate over the determinant (icp_math.h gicp_weight; eigenvalues of S in [2 eps, 2]).
// Task = IcpGicpRobustTask ("v6p"): the weight of r = sqrt(2 eps d^T M d) (icp_math::gicp_residual) scales M and M d before they enter A and
// b; the count and sum d^T M d stay unweighted.  The unweighted instantiation has none of that.
template <class Task>
__global__ __launch_bounds__(ICP_THREADS) void icp_gicp_kernel(const Task *__restrict__ tasks, int n_tasks, const int32_t *__restrict__ work,
                                                               const PairState *__restrict__ state, const double *__restrict__ sums,
                                                               double *__restrict__ ps, const int32_t *__restrict__ assign) {
    __shared__ double red[ICP_THREADS / 64][PLANE_W];
    __shared__ double cen[SUM_W];
    int pair, chunk;
    if (!work_row<true>(tasks, n_tasks, work, state, pair, chunk)) return;
    const Task tk = tasks[pair];
    const PairState &st = state[pair];
    const int n1 = tk.n_src;
    const int n0 = grid_desc(tk.tgt)->n;
    const float4 *__restrict__ trec = grid_recs(tk.tgt);
    const float4 *__restrict__ srec = grid_recs(tk.src);
    const double4 *__restrict__ nrm_q = reinterpret_cast<const double4 *>(tk.tgt_normals);
    const double4 *__restrict__ nrm_p = reinterpret_cast<const double4 *>(tk.src_normals);
    const double kappa = 1.0 - tk.epsilon;
    const int tid = threadIdx.x;
    if (tid < 7) cen[tid] = slot_sum(sums, tk.slot0, slots_of(n1), SUM_W, tid);
    __syncthreads();
    const double n = cen[0];
    double acc[PLANE_W];
#pragma unroll
    for (int q = 0; q < PLANE_W; ++q) acc[q] = 0.0;
    if (n > 0.0) {
        double R[9], t[3];
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = st.R[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) t[q] = st.t[q];
        double cx, cy, cz;
        transform_point(R, t, cen[4] / n, cen[5] / n, cen[6] / n, cx, cy, cz);
        const size_t off = (size_t)tk.slot0 * ICP_CHUNK;
        for (int it = 0; it < ICP_PER_THREAD; ++it) {
            const int j = chunk * ICP_CHUNK + it * ICP_THREADS + tid;
            if (j >= n1) continue;
            const int a = assign[off + j];
            if (a < 0 || a >= n0) continue;
            const float4 q = trec[a], p = srec[j];
            const int row = __float_as_int(q.w), prow = __float_as_int(p.w);
            if (row < 0 || row >= n0 || prow < 0 || prow >= n1) continue;          // (not a record of these grids: nothing to read a normal from)
            const double4 nq = nrm_q[row], np = nrm_p[prow];
            double tx, ty, tz;
            transform_point(R, t, (double)p.x, (double)p.y, (double)p.z, tx, ty, tz);
            const double ax = tx - cx, ay = ty - cy, az = tz - cz;
            const double dx = tx - (double)q.x, dy = ty - (double)q.y, dz = tz - (double)q.z;
            // m = R n_p
            const double mx = (R[0] * np.x + R[1] * np.y) + R[2] * np.z;
            const double my = (R[3] * np.x + R[4] * np.y) + R[5] * np.z;
            const double mz = (R[6] * np.x + R[7] * np.y) + R[8] * np.z;
            // M = (2 I - kappa (n_q n_q^T + m m^T))^-1
            double M[6];
            icp_math::gicp_weight(nq.x, nq.y, nq.z, mx, my, mz, kappa, M);
            double m00 = M[0], m01 = M[1], m02 = M[2], m11 = M[3], m12 = M[4], m22 = M[5];
            // w = M d
            double wx = (m00 * dx + m01 * dy) + m02 * dz, wy = (m01 * dx + m11 * dy) + m12 * dz, wz = (m02 * dx + m12 * dy) + m22 * dz;
            double q2;                                                // d^T M d, unweighted
            if constexpr (Task::robust) {
                q2 = (dx * wx + dy * wy) + dz * wz;
                const double wt = icp_math::robust_weight(tk.loss, icp_math::gicp_residual(q2, tk.epsilon), tk.scale);
                m00 *= wt; m01 *= wt; m02 *= wt; m11 *= wt; m12 *= wt; m22 *= wt;
                wx *= wt; wy *= wt; wz *= wt;
            }
            // G = [a]x M: column j is a x (column j of M)
            const double g00 = ay * m02 - az * m01, g01 = ay * m12 - az * m11, g02 = ay * m22 - az * m12;
            const double g10 = az * m00 - ax * m02, g11 = az * m01 - ax * m12, g12 = az * m02 - ax * m22;
            const double g20 = ax * m01 - ay * m00, g21 = ax * m11 - ay * m01, g22 = ax * m12 - ay * m02;
            acc[0] += 1.0;
            // row i of [a]x M [a]x^T is a x (row i of G); the upper entries of A row by row
            acc[1] += ay * g02 - az * g01; acc[2] += az * g00 - ax * g02; acc[3] += ax * g01 - ay * g00;
            acc[4] += g00; acc[5] += g01; acc[6] += g02;
            acc[7] += az * g10 - ax * g12; acc[8] += ax * g11 - ay * g10;
            acc[9] += g10; acc[10] += g11; acc[11] += g12;
            acc[12] += ax * g21 - ay * g20;
            acc[13] += g20; acc[14] += g21; acc[15] += g22;
            acc[16] += m00; acc[17] += m01; acc[18] += m02;
            acc[19] += m11; acc[20] += m12;
            acc[21] += m22;
            // b = -sum J^T M d = -(a x w, w)
            acc[22] -= ay * wz - az * wy; acc[23] -= az * wx - ax * wz; acc[24] -= ax * wy - ay * wx;
            acc[25] -= wx; acc[26] -= wy; acc[27] -= wz;
            if constexpr (!Task::robust) q2 = (dx * wx + dy * wy) + dz * wz;          // (where the v6i pass has always formed it)
            acc[28] += q2;
        }
    }
    slot_write<PLANE_W>(acc, red, ps + ((size_t)tk.slot0 + chunk) * PLANE_W);
}

// ---- v6g: read-only evaluation of (cloud 0, cloud 1, T) in both directions (tests/_dense_eval_oracle.py is the numpy restatement) --------
// One launch over the 2 n tasks of n pairs: task p < n is pair p forward (source -> target under T), task n + p the same pair backward (the
// binding's row n + p carries the grids swapped and the same T; the kernel takes the inverse by transposition).  The search is
// icp_search_kernel's (nearest_record); the 11 sums (n, sum x, the 6 upper entries of sum x x^T, sum d2; x the untransformed query point)
// go through the workgroup's fixed slot (work_row, transform_point and slot_write are the iteration's), and icp_eval_finish_kernel reduces a
// task's slots in ascending chunk order (slot_sum).  The backward moments are summed like the forward ones and not used.  sum d2 is carried
// with its rounding errors (two-sum, slot words 10 and 11, merged by dd_merge and not by the plain sums), so that its rounded value does
// not depend on the order of the terms: the backward direction's queries come in the order of cloud 0's grid, and the pair's result must
// not depend on the radius that grid was built for.

// (s, e) += (s2, e2): the two leading parts by two-sum, the error parts added
__device__ __forceinline__ void dd_merge(double &s, double &e, double s2, double e2) {
    const double t = s + s2;
    const double bb = t - s;
    e = (e + e2) + ((s - (t - bb)) + (s2 - bb));
    s = t;
}

enum { EVAL_OK = 0, EVAL_NONFINITE = 1 };

// A value every lane of the wave holds alike, moved to scalar registers: the backward task's transform is computed (the scalar unit has no
// float64 arithmetic), and twelve doubles kept per lane through the search cost the kernel a wave of occupancy per SIMD.
__device__ __forceinline__ double wave_uniform(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

__global__ __launch_bounds__(ICP_THREADS) void icp_eval_kernel(const IcpTask *__restrict__ tasks, int n_pairs, const int32_t *__restrict__ work,
                                                               double *__restrict__ sums, int32_t *__restrict__ assign_out, double thr2, double reach) {
    __shared__ double red[ICP_THREADS / 64][EVAL_W];
    int task, chunk;
    if (!work_row<false>(tasks, 2 * n_pairs, work, (const PairState *)nullptr, task, chunk)) return;
    const IcpTask tk = tasks[task];
    const int n1 = min(tk.n_src, grid_desc(tk.src)->n);
    if ((int64_t)chunk * ICP_CHUNK >= n1) return;
    const GridDesc g = *grid_desc(tk.tgt);
    const float4 *__restrict__ trec = grid_recs(tk.tgt);
    const int32_t *__restrict__ tst = grid_starts(tk.tgt, g.n);
    const float4 *__restrict__ srec = grid_recs(tk.src);
    const double inv = 1.0 / g.edge;
    const int tid = threadIdx.x;
    const size_t off = (size_t)tk.slot0 * ICP_CHUNK;
    double R[9], t[3];
    bool finite = true;
    {
        const double *T = tk.T0;
        double Rf[9], tf[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { Rf[r * 3 + c] = T[r * 4 + c]; finite = finite && isfinite(Rf[r * 3 + c]); }
            tf[r] = T[r * 4 + 3]; finite = finite && isfinite(tf[r]);
        }
        if (task < n_pairs) {
#pragma unroll
            for (int q = 0; q < 9; ++q) R[q] = Rf[q];
#pragma unroll
            for (int q = 0; q < 3; ++q) t[q] = tf[q];
        } else {                           // Rinv = R^T, tinv_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) R[r * 3 + c] = Rf[c * 3 + r];
                t[r] = -((Rf[r] * tf[0] + Rf[3 + r] * tf[1]) + Rf[6 + r] * tf[2]);
            }
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = wave_uniform(R[q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) t[q] = wave_uniform(t[q]);
    }
    double acc[EVAL_W];
#pragma unroll
    for (int q = 0; q < EVAL_W; ++q) acc[q] = 0.0;
    for (int it = 0; it < ICP_PER_THREAD; ++it) {
        const int j = chunk * ICP_CHUNK + it * ICP_THREADS + tid;
        if (j >= n1) continue;
        const float4 p = srec[j];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        double tx, ty, tz;
        transform_point(R, t, px, py, pz, tx, ty, tz);
        Nearest nn = {__builtin_inf(), 0x7fffffff, -1};
        if (finite) nn = nearest_record(g, trec, tst, inv, tx, ty, tz, reach);                    // (a non-finite T searches nothing)
        const double best = nn.d2;
        const int brow = nn.row, bk = nn.k;
        const bool in = bk >= 0 && best <= thr2;
        if (assign_out) {
            const int row = __float_as_int(p.w);
            if (row >= 0 && row < n1) assign_out[off + row] = in ? brow : -1;
        }
        if (in) {
            acc[0] += 1.0;
            acc[1] += px; acc[2] += py; acc[3] += pz;
            acc[4] += px * px; acc[5] += px * py; acc[6] += px * pz;
            acc[7] += py * py; acc[8] += py * pz; acc[9] += pz * pz;
            dd_add(acc[10], acc[11], best);
        }
    }
    // words 10 and 11 by their own merge, ahead of the barrier that slot_write holds for the ten plain words
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dd_merge(acc[10], acc[11], __shfl_xor(acc[10], o), __shfl_xor(acc[11], o));
    if ((tid & 63) == 0) { red[tid >> 6][10] = acc[10]; red[tid >> 6][11] = acc[11]; }
    double *slot = sums + ((size_t)tk.slot0 + chunk) * EVAL_W;
    slot_write<10>(acc, red, slot);
    if (tid == 10) {
        double a = red[0][10], b = red[0][11];
        for (int w = 1; w < ICP_THREADS / 64; ++w) dd_merge(a, b, red[w][10], red[w][11]);
        slot[10] = a; slot[11] = b;
    }
}

// One workgroup per pair: lanes 0..10 reduce the forward task's slots in ascending chunk order, lanes 12..22 the backward task's (lane 10
// and 22: sum d2 with its error word); lane 0 writes the rows.  Lambda = sum G^T G, G = [I | -2 [x]x], in closed form from the moments (include/roreg_hip.h, v6g).
__global__ __launch_bounds__(64) void icp_eval_finish_kernel(const IcpTask *__restrict__ tasks, int n_pairs, const double *__restrict__ sums,
                                                             double *__restrict__ stats_out, double *__restrict__ info_out, int32_t *__restrict__ status_out) {
    __shared__ double S[2 * EVAL_W];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const IcpTask fw = tasks[pair], bw = tasks[n_pairs + pair];
    const int n_src = min(fw.n_src, grid_desc(fw.src)->n), n_tgt = min(bw.n_src, grid_desc(bw.src)->n);
    if (tid < 2 * EVAL_W) {
        const bool back = tid >= EVAL_W;
        const int n1 = back ? n_tgt : n_src, slot0 = back ? bw.slot0 : fw.slot0, w = back ? tid - EVAL_W : tid;
        const int n_slots = slots_of(n1);
        double s = 0.0, e = 0.0;
        if (w < 10) {
            s = slot_sum(sums, slot0, n_slots, EVAL_W, w);
        } else if (w == 10) {
            for (int k = 0; k < n_slots; ++k) dd_merge(s, e, sums[((size_t)slot0 + k) * EVAL_W + 10], sums[((size_t)slot0 + k) * EVAL_W + 11]);
            s += e;
        }
        S[tid] = s;
    }
    __syncthreads();
    if (tid != 0) return;
    bool finite = true;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) finite = finite && isfinite(fw.T0[r * 4 + c]);
    const double n01 = S[0], n10 = S[EVAL_W], S01 = S[10], S10 = S[EVAL_W + 10];
    double *st = stats_out + (size_t)pair * 8;
    st[0] = n01; st[1] = n10;
    st[2] = n10 / (double)n_tgt; st[3] = n01 / (double)n_src;          // overlap0, overlap1: NaN for an empty cloud
    st[4] = sqrt(S01 / n01); st[5] = sqrt(S10 / n10);                  // NaN without correspondences
    st[6] = S01; st[7] = S10;
    const double sx = S[1], sy = S[2], sz = S[3];
    const double xx = S[4], xy = S[5], xz = S[6], yy = S[7], yz = S[8], zz = S[9];
    double *L = info_out + (size_t)pair * 36;
    for (int q = 0; q < 36; ++q) L[q] = 0.0;
    L[0] = n01; L[7] = n01; L[14] = n01;
    // Lambda_tr = -2 [sum x]x (rows 0..2, columns 3..5) and its transpose
    L[4] = 2.0 * sz; L[5] = 0.0 - 2.0 * sy;
    L[9] = 0.0 - 2.0 * sz; L[11] = 2.0 * sx;
    L[15] = 2.0 * sy; L[16] = 0.0 - 2.0 * sx;
    L[24] = L[4]; L[30] = L[5]; L[18 + 1] = L[9]; L[30 + 1] = L[11]; L[18 + 2] = L[15]; L[24 + 2] = L[16];
    // Lambda_rr = 4 (tr(M) I - M), M = sum x x^T: the diagonal as the sum of the two other squares (no cancellation)
    L[21] = 4.0 * (yy + zz); L[28] = 4.0 * (xx + zz); L[35] = 4.0 * (xx + yy);
    L[22] = 0.0 - 4.0 * xy; L[27] = L[22];
    L[23] = 0.0 - 4.0 * xz; L[33] = L[23];
    L[29] = 0.0 - 4.0 * yz; L[34] = L[29];
    status_out[pair] = finite ? EVAL_OK : EVAL_NONFINITE;
}

}  // namespace

extern "C" size_t roreg_icp_grid_size(const double *lo, const double *hi, int n, double max_dist, roreg_icp_grid_desc *desc, size_t *workspace_bytes) {
    if (!lo || !hi || !desc || n < 0 || !(max_dist > 0.0) || !std::isfinite(max_dist)) {
        roreg::set_error("roreg_icp_grid_size: bad arguments");
        return 0;
    }
    double ext[3];
    for (int a = 0; a < 3; ++a) {
        ext[a] = n > 0 ? hi[a] - lo[a] : 0.0;
        if (!(ext[a] >= 0.0) || !std::isfinite(ext[a]) || !std::isfinite(lo[a])) {
            roreg::set_error("roreg_icp_grid_size: the bounding box is not finite");
            return 0;
        }
    }
    double edge = max_dist;
    int64_t dims[3], cells = 0;
    for (int s = 0; s < 2000; ++s, edge *= 2.0) {
        bool ok = true;
        cells = 1;
        for (int a = 0; a < 3 && ok; ++a) {
            const double c = floor(ext[a] / edge) + 3.0;       // the box's cells and one of padding on either side
            ok = c <= (double)MAX_CELLS;
            dims[a] = ok ? (int64_t)c : 0;
            if (ok) { cells *= dims[a]; ok = cells <= MAX_CELLS; }
        }
        if (ok) break;
        cells = 0;
    }
    if (cells <= 0 || !std::isfinite(edge)) {
        roreg::set_error("roreg_icp_grid_size: no cell edge fits the bounding box");
        return 0;
    }
    memset(desc, 0, sizeof(*desc));
    for (int a = 0; a < 3; ++a) { desc->origin[a] = (n > 0 ? lo[a] : 0.0) - edge; desc->dims[a] = (int32_t)dims[a]; }
    desc->edge = edge; desc->n = n; desc->cells = cells;
    if (workspace_bytes) {
        const int64_t nb = (cells + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;
        *workspace_bytes = align_up((size_t)n * 16, 256) + align_up((size_t)nb * 4, 256);
    }
    return 64 + (size_t)n * 16 + (size_t)(cells + 2) * 4;
}

extern "C" int roreg_icp_grid_build(const float *points, const roreg_icp_grid_desc *desc, void *grid, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    ROREG_REQUIRE(desc && grid && workspace, "roreg_icp_grid_build: bad arguments");
    const GridDesc d = *desc;
    ROREG_REQUIRE(d.n >= 0 && (points || d.n == 0) && d.cells > 0 && d.cells <= MAX_CELLS && d.edge > 0.0 &&
                  (int64_t)d.dims[0] * d.dims[1] * d.dims[2] == d.cells, "roreg_icp_grid_build: bad descriptor");
    const int64_t m = d.cells + 1, nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const size_t tmp_bytes = align_up((size_t)d.n * 16, 256);
    ROREG_REQUIRE(workspace_bytes >= tmp_bytes + align_up((size_t)nb * 4, 256), "roreg_icp_grid_build: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    GridDesc *hdr = reinterpret_cast<GridDesc *>(grid);
    float4 *recs = reinterpret_cast<float4 *>(reinterpret_cast<char *>(grid) + 64);
    int32_t *starts = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(grid) + 64 + (size_t)d.n * 16);
    int32_t *S = starts + 1;
    float4 *tmp = reinterpret_cast<float4 *>(workspace);
    int32_t *bsum = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(workspace) + tmp_bytes);
    if (hipMemsetAsync(starts, 0, (size_t)(d.cells + 2) * 4, s) != hipSuccess) {
        roreg::set_error("roreg_icp_grid_build: memset failed");
        return 1;
    }
    if (d.n == 0) {
        hipLaunchKernelGGL(icp_header_kernel, dim3(1), dim3(1), 0, s, d, hdr);
        ROREG_CHECK_LAUNCH("roreg_icp_grid_build");
        return 0;
    }
    const int pb = (d.n + 255) / 256;
    hipLaunchKernelGGL(icp_hist_kernel, dim3(pb), dim3(256), 0, s, points, d, S, hdr);
    hipLaunchKernelGGL(icp_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const int32_t *)S, m, bsum);
    hipLaunchKernelGGL(icp_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, (int)nb);
    hipLaunchKernelGGL(icp_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, S, m, (const int32_t *)bsum);
    hipLaunchKernelGGL(icp_fill_kernel, dim3(pb), dim3(256), 0, s, points, d, S, tmp);
    hipLaunchKernelGGL(icp_rank_kernel, dim3(pb), dim3(256), 0, s, (const float4 *)tmp, d, (const int32_t *)starts, recs);
    ROREG_CHECK_LAUNCH("roreg_icp_grid_build");
    return 0;
}

// ---- the batch entries of the methods -------------------------------------------------------------------------------------------------------
namespace {

// workspace of a batch: the pairs' state, the first-pass slots, the second-pass slots of `second_w` words, the assignments (offsets in bytes)
struct Layout { size_t state, sums, second, assign, bytes; };

Layout layout(int n_tasks, long long total_slots, int second_w) {
    Layout L;
    size_t o = 0;
    L.state = o; o += align_up((size_t)n_tasks * sizeof(PairState), 256);
    L.sums = o; o += align_up((size_t)total_slots * SUM_W * 8, 256);
    L.second = o; o += align_up((size_t)total_slots * second_w * 8, 256);
    L.assign = o; o += align_up((size_t)total_slots * ICP_CHUNK * 4, 256);
    L.bytes = o + 256;
    return L;
}

// What distinguishes the methods on the host: the task record, the second pass (its kernel, slot width and profile slot) and the solve.
struct PointMethod {
    using Task = IcpTask;
    static constexpr const char *name = "roreg_icp_batch";
    static constexpr int pass_w = COV_W, pass_prof = -1;          // (the covariance pass has no bracket)
    static constexpr auto pass = icp_cov_kernel;
    static constexpr auto solve = icp_solve_kernel;
};
struct PlaneMethod {
    using Task = IcpPlaneTask;
    static constexpr const char *name = "roreg_icp_plane_batch";
    static constexpr int pass_w = PLANE_W, pass_prof = roreg::PROF_ICP_PLANE;
    static constexpr auto pass = icp_plane_kernel<IcpPlaneTask>;
    static constexpr auto solve = icp_plane_solve_kernel<IcpPlaneTask>;
};
struct GicpMethod {
    using Task = IcpGicpTask;
    static constexpr const char *name = "roreg_icp_gicp_batch";
    static constexpr int pass_w = PLANE_W, pass_prof = roreg::PROF_ICP_PLANE;          // (slot 7: the second pass of a normal-based method)
    static constexpr auto pass = icp_gicp_kernel<IcpGicpTask>;
    static constexpr auto solve = icp_plane_solve_kernel<IcpGicpTask>;
};
// v6p: the same two methods over the robust records; search, solve and driver are the ones above.
struct PlaneRobustMethod {
    using Task = IcpPlaneRobustTask;
    static constexpr const char *name = "roreg_icp_plane_robust_batch";
    static constexpr int pass_w = PLANE_W, pass_prof = roreg::PROF_ICP_PLANE;
    static constexpr auto pass = icp_plane_kernel<IcpPlaneRobustTask>;
    static constexpr auto solve = icp_plane_solve_kernel<IcpPlaneRobustTask>;
};
struct GicpRobustMethod {
    using Task = IcpGicpRobustTask;
    static constexpr const char *name = "roreg_icp_gicp_robust_batch";
    static constexpr int pass_w = PLANE_W, pass_prof = roreg::PROF_ICP_PLANE;
    static constexpr auto pass = icp_gicp_kernel<IcpGicpRobustTask>;
    static constexpr auto solve = icp_plane_solve_kernel<IcpGicpRobustTask>;
};

template <class M>
int icp_run(const void *tasks_dev, int n_tasks, const int32_t *work, int n_work, long long total_slots, double max_dist, int max_iter, double tol_deg,
            double tol_t, IcpOut out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes, void *stream) {
    using Task = typename M::Task;
    if (n_tasks == 0) return 0;
    ROREG_REQUIRE(tasks_dev && n_tasks > 0 && n_work >= 0 && (work || n_work == 0) && total_slots >= 0 && out.T && out.iters && out.inliers && out.rmse &&
                  out.status && workspace, "%s: bad arguments", M::name);
    ROREG_REQUIRE(max_dist > 0.0 && std::isfinite(max_dist) && max_iter >= 0, "%s: max_dist must be positive and finite, max_iter >= 0", M::name);
    const Layout L = layout(n_tasks, total_slots, M::pass_w);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "%s: workspace too small", M::name);
    hipStream_t s = roreg::as_stream(stream);
    const Task *tasks = reinterpret_cast<const Task *>(tasks_dev);
    char *w = reinterpret_cast<char *>(workspace);
    PairState *state = reinterpret_cast<PairState *>(w + L.state);
    double *sums = reinterpret_cast<double *>(w + L.sums), *second = reinterpret_cast<double *>(w + L.second);
    int32_t *assign = reinterpret_cast<int32_t *>(w + L.assign);
    const double thr2 = max_dist * max_dist, reach = max_dist * (1.0 + 1e-9);
    hipLaunchKernelGGL(icp_init_kernel<Task>, dim3((n_tasks + 63) / 64), dim3(64), 0, s, tasks, n_tasks, state, out);
    for (int it = 0; it < max_iter; ++it) {
        if (n_work > 0) {
            {
                roreg::ProfScope prof(roreg::PROF_ICP_SEARCH, s);
                hipLaunchKernelGGL(icp_search_kernel<Task>, dim3(n_work), dim3(ICP_THREADS), 0, s, tasks, n_tasks, work, (const PairState *)state, sums, assign, thr2,
                                   reach);
            }
            const bool prof = M::pass_prof >= 0 && roreg::prof_on();
            if (prof) roreg::prof_begin(M::pass_prof, s);
            hipLaunchKernelGGL(M::pass, dim3(n_work), dim3(ICP_THREADS), 0, s, tasks, n_tasks, work, (const PairState *)state, (const double *)sums, second,
                               (const int32_t *)assign);
            if (prof) roreg::prof_end(M::pass_prof, s);
        }
        hipLaunchKernelGGL(M::solve, dim3(n_tasks), dim3(64), 0, s, tasks, state, (const double *)sums, (const double *)second, it, max_iter, tol_deg, tol_t, out,
                           stats_out);
    }
    if (assign_out && n_work > 0)
        hipLaunchKernelGGL(icp_export_kernel<Task>, dim3(n_work), dim3(ICP_THREADS), 0, s, tasks, n_tasks, work, (const PairState *)state, (const int32_t *)assign,
                           assign_out);
    ROREG_CHECK_LAUNCH(M::name);
    return 0;
}

}  // namespace

extern "C" size_t roreg_icp_batch_workspace(int n_tasks, long long total_slots) {
    return n_tasks < 0 || total_slots < 0 ? 0 : layout(n_tasks, total_slots, PointMethod::pass_w).bytes;
}

extern "C" int roreg_icp_batch(const roreg_icp_task *tasks_dev, int n_tasks, const int32_t *work, int n_work, long long total_slots, double max_dist,
                               int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out, double *rmse_out,
                               int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes, void *stream) {
    return icp_run<PointMethod>(tasks_dev, n_tasks, work, n_work, total_slots, max_dist, max_iter, tol_deg, tol_t,
                                IcpOut{T_out, iters_out, inliers_out, rmse_out, status_out}, assign_out, stats_out, workspace, workspace_bytes, stream);
}

// ---- v6d entries ------------------------------------------------------------------------------------------------------------------------
extern "C" int roreg_icp_normals(const void *grid, double radius, int min_neighbors, double *out, void *stream) {
    ROREG_REQUIRE(grid && out, "roreg_icp_normals: bad arguments");
    ROREG_REQUIRE(radius > 0.0 && std::isfinite(radius) && min_neighbors >= 1, "roreg_icp_normals: radius must be positive and finite, min_neighbors >= 1");
    hipLaunchKernelGGL(icp_normals_kernel, dim3(NORMALS_BLOCKS), dim3(256), 0, roreg::as_stream(stream), grid, radius * radius, radius * (1.0 + 1e-9),
                       min_neighbors, out);
    ROREG_CHECK_LAUNCH("roreg_icp_normals");
    return 0;
}

// The plane entry's own table is read where it lies: no region for a converted copy, so this is 32 bytes per task less than it was.  (The
// lower bound that tests/test_icp_plane_oracle.py asserts at (3, 10) still counts those 32 bytes; it holds there through the 256-byte
// rounding of the regions and the 256 bytes of slack, not through the formula.)
extern "C" size_t roreg_icp_plane_batch_workspace(int n_tasks, long long total_slots) {
    return n_tasks < 0 || total_slots < 0 ? 0 : layout(n_tasks, total_slots, PlaneMethod::pass_w).bytes;
}

extern "C" int roreg_icp_plane_batch(const roreg_icp_plane_task *tasks_dev, int n_tasks, const int32_t *work, int n_work, long long total_slots,
                                     double max_dist, int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out,
                                     double *rmse_out, int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes,
                                     void *stream) {
    return icp_run<PlaneMethod>(tasks_dev, n_tasks, work, n_work, total_slots, max_dist, max_iter, tol_deg, tol_t,
                                IcpOut{T_out, iters_out, inliers_out, rmse_out, status_out}, assign_out, stats_out, workspace, workspace_bytes, stream);
}

// ---- v6i entries ------------------------------------------------------------------------------------------------------------------------
extern "C" size_t roreg_icp_gicp_batch_workspace(int n_tasks, long long total_slots) {
    return n_tasks < 0 || total_slots < 0 ? 0 : layout(n_tasks, total_slots, GicpMethod::pass_w).bytes;
}

extern "C" int roreg_icp_gicp_batch(const roreg_icp_gicp_task *tasks_dev, int n_tasks, const int32_t *work, int n_work, long long total_slots,
                                    double max_dist, int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out,
                                    double *rmse_out, int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    return icp_run<GicpMethod>(tasks_dev, n_tasks, work, n_work, total_slots, max_dist, max_iter, tol_deg, tol_t,
                               IcpOut{T_out, iters_out, inliers_out, rmse_out, status_out}, assign_out, stats_out, workspace, workspace_bytes, stream);
}

// ---- v6p entries: the plane and gicp iterations under a robust loss -------------------------------------------------------------------------
extern "C" size_t roreg_icp_plane_robust_batch_workspace(int n_tasks, long long total_slots) {
    return n_tasks < 0 || total_slots < 0 ? 0 : layout(n_tasks, total_slots, PlaneRobustMethod::pass_w).bytes;
}

extern "C" int roreg_icp_plane_robust_batch(const roreg_icp_plane_robust_task *tasks_dev, int n_tasks, const int32_t *work, int n_work, long long total_slots,
                                            double max_dist, int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out,
                                            int32_t *inliers_out, double *rmse_out, int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace,
                                            size_t workspace_bytes, void *stream) {
    return icp_run<PlaneRobustMethod>(tasks_dev, n_tasks, work, n_work, total_slots, max_dist, max_iter, tol_deg, tol_t,
                                      IcpOut{T_out, iters_out, inliers_out, rmse_out, status_out}, assign_out, stats_out, workspace, workspace_bytes, stream);
}

extern "C" size_t roreg_icp_gicp_robust_batch_workspace(int n_tasks, long long total_slots) {
    return n_tasks < 0 || total_slots < 0 ? 0 : layout(n_tasks, total_slots, GicpRobustMethod::pass_w).bytes;
}

extern "C" int roreg_icp_gicp_robust_batch(const roreg_icp_gicp_robust_task *tasks_dev, int n_tasks, const int32_t *work, int n_work, long long total_slots,
                                           double max_dist, int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out,
                                           int32_t *inliers_out, double *rmse_out, int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace,
                                           size_t workspace_bytes, void *stream) {
    return icp_run<GicpRobustMethod>(tasks_dev, n_tasks, work, n_work, total_slots, max_dist, max_iter, tol_deg, tol_t,
                                     IcpOut{T_out, iters_out, inliers_out, rmse_out, status_out}, assign_out, stats_out, workspace, workspace_bytes, stream);
}

// ---- v6g entries ------------------------------------------------------------------------------------------------------------------------
// workspace of an evaluation: the slots, at offset 0
static size_t eval_layout(long long total_slots) { return align_up((size_t)total_slots * EVAL_W * 8, 256) + 256; }

extern "C" size_t roreg_icp_eval_workspace(int n_pairs, long long total_slots) { return n_pairs < 0 || total_slots < 0 ? 0 : eval_layout(total_slots); }

extern "C" int roreg_icp_eval_batch(const roreg_icp_task *tasks_dev, int n_pairs, const int32_t *work, int n_work, long long total_slots, double max_dist,
                                    double *stats_out, double *info_out, int32_t *status_out, int32_t *assign_out, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    if (n_pairs == 0) return 0;
    ROREG_REQUIRE(tasks_dev && n_pairs > 0 && n_pairs <= (1 << 30) && n_work >= 0 && (work || n_work == 0) && total_slots >= 0 && stats_out && info_out &&
                  status_out && workspace, "roreg_icp_eval_batch: bad arguments");
    ROREG_REQUIRE(max_dist > 0.0 && std::isfinite(max_dist), "roreg_icp_eval_batch: max_dist must be positive and finite");
    ROREG_REQUIRE(workspace_bytes >= eval_layout(total_slots), "roreg_icp_eval_batch: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    const IcpTask *tasks = reinterpret_cast<const IcpTask *>(tasks_dev);
    double *sums = reinterpret_cast<double *>(workspace);
    if (n_work > 0)
        hipLaunchKernelGGL(icp_eval_kernel, dim3(n_work), dim3(ICP_THREADS), 0, s, tasks, n_pairs, work, sums, assign_out, max_dist * max_dist,
                           max_dist * (1.0 + 1e-9));
    hipLaunchKernelGGL(icp_eval_finish_kernel, dim3(n_pairs), dim3(64), 0, s, tasks, n_pairs, (const double *)sums, stats_out, info_out, status_out);
    ROREG_CHECK_LAUNCH("roreg_icp_eval_batch");
    return 0;
}
