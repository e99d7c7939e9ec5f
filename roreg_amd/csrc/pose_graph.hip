// Multiway registration on the device: batched Levenberg-Marquardt optimisation of pose graphs (include/roreg_hip.h, "v6h";
// tests/_pose_graph_oracle.py is the numpy restatement).  Everything is float64; the small formulas live in pg_math.h.
//
//   init      : one workgroup per graph.  Without given poses, thread 0 composes the measured transforms along the walk order the host
//               computed (topology is the host's, arithmetic the device's); every input is tested for finiteness; the starting cost.
//   per round : linearise -- one lane per edge writes a 56-double record (e, chi2, w, RE, Q, A, B, D: the Jacobians' structure, not 72 free
//               doubles);  assemble -- one workgroup per (graph, optimised node) owns that node's block row of H's lower triangle and its
//               six entries of g, adds its incident edges in ascending edge index (the larger node owns an off-diagonal block);  solve --
//               one workgroup per graph: damping, in-place blocked Cholesky of the lower triangle (32-wide panels: the diagonal block
//               factored in LDS, the panel by forward substitution with one row per thread, the trailing update in 64 x 64 tiles whose two
//               panel slices are staged in LDS), two blocked triangular solves, the candidate poses, their cost and the decision.
//   finish    : chi2 and weight of every edge at the final poses, the final cost, iterations and status.
// All rounds are enqueued at once; a per-graph `done` word makes the workgroups of a finished graph return at once (roreg_icp_batch's
// scheme).  No floating-point atomics: every sum has one owner and a fixed order, and nothing a graph computes depends on the other graphs
// of the call, so its bits do not depend on the batch or on its place in it.
#include "common.h"
#include <algorithm>
#include <cmath>
#include "pg_math.h"

#pragma clang fp contract(off)

namespace {

constexpr int PG_MAX_NODES = 256, PG_MAX_EDGES = 65536;
constexpr int PG_LIN = 56;                    // doubles per edge record: e 0..5, chi2 6, w 7, RE 8, Q 17, A 26, B 35, D 44, 53..55 unused
constexpr int PG_NB = 32;                     // Cholesky panel width
constexpr int PG_LDS_LD = PG_NB + 1;          // leading dimension of the LDS blocks: odd, so that rows fall into different banks
constexpr int PG_TILE = 64;                   // rows per trailing-update tile
constexpr int PG_THREADS = 256;
constexpr int PG_MAX_N = 6 * (PG_MAX_NODES - 1);
enum { ST_CONVERGED = 0, ST_MAX_ITER = 1, ST_STALLED = 2, ST_NONFINITE = 3 };
enum { DEC_NONE = 0, DEC_ACCEPT = 1, DEC_REJECT = 2, DEC_PIVOT = 3, DEC_STOP = 4 };

struct Tables {
    const roreg_pg_graph *graphs;
    const int32_t *edge_i, *edge_j, *edge_graph;          // [E_total]: local node numbers, the edge's graph
    const double *T, *Lam;                                // [E_total,16], [E_total,36]
    const int32_t *var;                                   // [C_total]: the node's block in its graph's system, -1 = not optimised
    const int32_t *inc_ptr, *inc_edge;                    // [C_total + 1], [2 E_total]: incident edges (numbers in the whole table), ascending
    const int32_t *act_graph, *act_node;                  // [A_total]: the optimised nodes, graph after graph in ascending node
    const int32_t *walk;                                  // [A_total,2]: (node, edge) in the order the initial poses are composed
};

struct Work {
    double *lin, *H, *g, *delta, *cand, *state;           // state [G,4] = (c, lambda, c0, -)
    int32_t *flags;                                       // [G,4] = (done, iters, status, -)
};

struct Layout { size_t lin, H, g, delta, cand, state, flags, bytes; };

Layout layout(int G, size_t n_nodes, size_t n_edges, size_t n_act, size_t h_doubles) {
    Layout L;
    size_t o = 0;
    L.lin = o; o += align_up(n_edges * PG_LIN * 8, 256);
    L.H = o; o += align_up(h_doubles * 8, 256);
    L.g = o; o += align_up(n_act * 6 * 8, 256);
    L.delta = o; o += align_up(n_act * 6 * 8, 256);
    L.cand = o; o += align_up(n_nodes * 16 * 8, 256);
    L.state = o; o += align_up((size_t)G * 4 * 8, 256);
    L.flags = o; o += align_up((size_t)G * 4 * 4, 256);
    L.bytes = o;
    return L;
}

// host-side check of the descriptors and the totals they imply; false = a limit is exceeded or the table is inconsistent
bool totals(const roreg_pg_graph *gh, int G, size_t &n_nodes, size_t &n_edges, size_t &n_act, size_t &h_doubles, int &max_edges) {
    n_nodes = n_edges = n_act = h_doubles = 0; max_edges = 0;
    for (int b = 0; b < G; ++b) {
        const roreg_pg_graph &g = gh[b];
        if (g.n_nodes < 1 || g.n_nodes > PG_MAX_NODES || g.n_edges < 0 || g.n_edges > PG_MAX_EDGES) return false;
        if (g.n_act < 0 || g.n_act > g.n_nodes - 1 || g.anchor < 0 || g.anchor >= g.n_nodes) return false;
        if ((size_t)g.node0 != n_nodes || (size_t)g.edge0 != n_edges || (size_t)g.act0 != n_act || (size_t)g.h0 != h_doubles) return false;
        n_nodes += (size_t)g.n_nodes; n_edges += (size_t)g.n_edges; n_act += (size_t)g.n_act;
        h_doubles += (size_t)(6 * g.n_act) * (size_t)(6 * g.n_act);
        max_edges = std::max(max_edges, g.n_edges);
    }
    return true;
}

struct BlockSync { __device__ __forceinline__ void operator()() const { __syncthreads(); } };

__device__ __forceinline__ bool reached(const roreg_pg_graph &g, const int32_t *var, int c) { return c == g.anchor || var[g.node0 + c] >= 0; }

// chi2, rho and w of edge k (number in the whole table) at the poses P ([n_nodes,16] of its graph); an edge whose ends are not both reached from
// the anchor, or whose node numbers are out of range, contributes nothing (w = 0)
__device__ __forceinline__ void edge_cost(const roreg_pg_graph &g, const Tables &t, const double *P, int k, double &chi2, double &rho, double &w) {
    const int i = t.edge_i[k], j = t.edge_j[k];
    chi2 = 0.0; rho = 0.0; w = 0.0;
    if (i < 0 || j < 0 || i >= g.n_nodes || j >= g.n_nodes || i == j) return;
    double Rm[9], tm[3], RE[9], e[6], q[4];
    pg_math::edge_error(P + (size_t)i * 16, P + (size_t)j * 16, t.T + (size_t)k * 16, Rm, tm, RE, e, q);
    const double *Lam = t.Lam + (size_t)k * 36;
    chi2 = pg_math::chi2_of(e, Lam);
    if (reached(g, t.var, i) && reached(g, t.var, j)) pg_math::robust(chi2, Lam[0], g.tau, rho, w);
}

// The graph's cost at P by the whole workgroup: thread t adds its edges t, t + 256, ... in ascending order, then a fixed tree over the 256
// partial sums.  Every thread returns the same value.  red: 256 doubles of LDS.
__device__ double graph_cost(const roreg_pg_graph &g, const Tables &t, const double *P, double *red, double *chi2_out, double *w_out) {
    double s = 0.0;
    for (int k = threadIdx.x; k < g.n_edges; k += PG_THREADS) {
        double chi2, rho, w;
        edge_cost(g, t, P, g.edge0 + k, chi2, rho, w);
        s += rho;
        if (chi2_out) { chi2_out[g.edge0 + k] = chi2; w_out[g.edge0 + k] = w; }
    }
    __syncthreads();
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = PG_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double c = red[0];
    __syncthreads();
    return c;
}

__global__ __launch_bounds__(PG_THREADS) void pg_init_kernel(Tables t, Work wk, double *__restrict__ poses, int has_init, double *__restrict__ cost_out) {
    __shared__ double red[PG_THREADS];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const roreg_pg_graph g = t.graphs[b];
    double *P = poses + (size_t)g.node0 * 16;
    if (tid == 0) bad = 0;
    if (!has_init) {
        for (int k = tid; k < g.n_nodes * 16; k += PG_THREADS) P[k] = ((k % 16) % 5 == 0) ? 1.0 : 0.0;
        __syncthreads();
        if (tid == 0) {
            for (int s = 0; s < g.n_act; ++s) {
                const int node = t.walk[2 * (size_t)(g.act0 + s)], k = t.walk[2 * (size_t)(g.act0 + s) + 1];
                if (node < 0 || node >= g.n_nodes || k < g.edge0 || k >= g.edge0 + g.n_edges) continue;
                const int i = t.edge_i[k], j = t.edge_j[k];
                if (i < 0 || j < 0 || i >= g.n_nodes || j >= g.n_nodes) continue;
                const bool fwd = (j == node);                          // P_j = P_i T_k, else P_i = P_j T_k^-1
                double Pc[16];
                pg_math::pose_compose(P + (size_t)(fwd ? i : j) * 16, t.T + (size_t)k * 16, !fwd, Pc);
                for (int q = 0; q < 16; ++q) P[(size_t)node * 16 + q] = Pc[q];
            }
        }
    }
    __syncthreads();
    int nf = 0;
    for (int k = tid; k < g.n_nodes * 16; k += PG_THREADS) nf |= !isfinite(P[k]);
    for (int k = tid; k < g.n_edges * 16; k += PG_THREADS) nf |= !isfinite(t.T[(size_t)g.edge0 * 16 + k]);
    for (int k = tid; k < g.n_edges * 36; k += PG_THREADS) nf |= !isfinite(t.Lam[(size_t)g.edge0 * 36 + k]);
    if (tid == 0) nf |= !(isfinite(g.tau) && isfinite(g.lambda0) && isfinite(g.tol_t) && isfinite(g.tol_rot) && isfinite(g.tol_cost));
    if (nf) bad = 1;
    __syncthreads();
    const double c0 = graph_cost(g, t, P, red, nullptr, nullptr);
    if (tid == 0) {
        const bool stop = bad || !isfinite(c0);
        wk.state[4 * b] = c0; wk.state[4 * b + 1] = g.lambda0; wk.state[4 * b + 2] = c0; wk.state[4 * b + 3] = 0.0;
        wk.flags[4 * b] = stop; wk.flags[4 * b + 1] = 0; wk.flags[4 * b + 2] = stop ? ST_NONFINITE : ST_MAX_ITER; wk.flags[4 * b + 3] = 0;
        cost_out[2 * b] = stop ? (double)NAN : c0;
    }
}

__global__ __launch_bounds__(PG_THREADS) void pg_linearise_kernel(Tables t, Work wk, const double *__restrict__ poses, int n_edges_total) {
    const int k = blockIdx.x * PG_THREADS + threadIdx.x;
    if (k >= n_edges_total) return;
    const int b = t.edge_graph[k];
    if (wk.flags[4 * b]) return;
    const roreg_pg_graph &g = t.graphs[b];
    double *rec = wk.lin + (size_t)k * PG_LIN;
    const int i = t.edge_i[k], j = t.edge_j[k];
    if (i < 0 || j < 0 || i >= g.n_nodes || j >= g.n_nodes || i == j) { rec[6] = 0.0; rec[7] = 0.0; return; }
    const double *P = poses + (size_t)g.node0 * 16;
    double Rm[9], tm[3], RE[9], e[6], q[4], Q[9], A[9], B[9], D[9];
    pg_math::edge_error(P + (size_t)i * 16, P + (size_t)j * 16, t.T + (size_t)k * 16, Rm, tm, RE, e, q);
    const double *Lam = t.Lam + (size_t)k * 36;
    const double chi2 = pg_math::chi2_of(e, Lam);
    double rho = 0.0, w = 0.0;
    if (reached(g, t.var, i) && reached(g, t.var, j)) pg_math::robust(chi2, Lam[0], g.tau, rho, w);
    pg_math::edge_jacobians(Rm, tm, RE, q, Q, A, B, D);
#pragma unroll
    for (int c = 0; c < 6; ++c) rec[c] = e[c];
    rec[6] = chi2; rec[7] = w;
#pragma unroll
    for (int c = 0; c < 9; ++c) { rec[8 + c] = RE[c]; rec[17 + c] = Q[c]; rec[26 + c] = A[c]; rec[35 + c] = B[c]; rec[44 + c] = D[c]; }
}

// One wave per optimised node a: block row `va` of the lower triangle of H = sum_k w_k J_k^T Lambda_k J_k and g_a = sum_k w_k J_a^T Lambda_k e_k.
__global__ __launch_bounds__(64) void pg_assemble_kernel(Tables t, Work wk) {
    __shared__ double sJa[36], sJb[36], sLam[36], sLJa[36], sLJb[36], se[6], sLe[6];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int b = t.act_graph[s];
    if (wk.flags[4 * b]) return;
    const roreg_pg_graph g = t.graphs[b];
    const int a = t.act_node[s];
    if (a < 0 || a >= g.n_nodes) return;
    const int va = t.var[g.node0 + a];
    if (va < 0 || va >= g.n_act) return;
    const int n = 6 * g.n_act;
    double *H = wk.H + g.h0, *gv = wk.g + (size_t)g.act0 * 6;
    const int width = 6 * va + 6;
    for (int k = tid; k < 6 * width; k += 64) H[(size_t)(6 * va + k / width) * n + k % width] = 0.0;
    __syncthreads();
    const int r = tid / 6, c = tid % 6;
    double dg = 0.0, gacc = 0.0;
    const int t0 = t.inc_ptr[g.node0 + a], t1 = t.inc_ptr[g.node0 + a + 1];
    for (int q = t0; q < t1; ++q) {
        const int k = t.inc_edge[q];
        if (k < g.edge0 || k >= g.edge0 + g.n_edges) continue;
        const double *rec = wk.lin + (size_t)k * PG_LIN;
        const double w = rec[7];
        const int i = t.edge_i[k], j = t.edge_j[k];
        if (!(w != 0.0) || (i != a && j != a) || i == j || i < 0 || j < 0 || i >= g.n_nodes || j >= g.n_nodes) continue;       // (uniform over the wave)
        const bool a_is_j = (j == a);
        const int vb = t.var[g.node0 + (a_is_j ? i : j)];
        if (tid < 36) {
            sJa[tid] = pg_math::dense_J(rec + 8, rec + 17, rec + 26, rec + 35, rec + 44, a_is_j, r, c);
            sJb[tid] = pg_math::dense_J(rec + 8, rec + 17, rec + 26, rec + 35, rec + 44, !a_is_j, r, c);
            sLam[tid] = t.Lam[(size_t)k * 36 + tid];
            if (tid < 6) se[tid] = rec[tid];
        }
        __syncthreads();
        if (tid < 36) {
            double x = sLam[r * 6] * sJa[c], y = sLam[r * 6] * sJb[c];
            for (int p = 1; p < 6; ++p) { x += sLam[r * 6 + p] * sJa[p * 6 + c]; y += sLam[r * 6 + p] * sJb[p * 6 + c]; }
            sLJa[tid] = x; sLJb[tid] = y;
            if (tid < 6) {
                double z = sLam[tid * 6] * se[0];
                for (int p = 1; p < 6; ++p) z += sLam[tid * 6 + p] * se[p];
                sLe[tid] = z;
            }
        }
        __syncthreads();
        if (tid < 36) {
            double x = sJa[r] * sLJa[c];
            for (int p = 1; p < 6; ++p) x += sJa[p * 6 + r] * sLJa[p * 6 + c];
            dg += w * x;
            if (vb >= 0 && vb < va) {
                double y = sJa[r] * sLJb[c];
                for (int p = 1; p < 6; ++p) y += sJa[p * 6 + r] * sLJb[p * 6 + c];
                H[(size_t)(6 * va + r) * n + 6 * vb + c] += w * y;
            }
            if (tid < 6) {
                double z = sJa[tid] * sLe[0];
                for (int p = 1; p < 6; ++p) z += sJa[p * 6 + tid] * sLe[p];
                gacc += w * z;
            }
        }
        __syncthreads();
    }
    if (tid < 36) H[(size_t)(6 * va + r) * n + 6 * va + c] = dg;
    if (tid < 6) gv[6 * va + tid] = gacc;
}

// In-place blocked Cholesky of the lower triangle of the n x n matrix H (row-major, ld = n) by the workgroup; false = a bad pivot.
// sI: 128 x 33 doubles of LDS (the panel stage; its two halves are the trailing update's two slices), sD: 32 x 33.
__device__ bool chol_blocked(double *H, int n, double *sD, double *sI) {
    const int tid = threadIdx.x;
    double *sJ = sI + PG_TILE * PG_LDS_LD;
    for (int k0 = 0; k0 < n; k0 += PG_NB) {
        const int kb = min(PG_NB, n - k0);
        for (int idx = tid; idx < PG_NB * PG_NB; idx += PG_THREADS) {
            const int r = idx / PG_NB, c = idx % PG_NB;
            sD[r * PG_LDS_LD + c] = (r < kb && c <= r) ? H[(size_t)(k0 + r) * n + k0 + c] : (r == c ? 1.0 : 0.0);
        }
        __syncthreads();
        if (!pg_math::chol_lower(sD, kb, PG_LDS_LD, tid, PG_THREADS, BlockSync())) return false;
        for (int idx = tid; idx < PG_NB * PG_NB; idx += PG_THREADS) {
            const int r = idx / PG_NB, c = idx % PG_NB;
            if (r < kb && c <= r) H[(size_t)(k0 + r) * n + k0 + c] = sD[r * PG_LDS_LD + c];
        }
        const int r0 = k0 + kb;
        // the panel below the block: row i of L21 = row i of A21 L11^-T, 128 rows at a time staged in LDS, one row per thread
        __syncthreads();
        for (int c0 = r0; c0 < n; c0 += 2 * PG_TILE) {
            for (int idx = tid; idx < 2 * PG_TILE * PG_NB; idx += PG_THREADS) {
                const int r = idx / PG_NB, c = idx % PG_NB;
                if (c0 + r < n && c < kb) sI[r * PG_LDS_LD + c] = H[(size_t)(c0 + r) * n + k0 + c];
            }
            __syncthreads();
            if (tid < 2 * PG_TILE && c0 + tid < n) {
                double *x = sI + tid * PG_LDS_LD;
                for (int j = 0; j < kb; ++j) {
                    double sacc = x[j];
                    for (int p = 0; p < j; ++p) sacc -= x[p] * sD[j * PG_LDS_LD + p];
                    x[j] = sacc / sD[j * PG_LDS_LD + j];
                }
            }
            __syncthreads();
            for (int idx = tid; idx < 2 * PG_TILE * PG_NB; idx += PG_THREADS) {
                const int r = idx / PG_NB, c = idx % PG_NB;
                if (c0 + r < n && c < kb) H[(size_t)(c0 + r) * n + k0 + c] = sI[r * PG_LDS_LD + c];
            }
            __syncthreads();
        }
        // trailing update A22 -= L21 L21^T on the lower triangle, in 64 x 64 tiles; thread (ti, tj) owns rows ti + 16 a, columns tj + 16 b
        const int ti = tid / 16, tj = tid % 16;
        for (int I0 = r0; I0 < n; I0 += PG_TILE) {
            for (int idx = tid; idx < PG_TILE * PG_NB; idx += PG_THREADS) {
                const int r = idx / PG_NB, c = idx % PG_NB;
                sI[r * PG_LDS_LD + c] = (I0 + r < n && c < kb) ? H[(size_t)(I0 + r) * n + k0 + c] : 0.0;
            }
            for (int J0 = r0; J0 <= I0; J0 += PG_TILE) {
                __syncthreads();
                for (int idx = tid; idx < PG_TILE * PG_NB; idx += PG_THREADS) {
                    const int r = idx / PG_NB, c = idx % PG_NB;
                    sJ[r * PG_LDS_LD + c] = (J0 + r < n && c < kb) ? H[(size_t)(J0 + r) * n + k0 + c] : 0.0;
                }
                __syncthreads();
                double acc[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int bb = 0; bb < 4; ++bb) acc[a][bb] = 0.0;
                for (int p = 0; p < PG_NB; ++p) {
                    double li[4], lj[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) { li[a] = sI[(ti + 16 * a) * PG_LDS_LD + p]; lj[a] = sJ[(tj + 16 * a) * PG_LDS_LD + p]; }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int bb = 0; bb < 4; ++bb) acc[a][bb] += li[a] * lj[bb];
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int bb = 0; bb < 4; ++bb) {
                        const int i = I0 + ti + 16 * a, j = J0 + tj + 16 * bb;
                        if (i < n && j <= i) H[(size_t)i * n + j] -= acc[a][bb];
                    }
            }
            __syncthreads();
        }
    }
    return true;
}

// x <- L^-T L^-1 x for the factor in H's lower triangle, x [n] in LDS, by the workgroup in 32-wide blocks
__device__ void chol_solve(const double *H, int n, double *x, double *sD) {
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < n; k0 += PG_NB) {
        const int kb = min(PG_NB, n - k0);
        for (int idx = tid; idx < kb * kb; idx += PG_THREADS) {
            const int r = idx / kb, c = idx % kb;
            if (c <= r) sD[r * PG_LDS_LD + c] = H[(size_t)(k0 + r) * n + k0 + c];
        }
        __syncthreads();
        if (tid == 0) pg_math::trsv_lower(sD, kb, PG_LDS_LD, x + k0);
        __syncthreads();
        for (int i = k0 + kb + tid; i < n; i += PG_THREADS) {
            const double *row = H + (size_t)i * n + k0;
            double s = x[i];
            for (int p = 0; p < kb; ++p) s -= row[p] * x[k0 + p];
            x[i] = s;
        }
        __syncthreads();
    }
    for (int k0 = (n - 1) / PG_NB * PG_NB; k0 >= 0; k0 -= PG_NB) {
        const int kb = min(PG_NB, n - k0);
        for (int idx = tid; idx < kb * kb; idx += PG_THREADS) {
            const int r = idx / kb, c = idx % kb;
            if (c <= r) sD[r * PG_LDS_LD + c] = H[(size_t)(k0 + r) * n + k0 + c];
        }
        __syncthreads();
        if (tid == 0) pg_math::trsv_lower_t(sD, kb, PG_LDS_LD, x + k0);
        __syncthreads();
        for (int j = tid; j < k0; j += PG_THREADS) {
            double s = x[j];
            for (int p = 0; p < kb; ++p) s -= H[(size_t)(k0 + p) * n + j] * x[k0 + p];
            x[j] = s;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PG_THREADS) void pg_solve_kernel(Tables t, Work wk, double *__restrict__ poses, int max_iter, double *__restrict__ history) {
    __shared__ double sD[PG_NB * PG_LDS_LD], sI[2 * PG_TILE * PG_LDS_LD], sx[PG_MAX_N + 6], red[PG_THREADS];
    __shared__ int big_step, take;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (wk.flags[4 * b]) return;
    const roreg_pg_graph g = t.graphs[b];
    const int n = 6 * g.n_act;
    double *H = wk.H + g.h0;
    const double *gv = wk.g + (size_t)g.act0 * 6;
    double *dv = wk.delta + (size_t)g.act0 * 6;
    double *P = poses + (size_t)g.node0 * 16, *cand = wk.cand + (size_t)g.node0 * 16;
    const double c = wk.state[4 * b], lam = wk.state[4 * b + 1];
    const int it = wk.flags[4 * b + 1];
    if (tid == 0) { big_step = 0; take = 0; }
    for (int d = tid; d < n; d += PG_THREADS) {
        const double h = H[(size_t)d * n + d];
        H[(size_t)d * n + d] = h + lam * h;
    }
    __syncthreads();
    const bool ok = chol_blocked(H, n, sD, sI);
    __syncthreads();
    double c1 = NAN;
    if (ok) {
        for (int d = tid; d < n; d += PG_THREADS) sx[d] = -gv[d];
        __syncthreads();
        chol_solve(H, n, sx, sD);
        for (int d = tid; d < n; d += PG_THREADS) dv[d] = sx[d];
        for (int node = tid; node < g.n_nodes; node += PG_THREADS) {
            const int v = t.var[g.node0 + node];
            if (v >= 0 && v < g.n_act) {
                const double *d = sx + 6 * v;
                const double nv = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), nw = sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
                if (!(nv <= g.tol_t && nw <= g.tol_rot)) big_step = 1;
                double dl[6], Pn[16];
                for (int q = 0; q < 6; ++q) dl[q] = d[q];
                pg_math::pose_update(P + (size_t)node * 16, dl, Pn);
                for (int q = 0; q < 16; ++q) cand[(size_t)node * 16 + q] = Pn[q];
            } else {
                for (int q = 0; q < 16; ++q) cand[(size_t)node * 16 + q] = P[(size_t)node * 16 + q];
            }
        }
        __syncthreads();
        c1 = graph_cost(g, t, cand, red, nullptr, nullptr);
    }
    if (tid == 0) {
        int dec;
        double lam_next = lam, c_next = c;
        int done = 0, status = ST_MAX_ITER;
        if (!ok) dec = DEC_PIVOT;
        else if (!big_step || fabs(c - c1) <= g.tol_cost * c) dec = DEC_STOP;
        else if (c1 < c) dec = DEC_ACCEPT;
        else dec = DEC_REJECT;
        if (dec == DEC_STOP) { c_next = c1; done = 1; status = ST_CONVERGED; }
        else if (dec == DEC_ACCEPT) { c_next = c1; lam_next = fmax(lam / 10.0, 1e-12); }
        else {
            lam_next = 10.0 * lam;
            if (lam_next > 1e12) { done = 1; status = ST_STALLED; }
        }
        if (it >= 0 && it < max_iter) {
            double *hrow = history + ((size_t)b * max_iter + it) * 4;
            hrow[0] = c; hrow[1] = c1; hrow[2] = lam; hrow[3] = (double)dec;
        }
        wk.state[4 * b] = c_next; wk.state[4 * b + 1] = lam_next;
        wk.flags[4 * b + 1] = it + 1; wk.flags[4 * b + 2] = status; wk.flags[4 * b] = done;
        take = (dec == DEC_STOP || dec == DEC_ACCEPT);
    }
    __syncthreads();
    if (take)
        for (int k = tid; k < g.n_nodes * 16; k += PG_THREADS) P[k] = cand[k];
}

__global__ __launch_bounds__(PG_THREADS) void pg_finish_kernel(Tables t, Work wk, const double *__restrict__ poses, double *__restrict__ cost_out,
                                                               int32_t *__restrict__ iters_out, int32_t *__restrict__ status_out,
                                                               double *__restrict__ chi2_out, double *__restrict__ w_out) {
    __shared__ double red[PG_THREADS];
    const int b = blockIdx.x;
    const roreg_pg_graph g = t.graphs[b];
    const double c = graph_cost(g, t, poses + (size_t)g.node0 * 16, red, chi2_out, w_out);
    if (threadIdx.x == 0) {
        const int status = wk.flags[4 * b + 2];
        cost_out[2 * b + 1] = status == ST_NONFINITE ? (double)NAN : c;
        iters_out[b] = wk.flags[4 * b + 1];
        status_out[b] = status;
    }
}

}  // namespace

extern "C" size_t roreg_pg_workspace(const roreg_pg_graph *graphs_host, int n_graphs) {
    size_t n_nodes, n_edges, n_act, h_doubles;
    int max_edges;
    if (n_graphs < 0 || (n_graphs && !graphs_host) || !totals(graphs_host, n_graphs, n_nodes, n_edges, n_act, h_doubles, max_edges)) return 0;
    return layout(n_graphs, n_nodes, n_edges, n_act, h_doubles).bytes;
}

extern "C" int roreg_pg_optimize_batch(const roreg_pg_graph *graphs_host, const roreg_pg_graph *graphs, int n_graphs, const int32_t *edge_i,
                                       const int32_t *edge_j, const int32_t *edge_graph, const double *transforms, const double *infos,
                                       const int32_t *var, const int32_t *inc_ptr, const int32_t *inc_edge, const int32_t *act_graph,
                                       const int32_t *act_node, const int32_t *walk, int has_init, int max_iter, double *poses, double *cost_out,
                                       int32_t *iters_out, int32_t *status_out, double *weights_out, double *chi2_out, double *history_out,
                                       double *lin_out, double *H_out, double *gd_out, void *workspace, size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(n_graphs >= 0 && max_iter >= 0 && max_iter <= 100000, "roreg_pg_optimize_batch: bad arguments");
    if (n_graphs == 0) return 0;
    ROREG_REQUIRE(graphs_host && graphs, "roreg_pg_optimize_batch: bad arguments");
    size_t n_nodes, n_edges, n_act, h_doubles;
    int max_edges;
    ROREG_REQUIRE(totals(graphs_host, n_graphs, n_nodes, n_edges, n_act, h_doubles, max_edges),
                  "roreg_pg_optimize_batch: a graph exceeds %d nodes or %d edges, or the descriptor table is inconsistent", PG_MAX_NODES, PG_MAX_EDGES);
    ROREG_REQUIRE(n_edges <= 0x7fffffffu / PG_LIN && n_nodes <= 0x7fffffffu / 16, "roreg_pg_optimize_batch: the batch is too large");
    ROREG_REQUIRE(var && inc_ptr && poses && cost_out && iters_out && status_out && workspace && (max_iter == 0 || history_out),
                  "roreg_pg_optimize_batch: bad arguments");
    ROREG_REQUIRE(n_edges == 0 || (edge_i && edge_j && edge_graph && transforms && infos && inc_edge && weights_out && chi2_out),
                  "roreg_pg_optimize_batch: bad arguments");
    ROREG_REQUIRE(n_act == 0 || (act_graph && act_node && walk), "roreg_pg_optimize_batch: bad arguments");
    const Layout L = layout(n_graphs, n_nodes, n_edges, n_act, h_doubles);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "roreg_pg_optimize_batch: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    char *w = reinterpret_cast<char *>(workspace);
    Tables t{graphs, edge_i, edge_j, edge_graph, transforms, infos, var, inc_ptr, inc_edge, act_graph, act_node, walk};
    Work wk{reinterpret_cast<double *>(w + L.lin), reinterpret_cast<double *>(w + L.H), reinterpret_cast<double *>(w + L.g),
            reinterpret_cast<double *>(w + L.delta), reinterpret_cast<double *>(w + L.cand), reinterpret_cast<double *>(w + L.state),
            reinterpret_cast<int32_t *>(w + L.flags)};
    if (max_iter && hipMemsetAsync(history_out, 0, (size_t)n_graphs * max_iter * 4 * 8, s) != hipSuccess) {
        roreg::set_error("roreg_pg_optimize_batch: memset failed");
        return 1;
    }
    hipLaunchKernelGGL(pg_init_kernel, dim3(n_graphs), dim3(PG_THREADS), 0, s, t, wk, poses, has_init, cost_out);
    const unsigned eb = (unsigned)((n_edges + PG_THREADS - 1) / PG_THREADS);
    for (int it = 0; it < max_iter; ++it) {
        if (n_edges) hipLaunchKernelGGL(pg_linearise_kernel, dim3(eb), dim3(PG_THREADS), 0, s, t, wk, (const double *)poses, (int)n_edges);
        if (n_act) hipLaunchKernelGGL(pg_assemble_kernel, dim3((unsigned)n_act), dim3(64), 0, s, t, wk);
        if (it == 0) {
            bool okc = true;
            if (lin_out && n_edges) okc = okc && hipMemcpyAsync(lin_out, wk.lin, n_edges * PG_LIN * 8, hipMemcpyDeviceToDevice, s) == hipSuccess;
            if (H_out && h_doubles) okc = okc && hipMemcpyAsync(H_out, wk.H, h_doubles * 8, hipMemcpyDeviceToDevice, s) == hipSuccess;
            if (gd_out && n_act) okc = okc && hipMemcpyAsync(gd_out, wk.g, n_act * 6 * 8, hipMemcpyDeviceToDevice, s) == hipSuccess;
            if (!okc) { roreg::set_error("roreg_pg_optimize_batch: copy failed"); return 1; }
        }
        {
            roreg::ProfScope ps(roreg::PROF_PG_SOLVE, s);
            hipLaunchKernelGGL(pg_solve_kernel, dim3(n_graphs), dim3(PG_THREADS), 0, s, t, wk, poses, max_iter, history_out);
        }
        if (it == 0 && gd_out && n_act &&
            hipMemcpyAsync(gd_out + n_act * 6, wk.delta, n_act * 6 * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            roreg::set_error("roreg_pg_optimize_batch: copy failed");
            return 1;
        }
    }
    hipLaunchKernelGGL(pg_finish_kernel, dim3(n_graphs), dim3(PG_THREADS), 0, s, t, wk, (const double *)poses, cost_out, iters_out, status_out, chi2_out,
                       weights_out);
    ROREG_CHECK_LAUNCH("roreg_pg_optimize_batch");
    return 0;
}
