// Spatial-compatibility hypotheses (tests/_sc2_oracle.py restates the definition in numpy): per pair, from the matched
// keypoints alone -- no network, no random draws --
//   C_ij = [i != j and |‖P_i - P_j‖ - ‖Q_i - Q_j‖| <= tau]          stored as M rows of ceil(M / 64) 64-bit words (bit j % 64 of word j / 64)
//   deg_i = popcount(row i);  seeds = the S = min(M, max_seeds) rows of greatest degree, ties to the lower index
//   N2[s, j] = C[s, j] * popcount(row s AND row j)                  (C is symmetric, so this is C[s, j] * (C C)[s, j])
//   set(s) = s, then at most K - 1 of its compatible j by greater N2, ties to the lower j;  hypothesis = Kabsch fit P ~ R Q + t over the set
// Six launches per call, whatever the number of pairs: gather, compatibility, degree, rank, second order, selection + fit.
// The distances follow the oracle's operation order (no FMA contraction) and every float64 sum has a fixed order (no float atomics).
#include "common.h"
#include "primitives.h"

#pragma clang fp contract(off)
#include "polar.h"          // polar_proper: the proper rotation nearest a 3x3 cross-covariance

namespace {

constexpr int SEED_TILE = ROREG_SC2_SEED_TILE, COL_TILE = ROREG_SC2_COL_TILE;   // the second-order kernel's tile of seed rows x column rows
constexpr int WORD_CHUNK = 16;                                                  // 64-bit words of every tile row staged in LDS per step
constexpr int MAX_M = ROREG_SC2_MAX_M;                                          // the rank key packs the row index into 13 bits
static_assert(SEED_TILE == 64 && COL_TILE == 64, "sc2_second_order_kernel: 256 threads own 4 x 4 outputs each of a 64 x 64 tile");
static_assert(MAX_M == 8192, "rank and selection keys: 13 bits of row index");

struct Sc2Task {                   // mirrors roreg_sc2_task (include/roreg_hip.h)
    const double *keys0, *keys1;   // the two clouds' keypoints [*,3]
    const int64_t *matches;        // [M,2] interleaved (row in cloud 0, row in cloud 1)
    int32_t M, S;                  // correspondences, seeds = min(M, max_seeds)
    int64_t koff;                  // first row of this pair in the gathered P / Q and in deg
    int64_t boff;                  // first 64-bit word of this pair's bit rows
    int64_t hoff;                  // first row of this pair in Trans / seeds / consensus
    int64_t noff;                  // first element of this pair's N2 [S, M]
};

__device__ __forceinline__ int words_of(int M) { return (M + 63) >> 6; }

__global__ __launch_bounds__(256) void sc2_gather_kernel(const Sc2Task *__restrict__ tasks, double *__restrict__ P, double *__restrict__ Q) {
    const Sc2Task t = tasks[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.M) return;
    const int64_t r0 = t.matches[2 * i], r1 = t.matches[2 * i + 1];
    double *a = P + (t.koff + i) * 3, *b = Q + (t.koff + i) * 3;
    a[0] = t.keys0[3 * r0]; a[1] = t.keys0[3 * r0 + 1]; a[2] = t.keys0[3 * r0 + 2];
    b[0] = t.keys1[3 * r1]; b[1] = t.keys1[3 * r1 + 1]; b[2] = t.keys1[3 * r1 + 2];
}

__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

// One wave = one word column (64 columns j, one per lane, held in registers) x 64 rows i, whose points are broadcast one after the other: the
// ballot of the predicate IS word (i, j / 64).  Lanes at or beyond M and the diagonal vote 0, so the padding needs no later mask.
__global__ __launch_bounds__(256) void sc2_compat_kernel(const Sc2Task *__restrict__ tasks, const double *__restrict__ P, const double *__restrict__ Q,
                                                         double tau, unsigned long long *__restrict__ bits) {
    const Sc2Task t = tasks[blockIdx.z];
    const int W = words_of(t.M), lane = threadIdx.x & 63;
    const int jw = blockIdx.x * 4 + (threadIdx.x >> 6), i0 = blockIdx.y * 64;
    if (jw >= W || i0 >= t.M) return;                              // (wave-uniform)
    const double *p = P + t.koff * 3, *q = Q + t.koff * 3;
    const int j = jw * 64 + lane;
    const bool live = j < t.M;
    const int jr = live ? j : 0;
    const double pjx = p[3 * jr], pjy = p[3 * jr + 1], pjz = p[3 * jr + 2], qjx = q[3 * jr], qjy = q[3 * jr + 1], qjz = q[3 * jr + 2];
    unsigned long long mine = 0;
    const int rows = min(64, t.M - i0);
    for (int r = 0; r < rows; ++r) {
        const int i = i0 + r;
        const double a = dist3(p[3 * i], p[3 * i + 1], p[3 * i + 2], pjx, pjy, pjz);
        const double b = dist3(q[3 * i], q[3 * i + 1], q[3 * i + 2], qjx, qjy, qjz);
        const unsigned long long word = __ballot(live && i != j && fabs(__dsub_rn(a, b)) <= tau);
        if (lane == r) mine = word;
    }
    if (lane < rows) bits[t.boff + (int64_t)(i0 + lane) * W + jw] = mine;
}

// deg_i = popcount of row i: one wave per row
__global__ __launch_bounds__(256) void sc2_degree_kernel(const Sc2Task *__restrict__ tasks, const unsigned long long *__restrict__ bits,
                                                         int32_t *__restrict__ deg) {
    const Sc2Task t = tasks[blockIdx.y];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= t.M) return;
    const int W = words_of(t.M);
    const unsigned long long *row = bits + t.boff + (int64_t)i * W;
    int n = 0;
    for (int w = lane; w < W; w += 64) n += __popcll(row[w]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) deg[t.koff + i] = n;
}

// Seeds: the rows sorted by the key (M - deg) << 13 | i (distinct keys: a bitonic sort in LDS gives the one order), the first S of them.
__global__ __launch_bounds__(256) void sc2_rank_kernel(const Sc2Task *__restrict__ tasks, const int32_t *__restrict__ deg, int32_t *__restrict__ seeds) {
    __shared__ uint32_t key[MAX_M];
    const Sc2Task t = tasks[blockIdx.x];
    if (t.M <= 0) return;
    int n = 64;
    while (n < t.M) n <<= 1;                                       // <= MAX_M: the entry point refuses a larger M
    for (int i = threadIdx.x; i < n; i += 256) key[i] = i < t.M ? ((uint32_t)(t.M - deg[t.koff + i]) << 13) | (uint32_t)i : 0xffffffffu;
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < n; i += 256) {
                const int x = i ^ j;
                if (x > i) {
                    const uint32_t a = key[i], b = key[x];
                    if ((a > b) == ((i & k) == 0)) { key[i] = b; key[x] = a; }
                }
            }
            __syncthreads();
        }
    for (int h = threadIdx.x; h < t.S; h += 256) seeds[t.hoff + h] = (int32_t)(key[h] & (MAX_M - 1));
}

// N2 for a tile of SEED_TILE seeds x COL_TILE columns: both tiles' bit rows go through LDS WORD_CHUNK words at a time, each thread ANDs and
// counts 4 x 4 row pairs.  Row pitch WORD_CHUNK + 1 words: consecutive rows start two banks apart, so the 16 column rows and the 2 seed rows a
// 32-lane group reads in one ds_read_b64 fall on distinct banks (equal addresses broadcast).
__global__ __launch_bounds__(256) void sc2_second_order_kernel(const Sc2Task *__restrict__ tasks, const unsigned long long *__restrict__ bits,
                                                               const int32_t *__restrict__ seeds, uint16_t *__restrict__ N2) {
    __shared__ unsigned long long As[SEED_TILE][WORD_CHUNK + 1], Bs[COL_TILE][WORD_CHUNK + 1];
    const Sc2Task t = tasks[blockIdx.z];
    const int j0 = blockIdx.x * COL_TILE, s0 = blockIdx.y * SEED_TILE;
    if (j0 >= t.M || s0 >= t.S) return;                            // (block-uniform)
    const int W = words_of(t.M), tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const unsigned long long *base = bits + t.boff;
    // the rows this thread stages: tile row r = tid / WORD_CHUNK + ROWS_PER_PASS q, word tid % WORD_CHUNK of the chunk
    constexpr int ROWS_PER_PASS = 256 / WORD_CHUNK, PASSES = SEED_TILE / ROWS_PER_PASS;
    const int lw = tid % WORD_CHUNK, lr = tid / WORD_CHUNK;
    int64_t arow[PASSES], brow[PASSES];
#pragma unroll
    for (int q = 0; q < PASSES; ++q) {
        const int s = s0 + lr + ROWS_PER_PASS * q, j = j0 + lr + ROWS_PER_PASS * q;
        arow[q] = s < t.S ? (int64_t)seeds[t.hoff + s] * W : -1;
        brow[q] = j < t.M ? (int64_t)j * W : -1;
    }
    uint32_t acc[4][4] = {};
    for (int w0 = 0; w0 < W; w0 += WORD_CHUNK) {
        const int nw = min(WORD_CHUNK, W - w0);
#pragma unroll
        for (int q = 0; q < PASSES; ++q) {
            As[lr + ROWS_PER_PASS * q][lw] = (lw < nw && arow[q] >= 0) ? base[arow[q] + w0 + lw] : 0ull;
            Bs[lr + ROWS_PER_PASS * q][lw] = (lw < nw && brow[q] >= 0) ? base[brow[q] + w0 + lw] : 0ull;
        }
        __syncthreads();
        for (int w = 0; w < nw; ++w) {
            unsigned long long a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = As[ty + 16 * u][w]; b[u] = Bs[tx + 16 * u][w]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] += __popcll(a[u] & b[v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int s = s0 + ty + 16 * u;
        if (s >= t.S) continue;
        const unsigned long long *srow = base + (int64_t)seeds[t.hoff + s] * W;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int j = j0 + tx + 16 * v;
            if (j < t.M) N2[t.noff + (int64_t)s * t.M + j] = (srow[j >> 6] >> (j & 63) & 1ull) ? (uint16_t)acc[u][v] : (uint16_t)0;
        }
    }
}

// The selection's per-lane cache: the four greatest keys of the lane's stripe of columns (j = lane, lane + 64, ...) below a bound, sorted.
struct Top4 {
    uint32_t c0, c1, c2, c3;
    __device__ __forceinline__ void clear() { c0 = c1 = c2 = c3 = 0; }
    __device__ __forceinline__ void insert(uint32_t key) {
        if (key <= c3) return;
        c3 = key;
        if (c3 > c2) { const uint32_t x = c2; c2 = c3; c3 = x; }
        if (c2 > c1) { const uint32_t x = c1; c1 = c2; c2 = x; }
        if (c1 > c0) { const uint32_t x = c0; c0 = c1; c1 = x; }
    }
    __device__ __forceinline__ void pop() { c0 = c1; c1 = c2; c2 = c3; c3 = 0; }
};

// the keys of the lane's stripe below `bound` -> its four greatest; true if the cache came back full (there may be more below its last one)
__device__ __forceinline__ bool sc2_refill(Top4 &top, const unsigned long long *__restrict__ row, const uint16_t *__restrict__ n2, int M, int lane,
                                           uint32_t bound) {
    top.clear();
    for (int j = lane; j < M; j += 64)
        if (row[j >> 6] >> lane & 1ull) {                          // key = (N2 << 13 | 8191 - j) + 1 > 0 for a compatible column
            const uint32_t key = (((uint32_t)n2[j] << 13) | (uint32_t)(MAX_M - 1 - j)) + 1u;
            if (key < bound) top.insert(key);
        }
    return top.c3 != 0;
}

// One wave per seed.  Selection: the K - 1 greatest (N2, -j) among the seed's compatible columns.  Every lane caches the four greatest keys of
// its stripe in ONE pass over the row; a round takes the greatest head of the 64 caches (keys are distinct) and pops it; a lane whose cache
// runs empty while its stripe may hold more scans the stripe again below its last pick.  Member r is kept by lane r; then the centroids and
// the cross-covariance as butterfly sums over the lanes and the fit on lane 0.
__global__ __launch_bounds__(256) void sc2_fit_kernel(const Sc2Task *__restrict__ tasks, const double *__restrict__ P, const double *__restrict__ Q,
                                                      const unsigned long long *__restrict__ bits, const int32_t *__restrict__ seeds,
                                                      const uint16_t *__restrict__ N2, int K, double *__restrict__ Trans, int32_t *__restrict__ cons) {
    const Sc2Task t = tasks[blockIdx.y];
    const int h = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (h >= t.S) return;                                          // (wave-uniform)
    const int W = words_of(t.M), s = seeds[t.hoff + h];
    const unsigned long long *row = bits + t.boff + (int64_t)s * W;
    const uint16_t *n2 = N2 + t.noff + (int64_t)h * t.M;
    int mine = lane == 0 ? s : -1, cnt = 1;
    Top4 top;
    bool more = sc2_refill(top, row, n2, t.M, lane, 0xffffffffu);
    for (int r = 1; r < K; ++r) {
        uint32_t best = top.c0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const uint32_t other = __shfl_xor(best, o); best = other > best ? other : best; }
        if (best == 0) break;                                      // (wave-uniform) fewer than K - 1 compatible columns
        if (top.c0 == best) {                                      // the one lane that holds it
            top.pop();
            if (top.c0 == 0 && more) more = sc2_refill(top, row, n2, t.M, lane, best);
        }
        if (lane == r) mine = MAX_M - 1 - (int)((best - 1u) & (uint32_t)(MAX_M - 1));
        ++cnt;
    }
    if (cons && lane < K) cons[(t.hoff + h) * K + lane] = mine;
    const double *p = P + t.koff * 3, *q = Q + t.koff * 3;
    double *T = Trans + (t.hoff + h) * 12;
    if (cnt < 3) {                                                 // R = I, t = P_s - Q_s: finite and exact
        if (lane < 12) {
            const int r = lane >> 2, c = lane & 3;
            T[lane] = c == 3 ? __dsub_rn(p[3 * s + r], q[3 * s + r]) : (r == c ? 1.0 : 0.0);
        }
        return;
    }
    const bool in = mine >= 0;
    const int m = in ? mine : 0;
    const double n = (double)cnt;
    const double px = in ? p[3 * m] : 0.0, py = in ? p[3 * m + 1] : 0.0, pz = in ? p[3 * m + 2] : 0.0;
    const double qx = in ? q[3 * m] : 0.0, qy = in ? q[3 * m + 1] : 0.0, qz = in ? q[3 * m + 2] : 0.0;
    const double cp[3] = {wave_sum(px) / n, wave_sum(py) / n, wave_sum(pz) / n};
    const double cq[3] = {wave_sum(qx) / n, wave_sum(qy) / n, wave_sum(qz) / n};
    const double dp[3] = {in ? px - cp[0] : 0.0, in ? py - cp[1] : 0.0, in ? pz - cp[2] : 0.0};
    const double dq[3] = {in ? qx - cq[0] : 0.0, in ? qy - cq[1] : 0.0, in ? qz - cq[2] : 0.0};
    double Hm[9];                                                  // sum (p - cp)(q - cq)^T: its polar factor maps Q onto P
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Hm[r * 3 + c] = wave_sum(dp[r] * dq[c]);
    if (lane == 0) {
        double R[9];
        polar_proper(Hm, R);
        for (int r = 0; r < 3; ++r) {
            T[r * 4] = R[r * 3]; T[r * 4 + 1] = R[r * 3 + 1]; T[r * 4 + 2] = R[r * 3 + 2];
            T[r * 4 + 3] = cp[r] - (R[r * 3] * cq[0] + R[r * 3 + 1] * cq[1] + R[r * 3 + 2] * cq[2]);
        }
    }
}

// the workspace's regions, each followed by a guard of at least 64 bytes that no kernel writes
struct Sc2Layout { size_t P, Q, bits, deg, N2, total; };
Sc2Layout sc2_layout(long long total_M, long long total_words, long long total_SM) {
    Sc2Layout l;
    size_t at = 0;
    auto region = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes + 64, 256); return o; };
    l.P = region((size_t)total_M * 3 * sizeof(double));
    l.Q = region((size_t)total_M * 3 * sizeof(double));
    l.bits = region((size_t)total_words * sizeof(unsigned long long));
    l.deg = region((size_t)total_M * sizeof(int32_t));
    l.N2 = region((size_t)total_SM * sizeof(uint16_t));
    l.total = at;
    return l;
}

}  // namespace

extern "C" size_t roreg_sc2_workspace(long long total_M, long long total_words, long long total_SM, size_t *offsets) {
    if (total_M < 0 || total_words < 0 || total_SM < 0) return 0;
    const Sc2Layout l = sc2_layout(total_M, total_words, total_SM);
    if (offsets) { offsets[0] = l.P; offsets[1] = l.Q; offsets[2] = l.bits; offsets[3] = l.deg; offsets[4] = l.N2; }
    return l.total;
}

extern "C" int roreg_sc2_hypotheses_batch(const roreg_sc2_task *tasks_dev, int n_tasks, long long total_M, long long total_words, long long total_SM,
                                          int max_M, int max_S, double tau, int K, double *Trans_out, int32_t *seeds_out, int32_t *cons_out,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    static_assert(sizeof(roreg_sc2_task) == sizeof(Sc2Task), "roreg_sc2_task layout");
    ROREG_REQUIRE(n_tasks >= 0 && n_tasks <= 65535, "roreg_sc2_hypotheses_batch: 0..65535 tasks per call, got %d", n_tasks);
    ROREG_REQUIRE(K >= 3 && K <= 64, "roreg_sc2_hypotheses_batch: K must lie in 3..64, got %d", K);
    ROREG_REQUIRE(max_M >= 0 && max_M <= ROREG_SC2_MAX_M, "roreg_sc2_hypotheses_batch: at most %d correspondences per pair, got %d", ROREG_SC2_MAX_M, max_M);
    ROREG_REQUIRE(tau >= 0.0 && max_S >= 0 && max_S <= max_M && total_M >= 0 && total_words >= 0 && total_SM >= 0, "roreg_sc2_hypotheses_batch: bad arguments");
    if (n_tasks == 0 || max_M == 0) return 0;
    ROREG_REQUIRE(tasks_dev && workspace && (max_S == 0 || (Trans_out && seeds_out)), "roreg_sc2_hypotheses_batch: null argument");
    const Sc2Layout l = sc2_layout(total_M, total_words, total_SM);
    ROREG_REQUIRE(workspace_bytes >= l.total, "roreg_sc2_hypotheses_batch: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    const Sc2Task *tasks = reinterpret_cast<const Sc2Task *>(tasks_dev);
    char *ws = reinterpret_cast<char *>(workspace);
    double *P = reinterpret_cast<double *>(ws + l.P), *Q = reinterpret_cast<double *>(ws + l.Q);
    unsigned long long *bits = reinterpret_cast<unsigned long long *>(ws + l.bits);
    int32_t *deg = reinterpret_cast<int32_t *>(ws + l.deg);
    uint16_t *N2 = reinterpret_cast<uint16_t *>(ws + l.N2);
    const int max_W = (max_M + 63) / 64;
    hipLaunchKernelGGL(sc2_gather_kernel, dim3((max_M + 255) / 256, n_tasks), dim3(256), 0, s, tasks, P, Q);
    hipLaunchKernelGGL(sc2_compat_kernel, dim3((max_W + 3) / 4, (max_M + 63) / 64, n_tasks), dim3(256), 0, s, tasks, P, Q, tau, bits);
    hipLaunchKernelGGL(sc2_degree_kernel, dim3((max_M + 3) / 4, n_tasks), dim3(256), 0, s, tasks, bits, deg);
    hipLaunchKernelGGL(sc2_rank_kernel, dim3(n_tasks), dim3(256), 0, s, tasks, deg, seeds_out);
    if (max_S > 0) {
        hipLaunchKernelGGL(sc2_second_order_kernel, dim3((max_M + COL_TILE - 1) / COL_TILE, (max_S + SEED_TILE - 1) / SEED_TILE, n_tasks), dim3(256), 0, s,
                           tasks, bits, seeds_out, N2);
        hipLaunchKernelGGL(sc2_fit_kernel, dim3((max_S + 3) / 4, n_tasks), dim3(256), 0, s, tasks, P, Q, bits, seeds_out, N2, K, Trans_out, cons_out);
    }
    ROREG_CHECK_LAUNCH("roreg_sc2_hypotheses_batch");
    return 0;
}
