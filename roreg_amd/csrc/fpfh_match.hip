// Mutual nearest-neighbour matching of FPFH descriptors (33 channels) on the matrix cores, with bit-exact results.
//
// Definition: per task, with S = desc0[rows0] (m0 rows) and T = desc1[rows1] (m1 rows), nn01 / dist01 / nn10 are what roreg_nn_search_ex(.., F = 33,
// squared = 0) answers for the two directions -- d = sqrtf((sum over ascending f of (s_f - t_f)^2, separate multiply and add) + 1e-7f), the first
// index among equal d -- and the mutual pairs are roreg_mutual_matches' (increasing i, mapped through the row lists).
// PRECONDITION: every selected row is finite and its squared norm is 0 or lies in [2^-60, 2^100] (roreg_fpfh_features writes values in [0, 200];
// fpfh.match selects valid rows only).  Rows the lists do not select are never read.
//
// Method (match_tile.h holds what this matcher shares with mfma_match.hip -- the tile product, the two passes' epilogues, the literal distance, the
// ordered compaction; the workspace, the prepare kernel, a(i,j), the margin and the debug hooks are this file's own):
//   prepare: rows gathered at a pitch of 36 floats (channels 0..32, three zeros), n = the squared norm over channels 0..31 (summed in float64, rounded
//            once), each side's greatest 33-channel squared norm; minima and packed keys initialised.  Each side of each task is padded to its own
//            multiple of the tile edge (pad rows: zeros with n = 1e30, never a minimum, never a candidate).
//   pass A:  a(i,j) = ((n_i + n_j) - 2 s.t|32) + (s_32 - t_32)^2 per 128 x 128 tile: s.t|32 = the dot product over channels 0..31 as fp16 x 2 split
//            MFMAs (primitives.h split2 / split_mma, per-row power-of-two scale), channel 32 on the vector pipe.  Row minima amin0[i] and column
//            minima amin1[j] from the same tile (the literal formula is bitwise symmetric in (s, t)), merged by 32-bit atomicMin on ordered keys.
//   pass B:  the tile again; every entry with a <= amin0[i] + margin0[i] (a CANDIDATE of row i) or a <= amin1[j] + margin1[j] (of column j) is
//            evaluated with the literal 33-channel formula from the staged rows and merged by 64-bit atomicMin on (float_bits(d) << 32 | index):
//            the least d, and among equal d (equal roots of different radicands included) the least index.
//   finish:  nn01 / dist01 / nn10 unpacked, the mutual check and the ordered compaction (one workgroup per task).
//
// The margin (u = 2^-24; N = squared norm over all 33 channels; x = the real number sum_f (s_f - t_f)^2 of the float32 inputs):
//  (1) |a - x| <= delta(i,j) = C_DELTA (N_i + N_j), C_DELTA = 8 u + (96 * 2^-23 + 3.01 * 2^-22 + 2^-34):
//      - operands: with 2^e |s|_32 in [2^13, 2^14) (norm_exp), hi = fp16(2^e s_f), lo = fp16(2^e s_f - hi): |2^e s_f - hi - lo| <= 2^-22 |2^e s_f| + 2^-25
//        (the second term where lo is subnormal in fp16; the MFMA takes subnormal operands as they are).  The product keeps lo.hi, hi.lo, hi.hi and
//        drops lo.lo (<= 2^-22 (1 + 2^-10) |s_f t_f|): in real units the dot product's truncation error is <= 3.01 * 2^-22 sum_f |s_f t_f| plus
//        2^-25 (|s|_1 2^-e_t + |t|_1 2^-e_s) <= 2 sqrt(32) 2^-38 |s||t| < 2^-34 |s||t|;
//      - accumulation: the 96 products are exact in float32; their float32 accumulation inside and across the six MFMAs, whatever its order and
//        even if every addition truncates (relative error 2^-23), is within 96 * 2^-23 sum |products| <= 96 * 2^-23 (1 + 2^-9) sum_f |s_f t_f|;
//      - the dot product enters a twice (- 2 s.t) and sum_f |s_f t_f| <= |s||t| <= (N_i + N_j) / 2: together (96 * 2^-23 + 3.01 * 2^-22 + 2^-34)(N_i + N_j);
//      - the epilogue: the norms are rounded once (u each), n_i + n_j (u), the subtraction (u |result| <= 2 u (n_i + n_j)), w = s_32 - t_32 and
//        w w (3 u w^2 <= 6 u (s_32^2 + t_32^2)), the last addition (u |a| <= 2 u (N_i + N_j)): <= 8 u (N_i + N_j).  The scalings by 2^-e are exact.
//  (2) literal formula: its float32 radicand is x (1 + theta), |theta| <= 36 u (33 terms of 3 roundings each, 32 additions of non-negative terms).
//      If target j* gives a root not greater than target j's, then fl(x32* + 1e-7) <= fl(x32 + 1e-7)(1 + 4.01 u) (two correctly rounded roots), hence
//      x(j*) <= x(j) + C_COLLAPSE (x(j) + 1e-7), C_COLLAPSE = 80 u >= (2 * 36 + 6.1 + slack) u: the "sqrt-collapse" term, relative to the distance itself.
//  (3) let j* be the exact winner of row i and j^ the minimiser of a(i, .) found in pass A (amin0[i] = a(i,j^); pass A's row minima come from the
//      transposed product, whose values also satisfy (1)).  With Delta_i = C_DELTA (N_i + max_j N_j) >= delta(i, .):
//        a(i,j*) <= x(j*) + Delta_i <= x(j^) + C_COLLAPSE (x(j^) + 1e-7) + Delta_i <= amin0[i] + 2 Delta_i + C_COLLAPSE (amin0[i] + Delta_i + 1e-7).
//      margin0[i] = MARGIN_MULT (2 Delta_i + C_COLLAPSE (max(amin0[i], 0) + Delta_i + 1e-7)) with MARGIN_MULT = 2: the factor covers the float32
//      evaluation of the margin itself and leaves room for an accumulation that is worse than (1) assumes.  So j* is a candidate of row i, every
//      candidate is evaluated literally, and the packed minimum returns j*.  Columns alike.  roreg_amd/_hip_fpfh.py restates C_DELTA, C_COLLAPSE and
//      the margin (fpfh_match_delta / fpfh_match_margin); tests/test_hip_fpfh_match.py checks (1) entry by entry against float64.
#include "common.h"
#include "match_tile.h"

#pragma clang fp contract(off)

namespace {

using namespace match_tile;

struct FmTask {                    // mirrors roreg_fpfh_match_task (include/roreg_hip.h)
    const float *desc0, *desc1;
    const int64_t *rows0, *rows1;
    int32_t m0, m1;
    int64_t r0, r1;                // first padded row of side 0 / side 1 in the workspace
    int64_t o0, o1, om;            // first element of this task in nn01 / dist01, in nn10, first row in matches
};
struct FmDebug {                   // mirrors roreg_fpfh_match_debug
    float *a, *amin0, *amin1;
    int32_t *cnt0, *cnt1;
};

constexpr int F = ROREG_FPFH_MATCH_WIDTH, FM = 32;               // channels; channels on the matrix cores
constexpr int MAX_ROWS = ROREG_FPFH_MATCH_MAX_ROWS, DEBUG_MAX = ROREG_FPFH_MATCH_DEBUG_MAX;
constexpr float PAD_NORM = 1e30f;
constexpr float C_DELTA = 8.f * 5.9604645e-8f + (96.f * 1.1920929e-7f + 3.01f * 2.3841858e-7f + 5.8207661e-11f);
constexpr float C_COLLAPSE = 80.f * 5.9604645e-8f;
constexpr float MARGIN_MULT = 2.f;
static_assert(F == 33 && ROREG_FPFH_MATCH_TILE == TILE, "fm_tile_kernel: match_tile.h's 128 x 128 tile; channel 32 rides the vector pipe");
// LP = 36 (the row pitch in floats, in LDS and in the workspace): a wave's b128 fragment reads touch rows r, r + 1, .. of one 16-lane group at word
// offsets 36 r mod 64 = 4 (9 r mod 16), sixteen different 4-bank groups for each of the hardware's lane groups
// {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}: conflict-free.

struct Layout { size_t G, N, AM, PK, MX, total; };
__host__ inline Layout fm_layout(long long total_rows, int n_tasks) {
    Layout l;
    size_t at = 0;
    auto region = [&](size_t bytes) { const size_t o = at; at = align_up(at + bytes + 64, 256); return o; };
    l.G = region((size_t)total_rows * LP * 4);
    l.N = region((size_t)total_rows * 4);
    l.AM = region((size_t)total_rows * 4);
    l.PK = region((size_t)total_rows * 8);
    l.MX = region((size_t)n_tasks * 2 * 4);
    l.total = at;
    return l;
}
struct WS { float *G, *N; unsigned *AM; unsigned long long *PK; unsigned *MX; };

__device__ __forceinline__ float margin_of(float amin, float n33, float mx_other) {
    const float delta = C_DELTA * (n33 + mx_other);
    return MARGIN_MULT * (2.f * delta + C_COLLAPSE * (fmaxf(amin, 0.f) + delta + 1e-7f));
}

// one wave per padded row
__global__ __launch_bounds__(256) void fm_prepare_kernel(const FmTask *__restrict__ tasks, WS w) {
    const int task = blockIdx.z >> 1, side = blockIdx.z & 1;
    const FmTask t = tasks[task];
    const float *desc = side ? t.desc1 : t.desc0;
    const int64_t *rows = side ? t.rows1 : t.rows0;
    const int m = side ? t.m1 : t.m0;
    const int64_t base = side ? t.r1 : t.r0;
    const int P = round_up(m, TILE);
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), f = threadIdx.x & 63;
    if (j >= P) return;                                             // (wave-uniform)
    float v = 0.f;
    if (j < m && f < F) v = desc[(size_t)(rows ? rows[j] : (int64_t)j) * F + f];
    if (f < LP) w.G[(size_t)(base + j) * LP + f] = v;
    const double sq = (double)v * (double)v;
    const double n32 = wave_sum(f < FM ? sq : 0.0), n33 = wave_sum(sq);
    if (f == 0) {
        w.N[base + j] = j < m ? (float)n32 : PAD_NORM;
        w.AM[base + j] = 0xffffffffu;
        w.PK[base + j] = ~0ull;
        if (j < m) {
            float up = (float)n33;
            if ((double)up < n33) up = __uint_as_float(__float_as_uint(up) + 1u);      // rounded up: the margin takes it as a bound
            atomicMax(&w.MX[2 * task + side], __float_as_uint(up));
        }
    }
}

// pass B's debug hooks (tasks of at most DEBUG_MAX rows a side): every real entry a(i,j), and how many literal evaluations each row and column received
struct FmSink {
    bool on;
    FmDebug D;
    int i0, j0, m0, m1;
    __device__ void entry(int i, int j, float av) const {
        if (on && D.a && j0 + j < m1 && i0 + i < m0) D.a[(size_t)(i0 + i) * m1 + j0 + j] = av;
    }
    __device__ void candidate(int i, int j, bool k0, bool k1) const {
        if (on) {
            if (k0 && D.cnt0) atomicAdd(&D.cnt0[i0 + i], 1);
            if (k1 && D.cnt1) atomicAdd(&D.cnt1[j0 + j], 1);
        }
    }
};

// One 128 x 128 tile of one task's distance matrix.  VERIFY = false: approximate row / column minima.  VERIFY = true: candidates -> literal
// distances -> packed keys.
template <bool VERIFY>
__global__ __launch_bounds__(256, 2) void fm_tile_kernel(const FmTask *__restrict__ tasks, WS w, const FmDebug *__restrict__ debug) {
    __shared__ __attribute__((aligned(16))) float S[TILE * LP], T[TILE * LP];
    __shared__ float n0s[TILE], n1s[TILE], v0s[TILE], v1s[TILE], thr0[TILE], thr1[TILE];
    __shared__ float xs0[TILE], xs1[TILE], is0[TILE], is1[TILE];        // the rows' scales 2^e and 2^-e
    const int task = blockIdx.z;
    const FmTask t = tasks[task];
    const int i0 = blockIdx.y * TILE, j0 = blockIdx.x * TILE;
    if (i0 >= t.m0 || j0 >= t.m1) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv & 1, wn = wv >> 1, jl = lane & 31, h = lane >> 5;
    const size_t g0 = (size_t)t.r0 + i0, g1 = (size_t)t.r1 + j0;      // the tiles' first workspace rows (both whole tiles: the sides are padded)

    {
        const float4 *p0 = reinterpret_cast<const float4 *>(w.G + g0 * LP);
        const float4 *p1 = reinterpret_cast<const float4 *>(w.G + g1 * LP);
        for (int q = tid; q < TILE * LP / 4; q += 256) {
            reinterpret_cast<float4 *>(S)[q] = p0[q];
            reinterpret_cast<float4 *>(T)[q] = p1[q];
        }
        if (tid < TILE) {
            const float a = w.N[g0 + tid], b = w.N[g1 + tid];
            const float va = w.G[(g0 + tid) * LP + FM], vb = w.G[(g1 + tid) * LP + FM];
            n0s[tid] = a; n1s[tid] = b; v0s[tid] = va; v1s[tid] = vb;
            const int ea = norm_exp(a), eb = norm_exp(b);
            xs0[tid] = ldexpf(1.f, ea); is0[tid] = ldexpf(1.f, -ea); xs1[tid] = ldexpf(1.f, eb); is1[tid] = ldexpf(1.f, -eb);
            if (VERIFY) {
                const float mx0 = __uint_as_float(w.MX[2 * task]), mx1 = __uint_as_float(w.MX[2 * task + 1]);
                const float am0 = o2f(w.AM[g0 + tid]), am1 = o2f(w.AM[g1 + tid]);
                // a pad row has no minimum: nothing is its candidate
                thr0[tid] = i0 + tid < t.m0 ? am0 + margin_of(am0, a + va * va, mx1) : -__builtin_inff();
                thr1[tid] = j0 + tid < t.m1 ? am1 + margin_of(am1, b + vb * vb, mx0) : -__builtin_inff();
            }
        }
    }
    __syncthreads();

    const Tile tl = {S, T, xs0, xs1, is0, is1, i0, j0, t.m0, t.m1, wm, wn, jl, h};
    f32x16 c[2][2], ct[2][2];
    tile_product<2, !VERIFY>(tl, c, ct);
    // a(i,j): channel 32 added on the vector pipe
    const auto a = [&](int i, int j, float dot) { return ((n0s[i] + n1s[j]) - 2.f * dot) + (v0s[i] - v1s[j]) * (v0s[i] - v1s[j]); };
    if constexpr (!VERIFY) tile_minima<2>(tl, c, ct, a, w.AM + g0, w.AM + g1);
    else {
        FmSink sink = {debug != nullptr && t.m0 <= DEBUG_MAX && t.m1 <= DEBUG_MAX, {}, i0, j0, t.m0, t.m1};
        if (sink.on) sink.D = debug[task];
        tile_verify<2, F>(tl, c, a, thr0, thr1, w.PK + g0, w.PK + g1, sink);
    }
}

// nn01 / dist01 / nn10 from the packed keys, then the mutual check and the ordered compaction: one workgroup per task
__global__ __launch_bounds__(1024) void fm_finish_kernel(const FmTask *__restrict__ tasks, WS w, int64_t *__restrict__ nn01_all, float *__restrict__ dist01_all,
                                                         int64_t *__restrict__ nn10_all, int64_t *__restrict__ match_all, int32_t *__restrict__ counts,
                                                         const FmDebug *__restrict__ debug) {
    const int task = blockIdx.x;
    const FmTask t = tasks[task];
    const unsigned long long *p01 = w.PK + t.r0, *p10 = w.PK + t.r1;
    const int tid = threadIdx.x;
    const bool live = t.m0 > 0 && t.m1 > 0;
    if (live) {
        // a key that no candidate ever updated (the precondition broken: every comparison with NaN is false) keeps index bits outside [0, m): the
        // row is unmatched, as roreg_mutual_matches treats an index outside the other side
        for (int j = tid; j < t.m1; j += 1024) nn10_all[t.o1 + j] = (int64_t)(p10[j] & 0xffffffffu);
        if (debug && t.m0 <= DEBUG_MAX && t.m1 <= DEBUG_MAX) {
            const FmDebug D = debug[task];
            if (D.amin0) for (int i = tid; i < t.m0; i += 1024) D.amin0[i] = o2f(w.AM[t.r0 + i]);
            if (D.amin1) for (int j = tid; j < t.m1; j += 1024) D.amin1[j] = o2f(w.AM[t.r1 + j]);
        }
    }
    const auto nn01 = [&](int i) {                 // (reading row i's key is also where its outputs are written)
        const unsigned long long k = p01[i];
        const int64_t j = (int64_t)(k & 0xffffffffu);
        nn01_all[t.o0 + i] = j;
        dist01_all[t.o0 + i] = __uint_as_float((unsigned)(k >> 32));
        return j;
    };
    compact_mutual(live ? t.m0 : 0, t.m1, nn01, [&](int64_t j) { return (int64_t)(p10[j] & 0xffffffffu); }, t.rows0, t.rows1, match_all + t.om * 2,
                   counts + task);
}

}  // namespace

extern "C" size_t roreg_fpfh_match_workspace(long long total_rows, int n_tasks, size_t *offsets) {
    if (total_rows < 0 || n_tasks < 0) return 0;
    const Layout l = fm_layout(total_rows, n_tasks);
    if (offsets) { offsets[0] = l.G; offsets[1] = l.N; offsets[2] = l.AM; offsets[3] = l.PK; offsets[4] = l.MX; }
    return l.total;
}

extern "C" int roreg_fpfh_match_batch(const roreg_fpfh_match_task *tasks_dev, int n_tasks, int max_m0, int max_m1, long long total_rows,
                                      int64_t *nn01_out, float *dist01_out, int64_t *nn10_out, int64_t *match_out, int32_t *counts_out,
                                      const roreg_fpfh_match_debug *debug_dev, void *workspace, size_t workspace_bytes, void *stream) {
    static_assert(sizeof(roreg_fpfh_match_task) == sizeof(FmTask) && sizeof(FmTask) == 80, "roreg_fpfh_match_task layout");
    static_assert(sizeof(roreg_fpfh_match_debug) == sizeof(FmDebug) && sizeof(FmDebug) == 40, "roreg_fpfh_match_debug layout");
    ROREG_REQUIRE(n_tasks >= 0 && n_tasks <= 32767, "roreg_fpfh_match_batch: 0..32767 tasks per call, got %d", n_tasks);
    ROREG_REQUIRE(max_m0 >= 0 && max_m1 >= 0 && max_m0 <= MAX_ROWS && max_m1 <= MAX_ROWS,
                  "roreg_fpfh_match_batch: at most %d rows per side, got %d and %d", MAX_ROWS, max_m0, max_m1);
    ROREG_REQUIRE(total_rows >= 0, "roreg_fpfh_match_batch: bad arguments");
    if (n_tasks == 0) return 0;
    ROREG_REQUIRE(tasks_dev && counts_out && workspace, "roreg_fpfh_match_batch: null argument");
    const Layout l = fm_layout(total_rows, n_tasks);
    ROREG_REQUIRE(workspace_bytes >= l.total, "roreg_fpfh_match_batch: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    const FmTask *tasks = reinterpret_cast<const FmTask *>(tasks_dev);
    const FmDebug *debug = reinterpret_cast<const FmDebug *>(debug_dev);
    char *ws = reinterpret_cast<char *>(workspace);
    WS w;
    w.G = reinterpret_cast<float *>(ws + l.G); w.N = reinterpret_cast<float *>(ws + l.N); w.AM = reinterpret_cast<unsigned *>(ws + l.AM);
    w.PK = reinterpret_cast<unsigned long long *>(ws + l.PK); w.MX = reinterpret_cast<unsigned *>(ws + l.MX);
    const int max_m = max_m0 > max_m1 ? max_m0 : max_m1;
    if (max_m0 > 0 && max_m1 > 0) {
        ROREG_REQUIRE(nn01_out && dist01_out && nn10_out && match_out, "roreg_fpfh_match_batch: null output");
        if (hipMemsetAsync(w.MX, 0, (size_t)n_tasks * 2 * 4, s) != hipSuccess) { roreg::set_error("roreg_fpfh_match_batch: hipMemsetAsync failed"); return 1; }
        hipLaunchKernelGGL(fm_prepare_kernel, dim3(round_up(max_m, TILE) / 4, 1, 2 * n_tasks), dim3(256), 0, s, tasks, w);
        const dim3 grid((max_m1 + TILE - 1) / TILE, (max_m0 + TILE - 1) / TILE, n_tasks);
        {
            roreg::ProfScope prof(roreg::PROF_FM_PASS_A, s);
            hipLaunchKernelGGL(fm_tile_kernel<false>, grid, dim3(256), 0, s, tasks, w, debug);
        }
        {
            roreg::ProfScope prof(roreg::PROF_FM_PASS_B, s);
            hipLaunchKernelGGL(fm_tile_kernel<true>, grid, dim3(256), 0, s, tasks, w, debug);
        }
    }
    hipLaunchKernelGGL(fm_finish_kernel, dim3(n_tasks), dim3(1024), 0, s, tasks, w, nn01_out, dist01_out, nn10_out, match_out, counts_out, debug);
    ROREG_CHECK_LAUNCH("roreg_fpfh_match_batch");
    return 0;
}
