// Mutual nearest-neighbour matching of FPFH descriptors (33 channels) on the matrix cores, with bit-exact results.
//
// Definition: per task, with S = desc0[rows0] (m0 rows) and T = desc1[rows1] (m1 rows), nn01 / dist01 / nn10 are what roreg_nn_search_ex(.., F = 33,
// squared = 0) answers for the two directions -- d = sqrtf((sum over ascending f of (s_f - t_f)^2, separate multiply and add) + 1e-7f), the first
// index among equal d -- and the mutual pairs are roreg_mutual_matches' (increasing i, mapped through the row lists).
// PRECONDITION: every selected row is finite and its squared norm is 0 or lies in [2^-60, 2^100] (roreg_fpfh_features writes values in [0, 200];
// fpfh.match selects valid rows only).  Rows the lists do not select are never read.
//
// Method (the shape of mfma_match.hip; that kernel's F = 32 and common pitch are hard-wired, this one stands beside it):
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
#include "primitives.h"

#pragma clang fp contract(off)

namespace {

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
constexpr int TILE = ROREG_FPFH_MATCH_TILE, LP = 36;             // tile edge; row pitch in floats, in LDS and in the workspace
constexpr int MAX_ROWS = ROREG_FPFH_MATCH_MAX_ROWS, DEBUG_MAX = ROREG_FPFH_MATCH_DEBUG_MAX;
constexpr float PAD_NORM = 1e30f;
constexpr float C_DELTA = 8.f * 5.9604645e-8f + (96.f * 1.1920929e-7f + 3.01f * 2.3841858e-7f + 5.8207661e-11f);
constexpr float C_COLLAPSE = 80.f * 5.9604645e-8f;
constexpr float MARGIN_MULT = 2.f;
static_assert(F == 33 && TILE == 128, "fm_tile_kernel: 4 waves own 64 x 64 blocks of a 128 x 128 tile; channel 32 rides the vector pipe");
// LP = 36: a wave's b128 fragment reads touch rows r, r + 1, .. of one 16-lane group at word offsets 36 r mod 64 = 4 (9 r mod 16), sixteen different
// 4-bank groups for each of the hardware's lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}: conflict-free.

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

// float -> unsigned with the same total order (a can be slightly negative)
__device__ __forceinline__ unsigned f2o(float x) { const unsigned b = __float_as_uint(x); return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float o2f(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

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

// Block scale of a row: 2^e |x|_32 in [2^13, 2^14) (mfma_match.hip's rule, from the squared norm)
__device__ __forceinline__ int norm_exp(float n2) {
    if (!(n2 > 0.f) || !(n2 < __builtin_inff())) return 0;
    int ex;
    (void)frexpf(n2, &ex);
    return 14 - ((ex + 1) >> 1);
}
// the literal distance (knn_generic_kernel's arithmetic at F = 33)
__device__ __forceinline__ float exact_dist(const float *__restrict__ s, const float *__restrict__ t) {
    float acc = 0.f;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const float d = __fsub_rn(s[f], t[f]);
        acc = __fadd_rn(acc, __fmul_rn(d, d));
    }
    return sqrtf(__fadd_rn(acc, 1e-7f));
}

// One 128 x 128 tile of one task's distance matrix.  VERIFY = false: approximate row / column minima.  VERIFY = true: candidates -> literal
// distances -> packed keys.  4 waves as a 2 x 2 grid of 64 x 64 blocks (2 x 2 MFMA tiles each).
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

    // C = S.T^T over channels 0..31 (lanes own columns j), and for the row minima also C' = T.S^T (lanes own columns i)
    f32x16 c[2][2], ct[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { c[a][b][r] = 0.f; ct[a][b][r] = 0.f; }
#pragma unroll
    for (int st = 0; st < FM / 16; ++st) {
        f16x8 sf[2][2], tf[2][2];                   // fragments of the wave's two 32-row groups of S (rows wm*64..) and T (rows wn*64..)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float x8[8];
            const int rs = wm * 64 + g * 32 + jl, rt = wn * 64 + g * 32 + jl;
            const float4 *ps = reinterpret_cast<const float4 *>(S + rs * LP + st * 16 + h * 8);
            const float4 u0 = ps[0], u1 = ps[1];
            x8[0] = u0.x; x8[1] = u0.y; x8[2] = u0.z; x8[3] = u0.w; x8[4] = u1.x; x8[5] = u1.y; x8[6] = u1.z; x8[7] = u1.w;
            split2(x8, xs0[rs], sf[g][0], sf[g][1]);
            const float4 *pt = reinterpret_cast<const float4 *>(T + rt * LP + st * 16 + h * 8);
            const float4 v0 = pt[0], v1 = pt[1];
            x8[0] = v0.x; x8[1] = v0.y; x8[2] = v0.z; x8[3] = v0.w; x8[4] = v1.x; x8[5] = v1.y; x8[6] = v1.z; x8[7] = v1.w;
            split2(x8, xs1[rt], tf[g][0], tf[g][1]);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                c[a][b] = split_mma<2>(sf[a], tf[b], c[a][b]);                  // rows i = wm*64 + a*32 + .., column j = wn*64 + b*32 + jl
                if (!VERIFY) ct[a][b] = split_mma<2>(tf[a], sf[b], ct[a][b]);   // rows j = wn*64 + a*32 + .., column i = wm*64 + b*32 + jl
            }
    }
    // a(i,j): the accumulator rescaled by the exact 2^-e_i 2^-e_j, channel 32 added on the vector pipe
#define A_C(a, b, r, ir, nj, isj, vj) ((((n0s[ir] + (nj)) - 2.f * ((c[a][b][r] * is0[ir]) * (isj)))) + (v0s[ir] - (vj)) * (v0s[ir] - (vj)))
#define A_CT(a, b, r, jr, ni, isi, vi) ((((ni) + n1s[jr]) - 2.f * ((ct[a][b][r] * is1[jr]) * (isi))) + ((vi) - v1s[jr]) * ((vi) - v1s[jr]))

    if (!VERIFY) {
        // column minima of C: over the wave's 64 rows i, for column j -> amin1[j]
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int jc = wn * 64 + b * 32 + jl;
            const float nj = n1s[jc], isj = is1[jc], vj = v1s[jc];
            float mn = __builtin_inff();
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ir = cd_row32(r, h, wm * 64 + a * 32);
                    mn = fminf(mn, A_C(a, b, r, ir, nj, isj, vj));
                }
            mn = fminf(mn, __shfl_xor(mn, 32));
            if (h == 0 && j0 + jc < t.m1) atomicMin(&w.AM[g1 + jc], f2o(mn));
        }
        // column minima of C': over the wave's 64 rows j, for column i -> amin0[i]
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int ic = wm * 64 + b * 32 + jl;
            const float ni = n0s[ic], isi = is0[ic], vi = v0s[ic];
            float mn = __builtin_inff();
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int jr = cd_row32(r, h, wn * 64 + a * 32);
                    mn = fminf(mn, A_CT(a, b, r, jr, ni, isi, vi));
                }
            mn = fminf(mn, __shfl_xor(mn, 32));
            if (h == 0 && i0 + ic < t.m0) atomicMin(&w.AM[g0 + ic], f2o(mn));
        }
    } else {
        const bool dbg = debug != nullptr && t.m0 <= DEBUG_MAX && t.m1 <= DEBUG_MAX;
        FmDebug D = {};
        if (dbg) D = debug[task];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int jc = wn * 64 + b * 32 + jl;
            const float nj = n1s[jc], isj = is1[jc], vj = v1s[jc], tj = thr1[jc];
            const bool jin = j0 + jc < t.m1;
            // candidate masks first (bit a*16 + r), the exact evaluations afterwards in ONE loop body (mfma_match.hip's strip kernel: 64 inlined
            // copies of the literal distance are 100 KB of code and spill)
            unsigned k0m = 0u, k1m = 0u;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ir = cd_row32(r, h, wm * 64 + a * 32);
                    const float av = A_C(a, b, r, ir, nj, isj, vj);
                    k0m |= (av <= thr0[ir] ? 1u : 0u) << (a * 16 + r);             // candidate of row i
                    k1m |= (av <= tj ? 1u : 0u) << (a * 16 + r);                   // candidate of column j
                    if (dbg && D.a && jin && i0 + ir < t.m0) D.a[(size_t)(i0 + ir) * t.m1 + j0 + jc] = av;
                }
            if (!jin) k0m = 0u;                     // a pad column is nobody's candidate (its a is 1e30: not within any margin; said again here)
            unsigned m = k0m | k1m;
            while (m) {
                const int q = __ffs(m) - 1;
                m &= m - 1;
                const int ir = cd_row32(q & 15, h, wm * 64 + (q >> 4) * 32);
                const bool iin = i0 + ir < t.m0;
                const bool k0 = (k0m >> q) & 1u, k1 = ((k1m >> q) & 1u) && iin;
                if (!(k0 || k1)) continue;
                const float d = exact_dist(S + ir * LP, T + jc * LP);
                const unsigned long long db = (unsigned long long)__float_as_uint(d) << 32;
                // (keys only fall: one that is not below a plain load of the slot, however stale, cannot change it -- near-duplicate rows send
                //  most of their candidates to the same few slots)
                const unsigned long long key0 = db | (unsigned)(j0 + jc), key1 = db | (unsigned)(i0 + ir);
                if (k0 && key0 < w.PK[g0 + ir]) atomicMin(&w.PK[g0 + ir], key0);
                if (k1 && key1 < w.PK[g1 + jc]) atomicMin(&w.PK[g1 + jc], key1);
                if (dbg) {
                    if (k0 && D.cnt0) atomicAdd(&D.cnt0[i0 + ir], 1);
                    if (k1 && D.cnt1) atomicAdd(&D.cnt1[j0 + jc], 1);
                }
            }
        }
    }
#undef A_C
#undef A_CT
}

// nn01 / dist01 / nn10 from the packed keys, then the mutual check and the ordered compaction: one workgroup per task
__global__ __launch_bounds__(1024) void fm_finish_kernel(const FmTask *__restrict__ tasks, WS w, int64_t *__restrict__ nn01_all, float *__restrict__ dist01_all,
                                                         int64_t *__restrict__ nn10_all, int64_t *__restrict__ match_all, int32_t *__restrict__ counts,
                                                         const FmDebug *__restrict__ debug) {
    __shared__ int wave_cnt[16];
    __shared__ int base;
    const int task = blockIdx.x;
    const FmTask t = tasks[task];
    const unsigned long long *p01 = w.PK + t.r0, *p10 = w.PK + t.r1;
    int64_t *match_out = match_all + t.om * 2;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool live = t.m0 > 0 && t.m1 > 0;
    if (tid == 0) base = 0;
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
    __syncthreads();
    const int m = live ? t.m0 : 0;
    for (int start = 0; start < m; start += 1024) {
        const int i = start + tid;
        bool keep = false;
        int64_t j = 0;
        if (i < m) {
            const unsigned long long k = p01[i];
            j = (int64_t)(k & 0xffffffffu);
            nn01_all[t.o0 + i] = j;
            dist01_all[t.o0 + i] = __uint_as_float((unsigned)(k >> 32));
            keep = j < (int64_t)t.m1 && (int64_t)(p10[j] & 0xffffffffu) == (int64_t)i;
        }
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_cnt[wv] = __popcll(mask);
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int cq = wave_cnt[q];
            if (q < wv) woff += cq;
            total += cq;
        }
        const int b0 = base;
        if (keep) {
            const int pos = b0 + woff + before;
            match_out[2 * pos] = t.rows0 ? t.rows0[i] : (int64_t)i;
            match_out[2 * pos + 1] = t.rows1 ? t.rows1[j] : j;
        }
        __syncthreads();
        if (tid == 0) base = b0 + total;
        __syncthreads();
    }
    if (tid == 0) counts[task] = base;
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
