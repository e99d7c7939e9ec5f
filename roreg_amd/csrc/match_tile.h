// What the bit-exact matrix-core matchers share, each defined once: the per-tile passes of mfma_match.hip (F = 32) and fpfh_match.hip (F = 33), and
// the ordered compaction of mutual pairs that nn_search.hip uses as well.
//
// Why a bound plus a literal re-check is exact.  The reference's distance d = sqrtf(sum over ascending f of (s_f - t_f)^2 + 1e-7f) decides the
// nearest neighbour bit for bit, and a dot-product expansion a(i,j) rounds differently, so a cannot DECIDE -- but it can bound.  If |a - x| <= delta
// for the literal radicand x, the true first minimum j* of row i has a(i,j*) <= (min_j a(i,j)) + margin for a margin that covers 2 delta and the
// rounding of the literal formula itself (each matcher derives its own beside its constants).  Pass A finds the minima of a along rows and columns
// (one matrix serves both search directions: the literal formula is bitwise symmetric in (s, t)); pass B evaluates every entry within the margin of
// its row's or column's minimum -- a CANDIDATE -- with the literal formula and merges the results with a 64-bit atomicMin on the packed key
// (float_bits(d) << 32 | index).  d >= 0, so the integer order of the keys is the order of (d, index): the least d and, among equal d, the least
// index -- "first minimum wins", exactly as the literal scan (nn_search.hip) answers, and whatever the order the candidates arrive in.
#pragma once
#include "primitives.h"

namespace match_tile {

constexpr int TILE = 128, LP = 36;      // tile edge; row pitch of a staged tile in floats (conflict-free b128 fragment reads, see fpfh_match.hip)

// float -> unsigned with the same total order (a can be slightly negative)
__device__ __forceinline__ unsigned f2o(float x) { const unsigned b = __float_as_uint(x); return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float o2f(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// Block scale of a descriptor row for the fp16 x 2 split: e with 2^e |x| in [2^13, 2^14), from the row's squared norm (0 for a zero or
// non-finite norm)
__device__ __forceinline__ int norm_exp(float n2) {
    if (!(n2 > 0.f) || !(n2 < __builtin_inff())) return 0;
    int ex;
    (void)frexpf(n2, &ex);                          // n2 = m 2^ex, m in [0.5, 1): |x| = sqrt(n2) < 2^ceil(ex / 2)
    return 14 - ((ex + 1) >> 1);
}

// the reference's literal distance (nn_search.hip's arithmetic): one channel's step, the root, and the whole of it for contiguous rows
__device__ __forceinline__ float dist_step(float acc, float s, float t) {
    const float d = __fsub_rn(s, t);
    return __fadd_rn(acc, __fmul_rn(d, d));
}
__device__ __forceinline__ float dist_root(float acc) { return sqrtf(__fadd_rn(acc, 1e-7f)); }
template <int F>
__device__ __forceinline__ float exact_dist(const float *__restrict__ s, const float *__restrict__ t) {
    float acc = 0.f;
#pragma unroll
    for (int f = 0; f < F; ++f) acc = dist_step(acc, s[f], t[f]);
    return dist_root(acc);
}

// One 128 x 128 tile of a distance matrix as one of its 256 threads sees it.  4 waves as a 2 x 2 grid of 64 x 64 blocks (2 x 2 MFMA tiles each).
struct Tile {
    const float *S, *T;                     // [TILE][LP] staged rows of side 0 / side 1: channels 0..31 feed the matrix cores
    const float *xs0, *xs1, *is0, *is1;     // [TILE] the rows' scales 2^e and 2^-e (NP = 2; not read for NP = 3)
    int i0, j0, m0, m1;                     // the tile's first row and column, the matrix's real rows and columns (the rest of a tile is padding)
    int wm, wn, jl, h;                      // the wave's block: rows wm*64.., columns wn*64..; lane = h*32 + jl
};

// C = S.T^T over channels 0..31 (lanes own columns j) and, with BOTH, C' = T.S^T (lanes own columns i).  NP = 2: fp16 x 2 with the rows' scales,
// NP = 3: bf16 x 3.
template <int NP, bool BOTH>
__device__ __forceinline__ void tile_product(const Tile &t, f32x16 (&c)[2][2], f32x16 (&ct)[2][2]) {
    const int wm = t.wm, wn = t.wn, jl = t.jl, h = t.h;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { c[a][b][r] = 0.f; ct[a][b][r] = 0.f; }
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        using frag = typename std::conditional<NP == 3, bf16x8, f16x8>::type;
        frag sf[2][NP], tf[2][NP];                  // fragments of the wave's two 32-row groups of S (rows wm*64..) and T (rows wn*64..)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float x8[8];
            const int rs = wm * 64 + g * 32 + jl, rt = wn * 64 + g * 32 + jl;
            const float4 *ps = reinterpret_cast<const float4 *>(t.S + rs * LP + st * 16 + h * 8);
            const float4 u0 = ps[0], u1 = ps[1];
            x8[0] = u0.x; x8[1] = u0.y; x8[2] = u0.z; x8[3] = u0.w; x8[4] = u1.x; x8[5] = u1.y; x8[6] = u1.z; x8[7] = u1.w;
            if constexpr (NP == 3) split3(x8, sf[g][0], sf[g][1], sf[g][2]); else split2(x8, t.xs0[rs], sf[g][0], sf[g][1]);
            const float4 *pt = reinterpret_cast<const float4 *>(t.T + rt * LP + st * 16 + h * 8);
            const float4 v0 = pt[0], v1 = pt[1];
            x8[0] = v0.x; x8[1] = v0.y; x8[2] = v0.z; x8[3] = v0.w; x8[4] = v1.x; x8[5] = v1.y; x8[6] = v1.z; x8[7] = v1.w;
            if constexpr (NP == 3) split3(x8, tf[g][0], tf[g][1], tf[g][2]); else split2(x8, t.xs1[rt], tf[g][0], tf[g][1]);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                c[a][b] = split_mma<NP>(sf[a], tf[b], c[a][b]);                 // rows i = wm*64 + a*32 + .., column j = wn*64 + b*32 + jl
                if (BOTH) ct[a][b] = split_mma<NP>(tf[a], sf[b], ct[a][b]);     // rows j = wn*64 + a*32 + .., column i = wm*64 + b*32 + jl
            }
    }
}
// the dot product in real units: the accumulator times the exact 2^-e of its row, then of its column (both 1 for NP = 3)
template <int NP>
__device__ __forceinline__ float real_dot(float acc, float is_row, float is_col) { return NP == 2 ? (acc * is_row) * is_col : acc; }

// Pass A's epilogue.  a(i, j, dot) is the matcher's approximate squared distance of tile row i and tile column j from their dot product over
// channels 0..31.  Column minima of C, over the wave's 64 rows i, go to side 1's ordered keys am1[j]; column minima of C', over the wave's 64
// rows j, to side 0's am0[i] (both pointers at the tile's first row; pad rows keep their initial key).
template <int NP, class Entry>
__device__ __forceinline__ void tile_minima(const Tile &t, const f32x16 (&c)[2][2], const f32x16 (&ct)[2][2], Entry a, unsigned *am0, unsigned *am1) {
    const int wm = t.wm, wn = t.wn, jl = t.jl, h = t.h;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int jc = wn * 64 + b * 32 + jl;
        const float isj = t.is1[jc];
        float mn = __builtin_inff();
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ir = cd_row32(r, h, wm * 64 + g * 32);
                mn = fminf(mn, a(ir, jc, real_dot<NP>(c[g][b][r], t.is0[ir], isj)));
            }
        mn = fminf(mn, __shfl_xor(mn, 32));
        if (h == 0 && t.j0 + jc < t.m1) atomicMin(&am1[jc], f2o(mn));
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int ic = wm * 64 + b * 32 + jl;
        const float isi = t.is0[ic];
        float mn = __builtin_inff();
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jr = cd_row32(r, h, wn * 64 + g * 32);
                mn = fminf(mn, a(ic, jr, real_dot<NP>(ct[g][b][r], t.is1[jr], isi)));
            }
        mn = fminf(mn, __shfl_xor(mn, 32));
        if (h == 0 && t.i0 + ic < t.m0) atomicMin(&am0[ic], f2o(mn));
    }
}

// Pass B's epilogue.  thr0[i] / thr1[j]: the tile rows' and columns' thresholds (minimum of pass A plus the matcher's margin); an entry at or below
// one is a candidate of that row / column.  Candidates are evaluated with the literal F-channel formula from the staged rows and merged into the
// packed keys pk0[i] / pk1[j] (pointers at the tile's first row).  A pad row or column is nobody's candidate and has none.  debug: see NoDebug.
struct NoDebug {
    __device__ void entry(int i, int j, float av) const {}                    // every entry a(i, j) of the tile, pad rows and columns included
    __device__ void candidate(int i, int j, bool k0, bool k1) const {}        // every literal evaluation: for row i (k0), for column j (k1)
};
template <int NP, int F, class Entry, class Debug>
__device__ __forceinline__ void tile_verify(const Tile &t, const f32x16 (&c)[2][2], Entry a, const float *thr0, const float *thr1,
                                            unsigned long long *pk0, unsigned long long *pk1, Debug debug) {
    const int wm = t.wm, wn = t.wn, jl = t.jl, h = t.h;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int jc = wn * 64 + b * 32 + jl;
        const float isj = t.is1[jc], tj = thr1[jc];
        // candidate masks first (bit g*16 + r), the rare exact evaluations afterwards in ONE loop body: 64 inlined copies of the literal distance
        // are 100 KB of code and spill registers
        unsigned k0m = 0u, k1m = 0u;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ir = cd_row32(r, h, wm * 64 + g * 32);
                const float av = a(ir, jc, real_dot<NP>(c[g][b][r], t.is0[ir], isj));
                k0m |= (av <= thr0[ir] ? 1u : 0u) << (g * 16 + r);             // candidate of row i
                k1m |= (av <= tj ? 1u : 0u) << (g * 16 + r);                   // candidate of column j
                debug.entry(ir, jc, av);
            }
        if (!(t.j0 + jc < t.m1)) k0m = 0u;          // a pad column is nobody's candidate (its a is 1e30: not within any margin; said again here)
        unsigned m = k0m | k1m;
        while (m) {
            const int q = __ffs(m) - 1;
            m &= m - 1;
            const int ir = cd_row32(q & 15, h, wm * 64 + (q >> 4) * 32);
            const bool k0 = (k0m >> q) & 1u, k1 = ((k1m >> q) & 1u) && t.i0 + ir < t.m0;
            if (!(k0 || k1)) continue;
            const float d = exact_dist<F>(t.S + ir * LP, t.T + jc * LP);
            const unsigned long long db = (unsigned long long)__float_as_uint(d) << 32;
            // (keys only fall: one that is not below a plain load of the slot, however stale, cannot change it -- near-duplicate rows send
            //  most of their candidates to the same few slots)
            const unsigned long long key0 = db | (unsigned)(t.j0 + jc), key1 = db | (unsigned)(t.i0 + ir);
            if (k0 && key0 < pk0[ir]) atomicMin(&pk0[ir], key0);
            if (k1 && key1 < pk1[jc]) atomicMin(&pk1[jc], key1);
            debug.candidate(ir, jc, k0, k1);
        }
        // (the second column group's entries are not to be computed ahead of this loop: held across it they cost the registers of a third
        //  workgroup per CU)
        asm volatile("" ::: "memory");
    }
}

// The mutual check and the ordered compaction, by one workgroup of 1024 threads: for increasing i in [0, m0) with j = nn01(i) in [0, m1) and
// nn10(j) == i, the pair (rows0[i], rows1[j]) (a null row list: the index itself) goes to match_out; *count_out = the number of pairs.  An index
// outside [0, m1) -- one that no comparison ever set -- is "unmatched" and never dereferenced.  nn01 may have side effects: it is called once per i.
template <class NN01, class NN10>
__device__ __forceinline__ void compact_mutual(int m0, int m1, NN01 nn01, NN10 nn10, const int64_t *__restrict__ rows0,
                                               const int64_t *__restrict__ rows1, int64_t *__restrict__ match_out, int32_t *__restrict__ count_out) {
    __shared__ int wave_cnt[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < m0; start += 1024) {
        const int i = start + tid;
        bool keep = false;
        int64_t j = 0;
        if (i < m0) {
            j = nn01(i);
            keep = j >= 0 && j < (int64_t)m1 && nn10(j) == (int64_t)i;
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
            match_out[2 * pos] = rows0 ? rows0[i] : (int64_t)i;
            match_out[2 * pos + 1] = rows1 ? rows1[j] : j;
        }
        __syncthreads();
        if (tid == 0) base = b0 + total;
        __syncthreads();
    }
    if (tid == 0) *count_out = base;
}

}  // namespace match_tile
