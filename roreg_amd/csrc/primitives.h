// The small pieces of arithmetic the bit-exact matrix-core paths share, each defined once.  Every one is a contract between kernels (and with
// the host-side packers in roreg_amd/_hip_fourier.py): a copy that drifts breaks "a keypoint's result does not depend on its batch" silently.
#pragma once
#include <hip/hip_runtime.h>

// MFMA operand / accumulator registers
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <class T>
constexpr T round_up(T x, int a) { return (x + a - 1) / a * a; }

// Block scale of the fp16 x 2 operand split: e with bound * 2^e < 2^14 (bound = f * 2^ex, f in [0.5, 1)).  A pure function of the
// keypoint's own bound, so the producer (ft_nonlin) and the consumer (the GEMM's epilogue) derive the same exponent independently.
// Contracts: roreg_ft_nonlin_packed (fourier.hip) writes words scaled by it and group_conv_split_kernel<.., PK = 1> (group_conv.hip, row_scale_exp)
// decodes them; hip.bound_exp is the same rule on the host.
__device__ __forceinline__ int bound_exp(float mx) {
    int e = 0;
    if (mx > 0.f && mx < __builtin_inff()) { int ex; (void)frexpf(mx, &ex); e = 14 - ex; }
    return e > 100 ? 100 : (e < -100 ? -100 : e);
}

// bf16 x 3: v = b1 + b2 + b3 exactly, each piece the round-to-nearest-even bf16 of the remainder (8 + 8 + 8 significant bits; the GEMM that
// consumes them is described in fourier.hip).  The host packs weights with the same rule (_bf16_split3).
__device__ __forceinline__ void split3(const float (&v)[8], bf16x8 &b1, bf16x8 &b2, bf16x8 &b3) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h1 = (__bf16)v[e];
        const float r1 = v[e] - (float)h1;
        const __bf16 h2 = (__bf16)r1;
        const float r2 = r1 - (float)h2;
        b1[e] = h1; b2[e] = h2; b3[e] = (__bf16)r2;
    }
}

// fp16 x 2: hi = fp16(v * scale), lo = fp16(v * scale - hi)   (round-to-nearest-even conversions, the remainder is exact in f32)
// The host packs weights with the same rule (_f16_split2); the matcher, the irrep GEMMs and the group convolution split activations with it.
__device__ __forceinline__ void split2(const float (&v)[8], float scale, f16x8 &hi, f16x8 &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = v[e] * scale;
        const _Float16 h1 = (_Float16)x;
        hi[e] = h1; lo[e] = (_Float16)(x - (float)h1);
    }
}

// The split PRODUCT, the other half of the contract: which cross terms of the split operands are kept and the order they enter the float32
// accumulator.  a[p], b[p] are the planes of the two operands (p = 0 the leading piece; fp16 x 2: 0 = hi, 1 = lo):
//   bf16 x 3:  a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1   (the six terms of order <= 4, smallest first)
//   fp16 x 2:  lo hi, hi lo, hi hi                        (lo lo is dropped) -- the last three terms of the bf16 x 3 order
// The order is part of the result's bits.  "A keypoint's result does not depend on its batch" and the propagated bounds hold because every
// kernel that multiplies split operands issues exactly this sequence per K16 step: the group convolution and the dense layer
// (group_conv.hip), the irrep GEMMs and both transforms of ft_nonlin_kernel (fourier.hip), the mutual matchers (match_tile.h's tile product for mfma_match.hip and fpfh_match.hip; mfma_match.hip's strip kernels).
// Not this contract: linear_mfma.hip's four-term product (it keeps lo lo), ot_flash.hip's table-driven steps and its VAR ablations, and the
// 16x16x32 step of the LDS-DMA irrep GEMM (fourier.hip, defined once there).
__device__ __forceinline__ f32x16 mfma_32x32x16(const bf16x8 &a, const bf16x8 &b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma_32x32x16(const f16x8 &a, const f16x8 &b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
// one accumulator: c + a . b
template <int NP, class F>
__device__ __forceinline__ f32x16 split_mma(const F (&a)[NP], const F (&b)[NP], f32x16 c) {
    static_assert(NP == 2 || NP == 3, "fp16 x 2 or bf16 x 3");
    if constexpr (NP == 3) {
        c = mfma_32x32x16(a[2], b[0], c);
        c = mfma_32x32x16(a[1], b[1], c);
        c = mfma_32x32x16(a[0], b[2], c);
    }
    c = mfma_32x32x16(a[1], b[0], c);
    c = mfma_32x32x16(a[0], b[1], c);
    c = mfma_32x32x16(a[0], b[0], c);
    return c;
}
// two accumulators sharing b, the same terms interleaved c0, c1, c0, ...: two independent MFMA chains, as the 2 x 4 tile kernels issue them.
// (Written out a second time, operands copied to locals first: a form that derives both functions from one term list compiles, but not to the
// instruction streams the kernels had -- tools/compare_kernel_streams.py.)
template <int NP, class F>
__device__ __forceinline__ void split_mma_pair(const F (&a)[2][NP], const F (&b)[NP], f32x16 &c0, f32x16 &c1) {
    static_assert(NP == 2 || NP == 3, "fp16 x 2 or bf16 x 3");
    f32x16 x = c0, y = c1;
    const F b1 = b[0], b2 = b[1];
    if constexpr (NP == 3) {
        const F b3 = b[2];
        x = mfma_32x32x16(a[0][2], b1, x); y = mfma_32x32x16(a[1][2], b1, y);
        x = mfma_32x32x16(a[0][1], b2, x); y = mfma_32x32x16(a[1][1], b2, y);
        x = mfma_32x32x16(a[0][0], b3, x); y = mfma_32x32x16(a[1][0], b3, y);
    }
    x = mfma_32x32x16(a[0][1], b1, x); y = mfma_32x32x16(a[1][1], b1, y);
    x = mfma_32x32x16(a[0][0], b2, x); y = mfma_32x32x16(a[1][0], b2, y);
    x = mfma_32x32x16(a[0][0], b1, x); y = mfma_32x32x16(a[1][0], b1, y);
    c0 = x; c1 = y;
}

// Row of accumulator element r (0..15) of a 32x32 MFMA tile in lane (j = lane & 31, h = lane >> 5); the column is j.  `first`: the tile's first
// row in whatever the caller indexes; it is added on the left, the association every site's address arithmetic was compiled from (signed
// sums are not reassociated freely: cd_row32(r, h) + first compiles to other code in some kernels).
__host__ __device__ constexpr int cd_row32(int r, int h, int first = 0) { return first + (r & 3) + 8 * (r >> 2) + 4 * h; }

// The sum of v over the wave's 64 lanes, the same bits in every lane: a butterfly, lane l adding lane l ^ o for o = 32, 16, .. 1.  The order is
// part of the float64 sums' contracts (csrc/icp.hip's slots, csrc/ransac.hip's refinement sums).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// numpy's pairwise float32 sum for a contiguous run of n (8 <= n <= 128) elements, reproduced exactly
// (numpy/_core/src/umath/loops_utils.h.src, @TYPE@_pairwise_sum): eight strided partial sums, a fixed
// combine tree, then the tail.  Used so that the matcher's invariant descriptor (np.mean / np.sum,
// test/matcher.py:69-72) is bit-identical to the reference's on the same input.
__device__ __forceinline__ float np_pairwise_sum(const float *a, int n) {
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = __fadd_rn(r[j], a[i + j]);
    }
    float res = __fadd_rn(__fadd_rn(__fadd_rn(r[0], r[1]), __fadd_rn(r[2], r[3])),
                          __fadd_rn(__fadd_rn(r[4], r[5]), __fadd_rn(r[6], r[7])));
    for (; i < n; ++i) res = __fadd_rn(res, a[i]);
    return res;
}

// torch.clamp_min(norm, 1e-4) (network/group_feat.py:42-43): a NaN norm stays NaN (fmaxf would return the clamp and let the rest of a NaN's
// column, or of its keypoint's inv, through as finite values / 1e-4)
__device__ __forceinline__ float clamp_min_norm(float n) { return n < 1e-4f ? 1e-4f : n; }

// segment of row r in offsets off[0..n_seg] (off[n_seg] = total): the last s with off[s] <= r
__device__ __forceinline__ int seg_of(const int *__restrict__ off, int n_seg, int r) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one DPP move (no LDS crossbar): lanes without a source under CTRL / ROW_MASK keep x
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_mov(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), CTRL, ROW_MASK, 0xf, false));
}
