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

// The sum of v over the wave's 64 lanes, the same bits in every lane: a butterfly, lane l adding lane l ^ o for o = 32, 16, .. 1.  The order is
// part of the float64 sums' contracts (csrc/icp.hip's slots, csrc/ransac.hip's refinement sums).
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

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
