// Assembly of a cloud's [N,F,60] group feature from the backbone's output on a batch of rotated copies (v6l; testset.py:170-181 of the
// reference: every rotated keypoint takes the feature row of its nearest down-sampled point, written to the rotation's group column).
//   out[n, f, g0 + r] = feats[cuts[r] + nn[r, n], f]                      r < R rotations of the batch, n < N keypoints, f < F channels
// A pure move: feature rows are read whole (F contiguous floats), turned in LDS, and leave as runs of R consecutive group columns per (n, f),
// so that a full batch (R = 60) writes a keypoint's 60 F values as one contiguous block.  No arithmetic but the optional rounding of the
// stored value to bfloat16 (round to nearest even, the conversion of gf_finalize_kernel in pointwise.hip); no atomics.
#include "common.h"

namespace {

constexpr int GFA_KP = 4;                          // keypoints per workgroup: one wave each
constexpr int GFA_MAX_F = ROREG_F;                 // the hot path's channel count bounds the LDS tile
constexpr int GFA_TILE = ROREG_G * (GFA_MAX_F + 1);

struct alignas(8) Bf16x4 { __bf16 v[4]; };

__device__ __forceinline__ void store4(float *p, float a, float b, float c, float d) { *reinterpret_cast<float4 *>(p) = make_float4(a, b, c, d); }
__device__ __forceinline__ void store4(__bf16 *p, float a, float b, float c, float d) {
    Bf16x4 q;
    q.v[0] = (__bf16)a; q.v[1] = (__bf16)b; q.v[2] = (__bf16)c; q.v[3] = (__bf16)d;
    *reinterpret_cast<Bf16x4 *>(p) = q;
}

// OT = float or __bf16 (the engine's storage types).  VEC: R and g0 are multiples of 4, so every run of R columns is a whole number of aligned
// 4-element stores (16 bytes of float32, 8 of bfloat16: a row of 60 columns starts on a 16-byte / 8-byte boundary for either type).
// LDS tile per wave: [R][F + 1] floats.  The load phase writes consecutive f (stride 1), the scalar store phase reads consecutive r (stride
// F + 1, odd for even F: conflict-free); the VEC phase reads four r per lane at stride 4 (F + 1), two lanes of a 32-lane half per bank.
// A source row outside its item (nn < 0, nn >= the item's rows, or past the end of feats) is never read: the element is stored as 0 and info[0]
// is set to 1 by a plain store (every writer stores the same word), which the caller reads back before it trusts `out`.
template <typename OT, bool VEC>
__global__ __launch_bounds__(64 * GFA_KP) void group_feature_assemble_kernel(const float *__restrict__ feats, int M, int F, const int32_t *__restrict__ cuts,
                                                                             const int64_t *__restrict__ nn, int R, int N, int g0, OT *__restrict__ out,
                                                                             int32_t *__restrict__ info) {
    __shared__ float tile[GFA_KP][GFA_TILE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x * GFA_KP + w;
    const bool live = n < N;
    const int S = F + 1;
    float *t = tile[w];
    // lane r < R resolves rotation r's source row once; the row loads below take it by a lane read and are independent of one another
    int src = -1;
    if (live && lane < R) {
        const int64_t a = cuts[lane], b = cuts[lane + 1], v = nn[(size_t)lane * N + n];
        if (v >= 0 && v < b - a && a >= 0 && a + v < (int64_t)M) src = (int)(a + v);
        else info[0] = 1;
    }
    const int total = R * F;
    for (int base = 0; base < total; base += 64) {                  // every lane takes every trip: the lane read below needs its source lane active
        const int i = min(base + lane, total - 1);
        const int r = i / F, f = i - r * F;
        const int row = __shfl(src, r);
        if (base + lane < total) t[r * S + f] = (live && row >= 0) ? feats[(size_t)row * F + f] : 0.f;
    }
    __syncthreads();
    if (!live) return;
    OT *dst = out + (size_t)n * F * ROREG_G + g0;
    if constexpr (VEC) {
        const int R4 = R >> 2;
        for (int q = lane; q < F * R4; q += 64) {
            const int f = q / R4, r = (q - f * R4) << 2;
            store4(dst + f * ROREG_G + r, t[r * S + f], t[(r + 1) * S + f], t[(r + 2) * S + f], t[(r + 3) * S + f]);
        }
    } else {
        for (int j = lane; j < total; j += 64) {
            const int f = j / R, r = j - f * R;
            dst[f * ROREG_G + r] = (OT)t[r * S + f];
        }
    }
}

template <typename OT>
void launch_assemble(const float *feats, int M, int F, const int32_t *cuts, const int64_t *nn, int R, int N, int g0, void *out, int32_t *info, hipStream_t s) {
    const dim3 grid((unsigned)((N + GFA_KP - 1) / GFA_KP)), block(64 * GFA_KP);
    OT *o = reinterpret_cast<OT *>(out);
    if ((R & 3) == 0 && (g0 & 3) == 0)
        hipLaunchKernelGGL((group_feature_assemble_kernel<OT, true>), grid, block, 0, s, feats, M, F, cuts, nn, R, N, g0, o, info);
    else
        hipLaunchKernelGGL((group_feature_assemble_kernel<OT, false>), grid, block, 0, s, feats, M, F, cuts, nn, R, N, g0, o, info);
}

}  // namespace

extern "C" int roreg_group_feature_assemble(const float *feats, int M, int F, const int32_t *cuts, const int64_t *nn, int R, int N, int g0, void *out,
                                            int out_bf16, int32_t *info, void *stream) {
    ROREG_REQUIRE(feats && cuts && nn && out && info, "roreg_group_feature_assemble: null argument");
    ROREG_REQUIRE(M >= 1 && F >= 1 && F <= GFA_MAX_F && N >= 1 && N <= (1 << 28) && R >= 1 && g0 >= 0 && g0 + R <= ROREG_G,
                  "roreg_group_feature_assemble: bad arguments (M %d, F %d (1..%d), N %d, R %d, g0 %d: columns g0 .. g0 + R - 1 of %d)", M, F, GFA_MAX_F, N, R,
                  g0, ROREG_G);
    hipStream_t s = roreg::as_stream(stream);
    if (out_bf16) launch_assemble<__bf16>(feats, M, F, cuts, nn, R, N, g0, out, info, s);
    else launch_assemble<float>(feats, M, F, cuts, nn, R, N, g0, out, info, s);
    ROREG_CHECK_LAUNCH("roreg_group_feature_assemble");
    return 0;
}
