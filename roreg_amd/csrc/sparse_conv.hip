// Sparse 3-D convolutions on the device (include/roreg_hip.h, "v6j"; tests/_sparse_conv_oracle.py is the numpy restatement): the pieces of the
// FCGF backbone (roreg_amd/backbone/fcgf.py), the reference's MinkowskiEngine network, from integer coordinates to features.
//
//   coordinates : int32 [n,4] rows (item, x, y, z) at tensor stride ts; an item's rows are one contiguous segment.
//   key         : item in 15 bits beside three 16-bit axes (63 bits; the all-ones word is the table's empty marker, csrc/voxel_hash.h):
//                 0 <= item < 2^15, -2^15 <= x, y, z < 2^15.  A row outside sets FLAG_RANGE in info[1] and the caller refuses the result;
//                 a QUERY outside (a neighbour offset past the range) is simply absent.  No two rows alias.
//   stride map  : coarse coordinate = floor(c / (2 ts)) (2 ts) per axis; one lane per fine row inserts its coarse key, per slot an integer
//                 minimum of the row; a row that is its slot's minimum is a coarse voxel's lowest fine row, and the exclusive scan of those
//                 flags (csrc/scan.h) numbers the coarse rows in ascending lowest fine row -- whatever the hash or the atomics' order.
//                 Items are contiguous and ascending among the fine rows, so they are among the coarse rows: coarse_cuts[b] = S[cuts[b]].
//   kernel map  : a table of the input rows; one lane per (output row, kappa) looks out + offset(kappa) step up: int32 [n_out, K], -1 = none.
//                 kappa = kx + k ky + k^2 kz; step = ts (stride 1 and 2), -ts_fine (transposed: the strided map with in and out swapped).
//   convolution : output stationary.  A workgroup owns 64 output rows x TN output channels, loops kappa ascending, skips a kappa none of its rows
//                 has, gathers its input rows 32 channels at a time into LDS beside that slice of W[kappa], and every lane adds its rows' terms
//                 by fmaf in ascending (kappa, channel): float32 operands, no narrowing, a missing neighbour is a term left out.  No
//                 floating-point atomic: an output element's chain is fixed, so a row's result does not depend on the tile or the batch it is in.
//                 Epilogue: y scale + shift (one fmaf), + residual, relu, into a column window of a wider output.
#include "common.h"
#include <algorithm>

#pragma clang fp contract(off)

namespace {

#include "scan.h"
#include "voxel_hash.h"

constexpr int AXIS_BITS = 16, AXIS_LIM = 1 << 15, ITEM_LIM = 1 << 15;
constexpr int MAX_ROWS = 1 << 30;                         // capacity 2n <= 2^31: a slot number fits an int32
enum { FLAG_RANGE = 2, FLAG_TABLE = 4 };

struct Layout {
    size_t cap, keys, val, slot, S, bsum, bytes;
};

Layout layout(int n) {
    Layout L;
    size_t cap = 64;
    while (cap < 2 * (size_t)n) cap <<= 1;
    L.cap = cap;
    const size_t nb = ((size_t)n + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;
    size_t o = 0;
    L.keys = o; o += align_up(cap * 8, 256);
    L.val = o; o += align_up(cap * 4, 256);
    L.slot = o; o += align_up((size_t)n * 4, 256);
    L.S = o; o += align_up(((size_t)n + 1) * 4, 256);
    L.bsum = o; o += align_up(nb * 4, 256);
    L.bytes = o;
    return L;
}

__device__ __forceinline__ bool key_of(int item, int x, int y, int z, unsigned long long &key) {
    if (item < 0 || item >= ITEM_LIM || x < -AXIS_LIM || x >= AXIS_LIM || y < -AXIS_LIM || y >= AXIS_LIM || z < -AXIS_LIM || z >= AXIS_LIM) return false;
    key = ((unsigned long long)item << (3 * AXIS_BITS)) | ((unsigned long long)(x + AXIS_LIM) << (2 * AXIS_BITS)) |
          ((unsigned long long)(y + AXIS_LIM) << AXIS_BITS) | (unsigned long long)(z + AXIS_LIM);
    return true;
}

// c rounded down to a multiple of s (s > 0): a floor, -1 -> -s
__device__ __forceinline__ int floor_to(int c, int s) {
    const int r = c % s;
    return c - (r < 0 ? r + s : r);
}

__global__ __launch_bounds__(256) void sc_clear_kernel(unsigned long long *__restrict__ keys, int32_t *__restrict__ val, size_t cap, int32_t *__restrict__ info) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) { keys[i] = EMPTY; val[i] = 0x7fffffff; }
    if (blockIdx.x == 0 && threadIdx.x < 2) info[threadIdx.x] = 0;
}

// s2 > 0: the key is the row's coordinate rounded down to a multiple of s2 = 2 ts (stride map); s2 == 0: the row's own coordinate (kernel map).
// val[slot] = the lowest row of the slot's key.
__global__ __launch_bounds__(256) void sc_insert_kernel(const int32_t *__restrict__ coords, int n, int s2, unsigned long long *__restrict__ keys,
                                                        int32_t *__restrict__ val, size_t cap, int32_t *__restrict__ slot, int32_t *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t *c = coords + 4 * (size_t)i;
    int x = c[1], y = c[2], z = c[3];
    if (s2 > 0) { x = floor_to(x, s2); y = floor_to(y, s2); z = floor_to(z, s2); }
    unsigned long long key;
    int32_t s_out = -1;
    if (!key_of(c[0], x, y, z, key)) {
        atomicOr(&info[1], FLAG_RANGE);
    } else {
        const long long s = hash_insert(keys, cap, key);
        if (s >= 0) {
            atomicMin(&val[s], i);
            s_out = (int32_t)s;
        } else {
            atomicOr(&info[1], FLAG_TABLE);
        }
    }
    if (slot) slot[i] = s_out;
}

// S[i] = 1 iff fine row i is the lowest row of its coarse voxel; S[n] = 0, so that the exclusive scan leaves the number of coarse rows there
__global__ __launch_bounds__(256) void sc_flag_kernel(const int32_t *__restrict__ slot, const int32_t *__restrict__ val, int n, size_t cap, int32_t *__restrict__ S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    int f = 0;
    if (i < n) {
        const int32_t s = slot[i];
        f = s >= 0 && (size_t)s < cap && val[s] == i;
    }
    S[i] = f;
}

__global__ __launch_bounds__(256) void sc_number_kernel(const int32_t *__restrict__ coords, const int32_t *__restrict__ slot, const int32_t *__restrict__ val,
                                                        const int32_t *__restrict__ S, int n, int s2, size_t cap, const int32_t *__restrict__ cuts, int n_items,
                                                        int32_t *__restrict__ coarse, int32_t *__restrict__ parent, int32_t *__restrict__ coarse_cuts,
                                                        int32_t *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n_items) {                                   // n_items + 1 <= n + 1 cuts; the grid covers n + 1 lanes
        const int32_t c = cuts[i];
        coarse_cuts[i] = c >= 0 && c <= n ? S[c] : -1;
    }
    if (i >= n) return;
    if (i == 0) info[0] = S[n];
    const int32_t s = slot[i];
    int32_t v = -1;
    if (s >= 0 && (size_t)s < cap) {
        const int32_t f = val[s];
        if (f >= 0 && f < n) v = S[f];
        if (v < 0 || v >= n) v = -1;
        if (v >= 0 && f == i) {
            const int32_t *c = coords + 4 * (size_t)i;
            coarse[4 * (size_t)v] = c[0];
            coarse[4 * (size_t)v + 1] = floor_to(c[1], s2);
            coarse[4 * (size_t)v + 2] = floor_to(c[2], s2);
            coarse[4 * (size_t)v + 3] = floor_to(c[3], s2);
        }
    }
    parent[i] = v;
}

// one lane per (output row, kappa), 64-bit element index, grid-stride
__global__ __launch_bounds__(256) void sc_lookup_kernel(const int32_t *__restrict__ out, int n_out, int k, int step, const unsigned long long *__restrict__ keys,
                                                        const int32_t *__restrict__ val, size_t cap, int n_in, int32_t *__restrict__ map) {
    const int K = k * k * k, h = k / 2;
    const int64_t total = (int64_t)n_out * K, stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t u = e / K;
        const int kap = (int)(e - u * K);
        const int32_t *c = out + 4 * (size_t)u;
        // |offset| <= 171 * 2^15 and |c| < 2^31 - that only for coordinates the insert would have refused: compute in 64 bits, compare, then narrow
        const int64_t x = (int64_t)c[1] + (int64_t)(kap % k - h) * step, y = (int64_t)c[2] + (int64_t)(kap / k % k - h) * step,
                      z = (int64_t)c[3] + (int64_t)(kap / (k * k) - h) * step;
        int32_t row = -1;
        unsigned long long key;
        if (x >= -AXIS_LIM && x < AXIS_LIM && y >= -AXIS_LIM && y < AXIS_LIM && z >= -AXIS_LIM && z < AXIS_LIM && key_of(c[0], (int)x, (int)y, (int)z, key)) {
            const long long s = hash_find(keys, cap, key);
            if (s >= 0) {
                const int32_t r = val[s];
                if (r >= 0 && r < n_in) row = r;
            }
        }
        map[e] = row;
    }
}

// y scale + shift (folded BatchNorm, or the bias with scale null), + residual, relu: shared by both convolution kernels
__device__ __forceinline__ float epilogue(float y, int o, size_t u, const float *__restrict__ scale, const float *__restrict__ shift,
                                          const float *__restrict__ residual, int ldr, int relu) {
    if (scale) y = fmaf(y, scale[o], shift ? shift[o] : 0.0f);
    else if (shift) y = y + shift[o];
    if (residual) y = y + residual[u * (size_t)ldr + o];
    if (relu) y = fmaxf(y, 0.0f);
    return y;
}

constexpr int TM = 64, KC = 32;

template <int TN>
__global__ __launch_bounds__(256) void sparse_conv_kernel(const float *__restrict__ x, int ldx, int Cin, int n_in, const int32_t *__restrict__ map, int n_out,
                                                          int K, const float *__restrict__ W, int Cout, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, const float *__restrict__ residual, int ldr, int relu,
                                                          float *__restrict__ out, int ldo) {
    constexpr int CPT = 4, TX = TN / CPT, RPT = TM / (256 / TX);          // TN 64: 16 x 16 lanes of 4 rows x 4 channels; TN 32: 8 x 32 lanes of 2 x 4
    __shared__ float Xs[TM][KC + 1];
    __shared__ float Ws[KC][TN];
    __shared__ int32_t Ms[TM];
    const int t = threadIdx.x, tx = t % TX, ty = t / TX;
    const int64_t u0 = (int64_t)blockIdx.x * TM;
    const int n0 = blockIdx.y * TN;
    float acc[RPT][CPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r)
#pragma unroll
        for (int j = 0; j < CPT; ++j) acc[r][j] = 0.0f;
    for (int kap = 0; kap < K; ++kap) {
        int32_t m = -1;
        if (t < TM) {
            if (u0 + t < n_out) {
                m = map[(size_t)(u0 + t) * K + kap];
                if (m >= n_in) m = -1;                                    // a row the input does not have is never read
            }
            Ms[t] = m;
        }
        if (!__syncthreads_or(m >= 0)) continue;                          // an offset none of the tile's rows has
        bool has[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) has[r] = Ms[ty * RPT + r] >= 0;
        const float *Wk = W + (size_t)kap * Cin * Cout;
        for (int c0 = 0; c0 < Cin; c0 += KC) {
            const int kc = min(KC, Cin - c0);
            for (int i = t; i < TM * KC; i += 256) {
                const int r = i / KC, c = i % KC;
                const int32_t mm = Ms[r];
                Xs[r][c] = (mm >= 0 && c < kc) ? x[(size_t)mm * ldx + c0 + c] : 0.0f;
            }
            for (int i = t; i < KC * TN; i += 256) {
                const int c = i / TN, j = i % TN;
                Ws[c][j] = (c < kc && n0 + j < Cout) ? Wk[(size_t)(c0 + c) * Cout + n0 + j] : 0.0f;
            }
            __syncthreads();
            for (int c = 0; c < kc; ++c) {
                float w[CPT];
#pragma unroll
                for (int j = 0; j < CPT; ++j) w[j] = Ws[c][tx * CPT + j];
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    if (has[r]) {                                         // a missing neighbour is a term left out, not a product with zero
                        const float xv = Xs[ty * RPT + r][c];
#pragma unroll
                        for (int j = 0; j < CPT; ++j) acc[r][j] = fmaf(xv, w[j], acc[r][j]);
                    }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int64_t u = u0 + ty * RPT + r;
        if (u >= n_out) continue;
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            const int o = n0 + tx * CPT + j;
            if (o < Cout) out[(size_t)u * ldo + o] = epilogue(acc[r][j], o, (size_t)u, scale, shift, residual, ldr, relu);
        }
    }
}

// Cin = 1 (the network's first layer: K = 125 or 343 offsets of a one-channel input): one lane per (output row, channel), kappa ascending
__global__ __launch_bounds__(256) void sparse_conv_c1_kernel(const float *__restrict__ x, int ldx, int n_in, const int32_t *__restrict__ map, int n_out, int K,
                                                             const float *__restrict__ W, int Cout, const float *__restrict__ scale,
                                                             const float *__restrict__ shift, const float *__restrict__ residual, int ldr, int relu,
                                                             float *__restrict__ out, int ldo) {
    const int64_t total = (int64_t)n_out * Cout, stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const int64_t u = e / Cout;
        const int o = (int)(e - u * Cout);
        const int32_t *mu = map + (size_t)u * K;
        float acc = 0.0f;
        for (int kap = 0; kap < K; ++kap) {
            const int32_t m = mu[kap];
            if (m >= 0 && m < n_in) acc = fmaf(x[(size_t)m * ldx], W[(size_t)kap * Cout + o], acc);
        }
        out[(size_t)u * ldo + o] = epilogue(acc, o, (size_t)u, scale, shift, residual, ldr, relu);
    }
}

// out[u] = x[u] / sqrt(sum_c x[u][c]^2): the squares added by fmaf in ascending channel, one lane per row; no epsilon (the reference has none)
__global__ __launch_bounds__(256) void sparse_l2norm_kernel(const float *__restrict__ x, int n, int C, float *__restrict__ out) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    const float *xu = x + (size_t)u * C;
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s = fmaf(xu[c], xu[c], s);
    const float nrm = sqrtf(s);
    for (int c = 0; c < C; ++c) out[(size_t)u * C + c] = xu[c] / nrm;
}

void launch_scan(int32_t *S, int64_t m, int32_t *bsum, hipStream_t s) {
    const int64_t nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
    hipLaunchKernelGGL(icp_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const int32_t *)S, m, bsum);
    hipLaunchKernelGGL(icp_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, (int)nb);
    hipLaunchKernelGGL(icp_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, S, m, (const int32_t *)bsum);
}

}  // namespace

extern "C" size_t roreg_sparse_map_workspace(int n) {
    if (n < 0 || n > MAX_ROWS) return 0;
    return layout(n).bytes;
}

extern "C" int roreg_sparse_stride_map(const int32_t *coords, int n, int ts, const int32_t *cuts, int n_items, int32_t *coarse, int32_t *parent,
                                       int32_t *coarse_cuts, int32_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(n >= 1 && n <= MAX_ROWS && ts >= 1 && ts < AXIS_LIM && n_items >= 1 && n_items <= n && n_items <= ITEM_LIM,
                  "roreg_sparse_stride_map: bad arguments (n %d, ts %d, items %d)", n, ts, n_items);
    ROREG_REQUIRE(coords && cuts && coarse && parent && coarse_cuts && info && workspace, "roreg_sparse_stride_map: null argument");
    const Layout L = layout(n);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "roreg_sparse_stride_map: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    char *w = reinterpret_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w + L.keys);
    int32_t *val = reinterpret_cast<int32_t *>(w + L.val), *slot = reinterpret_cast<int32_t *>(w + L.slot), *S = reinterpret_cast<int32_t *>(w + L.S);
    int32_t *bsum = reinterpret_cast<int32_t *>(w + L.bsum);
    const unsigned pb = (unsigned)(((int64_t)n + 255) / 256), pb1 = (unsigned)(((int64_t)n + 1 + 255) / 256);
    const unsigned cb = (unsigned)std::min<size_t>((L.cap + 255) / 256, 4096);
    hipLaunchKernelGGL(sc_clear_kernel, dim3(cb), dim3(256), 0, s, keys, val, L.cap, info);
    hipLaunchKernelGGL(sc_insert_kernel, dim3(pb), dim3(256), 0, s, coords, n, 2 * ts, keys, val, L.cap, slot, info);
    hipLaunchKernelGGL(sc_flag_kernel, dim3(pb1), dim3(256), 0, s, (const int32_t *)slot, (const int32_t *)val, n, L.cap, S);
    launch_scan(S, (int64_t)n + 1, bsum, s);
    hipLaunchKernelGGL(sc_number_kernel, dim3(pb1), dim3(256), 0, s, coords, (const int32_t *)slot, (const int32_t *)val, (const int32_t *)S, n, 2 * ts, L.cap,
                       cuts, n_items, coarse, parent, coarse_cuts, info);
    ROREG_CHECK_LAUNCH("roreg_sparse_stride_map");
    return 0;
}

extern "C" int roreg_sparse_kernel_map(const int32_t *coords_in, int n_in, const int32_t *coords_out, int n_out, int k, int step, int32_t *map,
                                       int32_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(n_in >= 1 && n_in <= MAX_ROWS && n_out >= 1 && n_out <= MAX_ROWS && k >= 1 && k <= 7 && (k & 1) && step > -AXIS_LIM && step < AXIS_LIM && step != 0,
                  "roreg_sparse_kernel_map: bad arguments (n_in %d, n_out %d, k %d, step %d)", n_in, n_out, k, step);
    ROREG_REQUIRE(coords_in && coords_out && map && info && workspace, "roreg_sparse_kernel_map: null argument");
    const Layout L = layout(n_in);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "roreg_sparse_kernel_map: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    char *w = reinterpret_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w + L.keys);
    int32_t *val = reinterpret_cast<int32_t *>(w + L.val);
    const unsigned pb = (unsigned)(((int64_t)n_in + 255) / 256);
    const unsigned cb = (unsigned)std::min<size_t>((L.cap + 255) / 256, 4096);
    const int64_t total = (int64_t)n_out * k * k * k;
    const unsigned lb = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 20);
    hipLaunchKernelGGL(sc_clear_kernel, dim3(cb), dim3(256), 0, s, keys, val, L.cap, info);
    hipLaunchKernelGGL(sc_insert_kernel, dim3(pb), dim3(256), 0, s, coords_in, n_in, 0, keys, val, L.cap, (int32_t *)nullptr, info);
    hipLaunchKernelGGL(sc_lookup_kernel, dim3(lb), dim3(256), 0, s, coords_out, n_out, k, step, (const unsigned long long *)keys, (const int32_t *)val, L.cap,
                       n_in, map);
    ROREG_CHECK_LAUNCH("roreg_sparse_kernel_map");
    return 0;
}

extern "C" int roreg_sparse_conv(const float *x, int ldx, int Cin, int n_in, const int32_t *map, int n_out, int K, const float *W, int Cout,
                                 const float *scale, const float *shift, const float *residual, int ldr, int relu, float *out, int ldo, void *stream) {
    ROREG_REQUIRE(x && map && W && out, "roreg_sparse_conv: null argument");
    ROREG_REQUIRE(n_in >= 1 && n_out >= 1 && n_out <= MAX_ROWS && K >= 1 && K <= 343 && Cin >= 1 && Cin <= 4096 && Cout >= 1 && Cout <= 4096 && ldx >= Cin &&
                  ldo >= Cout && (!residual || ldr >= Cout) && (!scale || shift),
                  "roreg_sparse_conv: bad arguments (n_in %d, n_out %d, K %d, Cin %d / ldx %d, Cout %d / ldo %d, ldr %d)", n_in, n_out, K, Cin, ldx, Cout, ldo, ldr);
    hipStream_t s = roreg::as_stream(stream);
    if (Cin == 1) {
        const int64_t total = (int64_t)n_out * Cout;
        const unsigned gb = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)1 << 20);
        hipLaunchKernelGGL(sparse_conv_c1_kernel, dim3(gb), dim3(256), 0, s, x, ldx, n_in, map, n_out, K, W, Cout, scale, shift, residual, ldr, relu, out, ldo);
    } else if (Cout > 32) {
        const dim3 grid((unsigned)(((int64_t)n_out + TM - 1) / TM), (unsigned)((Cout + 63) / 64));
        hipLaunchKernelGGL(sparse_conv_kernel<64>, grid, dim3(256), 0, s, x, ldx, Cin, n_in, map, n_out, K, W, Cout, scale, shift, residual, ldr, relu, out, ldo);
    } else {
        const dim3 grid((unsigned)(((int64_t)n_out + TM - 1) / TM), 1);
        hipLaunchKernelGGL(sparse_conv_kernel<32>, grid, dim3(256), 0, s, x, ldx, Cin, n_in, map, n_out, K, W, Cout, scale, shift, residual, ldr, relu, out, ldo);
    }
    ROREG_CHECK_LAUNCH("roreg_sparse_conv");
    return 0;
}

extern "C" int roreg_sparse_l2norm(const float *x, int n, int C, float *out, void *stream) {
    ROREG_REQUIRE(x && out && n >= 1 && C >= 1, "roreg_sparse_l2norm: bad arguments");
    hipLaunchKernelGGL(sparse_l2norm_kernel, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, roreg::as_stream(stream), x, n, C, out);
    ROREG_CHECK_LAUNCH("roreg_sparse_l2norm");
    return 0;
}
