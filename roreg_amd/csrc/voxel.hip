// Voxel-grid downsampling of a dense cloud on the device (include/roreg_hip.h, "v6e"; tests/_voxel_oracle.py is the numpy restatement).
// The reference's first upstream step (testset.py: ME.utils.sparse_quantize(xyz / voxel_size, return_index=True), np.floor(xyz / voxel_size)):
// one representative row per occupied voxel plus integer voxel coordinates -- here with every output defined independently of how the work
// was scheduled.
//
//   key     : per axis k = floor((double)x / voxel), ONE float64 division; valid keys -2^20 <= k < 2^20 pack into 63 bits, the all-ones word
//             is the empty marker of the table.
//   insert  : one lane per row, open addressing (linear probing from a mixed hash) in a table of 64-bit words, capacity a power of two
//             >= 2n: 64-bit compare-and-swap claims a slot, per slot an integer minimum of the row and an integer count.
//   number  : a row that is its slot's minimum is a voxel's lowest row; the exclusive scan of those flags over the rows (csrc/scan.h, the grid
//             build's three launches) numbers the voxels in ascending lowest row -- whatever the hash, the capacity or the atomics' order.
//   members : segment starts = the scan of the counts in voxel order, fill by an integer cursor, then every segment put in ascending row (a
//             record's place is the number of its segment's records with a lower row, as icp_rank_kernel), and one lane per voxel adds its
//             members in that order, starting from the first: a sequential float64 sum, no tree, no wave reduction, no floating-point atomic.
// Cost: linear in n, quadratic only in one voxel's occupancy; the cloud's extent does not enter (a far outlier is one more key).
// A row with a non-finite coordinate or a key out of range sets a flag in info[1], takes no slot and gets inverse = -1.
#include "common.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

#include "scan.h"
#include "voxel_hash.h"

constexpr int KEY_BITS = 21;
constexpr double KEY_LIM = 1048576.0;                     // 2^20
constexpr int MAX_ROWS = 1 << 30;                         // capacity 2n <= 2^31: a slot number fits an int32
enum { FLAG_NONFINITE = 1, FLAG_RANGE = 2, FLAG_TABLE = 4 };

struct Layout {
    size_t cap, keys, smin, scnt, slot, S, seg, cursor, tmp, members, bsum, bytes;
    int64_t nb;
};

Layout layout(int n) {
    Layout L;
    size_t cap = 64;
    while (cap < 2 * (size_t)n) cap <<= 1;
    L.cap = cap;
    L.nb = ((int64_t)n + 2 + SCAN_BLOCK - 1) / SCAN_BLOCK;
    size_t o = 0;
    L.keys = o; o += align_up(cap * 8, 256);
    L.smin = o; o += align_up(cap * 4, 256);
    L.scnt = o; o += align_up(cap * 4, 256);
    L.slot = o; o += align_up((size_t)n * 4, 256);
    L.S = o; o += align_up(((size_t)n + 1) * 4, 256);
    L.seg = o; o += align_up(((size_t)n + 2) * 4, 256);
    L.cursor = o; o += align_up((size_t)n * 4, 256);
    L.tmp = o; o += align_up((size_t)n * 4, 256);
    L.members = o; o += align_up((size_t)n * 4, 256);
    L.bsum = o; o += align_up((size_t)L.nb * 4, 256);
    L.bytes = o;
    return L;
}

// the table, the cursors and the counts-in-voxel-order are cleared by the call itself: nothing depends on what the workspace held
__global__ __launch_bounds__(256) void voxel_clear_kernel(unsigned long long *__restrict__ keys, int32_t *__restrict__ smin, int32_t *__restrict__ scnt,
                                                          size_t cap, int32_t *__restrict__ seg, int32_t *__restrict__ cursor, int n,
                                                          int32_t *__restrict__ info) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += stride) { keys[i] = EMPTY; smin[i] = 0x7fffffff; scnt[i] = 0; }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n + 2; i += stride) {
        seg[i] = 0;
        if (i < (size_t)n) cursor[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 2) info[threadIdx.x] = 0;
}

__global__ __launch_bounds__(256) void voxel_insert_kernel(const float *__restrict__ pts, int n, double voxel, unsigned long long *__restrict__ keys,
                                                           int32_t *__restrict__ smin, int32_t *__restrict__ scnt, size_t cap, int32_t *__restrict__ slot,
                                                           int32_t *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    int32_t s_out = -1;
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
        atomicOr(&info[1], FLAG_NONFINITE);
    } else {
        const double kx = floor((double)x / voxel), ky = floor((double)y / voxel), kz = floor((double)z / voxel);       // -0.0 -> voxel 0
        if (!(kx >= -KEY_LIM && kx < KEY_LIM && ky >= -KEY_LIM && ky < KEY_LIM && kz >= -KEY_LIM && kz < KEY_LIM)) {
            atomicOr(&info[1], FLAG_RANGE);
        } else {
            const unsigned long long key = ((unsigned long long)(long long)(kx + KEY_LIM) << (2 * KEY_BITS)) |
                                           ((unsigned long long)(long long)(ky + KEY_LIM) << KEY_BITS) | (unsigned long long)(long long)(kz + KEY_LIM);
            const long long s = hash_insert(keys, cap, key);          // csrc/voxel_hash.h: the probe is bounded by the capacity
            if (s >= 0) {
                atomicMin(&smin[s], i);
                atomicAdd(&scnt[s], 1);
                s_out = (int32_t)s;
            } else {
                atomicOr(&info[1], FLAG_TABLE);
            }
        }
    }
    slot[i] = s_out;
}

// S[i] = 1 iff row i is the lowest row of its voxel; S[n] = 0, so that the exclusive scan leaves the number of voxels there
__global__ __launch_bounds__(256) void voxel_flag_kernel(const int32_t *__restrict__ slot, const int32_t *__restrict__ smin, int n, size_t cap,
                                                         int32_t *__restrict__ S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    int f = 0;
    if (i < n) {
        const int32_t s = slot[i];
        f = s >= 0 && (size_t)s < cap && smin[s] == i;
    }
    S[i] = f;
}

// voxel number of row i = S[lowest row of its slot]; the lowest row writes its voxel's first, counts, coords and the count in voxel order
__global__ __launch_bounds__(256) void voxel_number_kernel(const int32_t *__restrict__ slot, const unsigned long long *__restrict__ keys,
                                                           const int32_t *__restrict__ smin, const int32_t *__restrict__ scnt, const int32_t *__restrict__ S,
                                                           int n, size_t cap, int32_t *__restrict__ inverse, int32_t *__restrict__ first,
                                                           int32_t *__restrict__ counts, int32_t *__restrict__ coords, int32_t *__restrict__ seg,
                                                           int32_t *__restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == 0) info[0] = S[n];
    const int32_t s = slot[i];
    int32_t v = -1;
    if (s >= 0 && (size_t)s < cap) {
        const int32_t f = smin[s];
        if (f >= 0 && f < n) v = S[f];
        if (v < 0 || v >= n) v = -1;
        if (v >= 0 && f == i) {
            const unsigned long long key = keys[s];
            const int32_t c = scnt[s];
            first[v] = i;
            counts[v] = c;
            coords[3 * (size_t)v] = (int32_t)((key >> (2 * KEY_BITS)) & 0x1fffff) - (1 << 20);
            coords[3 * (size_t)v + 1] = (int32_t)((key >> KEY_BITS) & 0x1fffff) - (1 << 20);
            coords[3 * (size_t)v + 2] = (int32_t)(key & 0x1fffff) - (1 << 20);
            seg[v] = c;
        }
    }
    inverse[i] = v;
}

// seg[v] = start of voxel v's segment (after the scan); a row's place inside it comes from an integer cursor, in whatever order
__global__ __launch_bounds__(256) void voxel_fill_kernel(const int32_t *__restrict__ inverse, const int32_t *__restrict__ seg, int n,
                                                         int32_t *__restrict__ cursor, int32_t *__restrict__ tmp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t v = inverse[i];
    if (v < 0 || v >= n) return;
    const int pos = seg[v] + atomicAdd(&cursor[v], 1);
    if (pos >= 0 && pos < n) tmp[pos] = i;
}

// canonical order inside a voxel: a row's place is the number of rows of its voxel that are lower (icp_rank_kernel's scheme)
__global__ __launch_bounds__(256) void voxel_rank_kernel(const int32_t *__restrict__ tmp, const int32_t *__restrict__ inverse, const int32_t *__restrict__ seg,
                                                         int n, int32_t *__restrict__ members) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || j >= seg[n]) return;                    // seg[n] = the rows that have a voxel (every row of a clean cloud)
    const int32_t row = tmp[j];
    if (row < 0 || row >= n) return;
    const int32_t v = inverse[row];
    if (v < 0 || v >= n) return;
    const int b = max(seg[v], 0), e = min(seg[v + 1], n);
    int rank = 0;
    for (int k = b; k < e; ++k) rank += tmp[k] < row;
    if (b + rank < n) members[b + rank] = row;
}

// one lane per voxel: the float64 sum of its members in ascending row, starting from the first member, and ONE float64 division
__global__ __launch_bounds__(256) void voxel_sum_kernel(const float *__restrict__ pts, const int32_t *__restrict__ members, const int32_t *__restrict__ seg,
                                                        const int32_t *__restrict__ S, int n, double *__restrict__ centroid) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n || v >= S[n]) return;
    const int b = max(seg[v], 0), e = min(seg[v + 1], n);
    if (e <= b) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = b; k < e; ++k) {
        const int32_t row = members[k];
        if (row < 0 || row >= n) continue;
        const double x = (double)pts[3 * (size_t)row], y = (double)pts[3 * (size_t)row + 1], z = (double)pts[3 * (size_t)row + 2];
        if (k == b) { sx = x; sy = y; sz = z; } else { sx += x; sy += y; sz += z; }
    }
    const double c = (double)(e - b);
    centroid[3 * (size_t)v] = sx / c;
    centroid[3 * (size_t)v + 1] = sy / c;
    centroid[3 * (size_t)v + 2] = sz / c;
}

void launch_scan(int32_t *S, int64_t m, int32_t *bsum, hipStream_t s) {
    const int64_t nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
    hipLaunchKernelGGL(icp_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const int32_t *)S, m, bsum);
    hipLaunchKernelGGL(icp_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, (int)nb);
    hipLaunchKernelGGL(icp_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, S, m, (const int32_t *)bsum);
}

}  // namespace

extern "C" size_t roreg_voxel_workspace(int n) {
    if (n < 0 || n > MAX_ROWS) return 0;
    return layout(n).bytes;
}

extern "C" int roreg_voxel_downsample(const float *points, int n, double voxel, int32_t *inverse, int32_t *first, int32_t *counts, int32_t *coords,
                                      double *centroid, int32_t *info, void *workspace, size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(n >= 0 && n <= MAX_ROWS && info, "roreg_voxel_downsample: bad arguments");
    ROREG_REQUIRE(voxel > 0.0 && std::isfinite(voxel), "roreg_voxel_downsample: voxel must be positive and finite");
    hipStream_t s = roreg::as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(info, 0, 8, s) != hipSuccess) {
            roreg::set_error("roreg_voxel_downsample: memset failed");
            return 1;
        }
        return 0;
    }
    ROREG_REQUIRE(points && inverse && first && counts && coords && centroid && workspace, "roreg_voxel_downsample: bad arguments");
    const Layout L = layout(n);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "roreg_voxel_downsample: workspace too small");
    char *w = reinterpret_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(w + L.keys);
    int32_t *smin = reinterpret_cast<int32_t *>(w + L.smin), *scnt = reinterpret_cast<int32_t *>(w + L.scnt), *slot = reinterpret_cast<int32_t *>(w + L.slot);
    int32_t *S = reinterpret_cast<int32_t *>(w + L.S), *seg = reinterpret_cast<int32_t *>(w + L.seg), *cursor = reinterpret_cast<int32_t *>(w + L.cursor);
    int32_t *tmp = reinterpret_cast<int32_t *>(w + L.tmp), *members = reinterpret_cast<int32_t *>(w + L.members), *bsum = reinterpret_cast<int32_t *>(w + L.bsum);
    const unsigned pb = (unsigned)(((int64_t)n + 255) / 256), pb1 = (unsigned)(((int64_t)n + 1 + 255) / 256);
    const unsigned cb = (unsigned)std::min<size_t>((L.cap + 255) / 256, 4096);
    hipLaunchKernelGGL(voxel_clear_kernel, dim3(cb), dim3(256), 0, s, keys, smin, scnt, L.cap, seg, cursor, n, info);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3(pb), dim3(256), 0, s, points, n, voxel, keys, smin, scnt, L.cap, slot, info);
    hipLaunchKernelGGL(voxel_flag_kernel, dim3(pb1), dim3(256), 0, s, (const int32_t *)slot, (const int32_t *)smin, n, L.cap, S);
    launch_scan(S, (int64_t)n + 1, bsum, s);
    hipLaunchKernelGGL(voxel_number_kernel, dim3(pb), dim3(256), 0, s, (const int32_t *)slot, (const unsigned long long *)keys, (const int32_t *)smin,
                       (const int32_t *)scnt, (const int32_t *)S, n, L.cap, inverse, first, counts, coords, seg, info);
    launch_scan(seg, (int64_t)n + 1, bsum, s);
    hipLaunchKernelGGL(voxel_fill_kernel, dim3(pb), dim3(256), 0, s, (const int32_t *)inverse, (const int32_t *)seg, n, cursor, tmp);
    hipLaunchKernelGGL(voxel_rank_kernel, dim3(pb), dim3(256), 0, s, (const int32_t *)tmp, (const int32_t *)inverse, (const int32_t *)seg, n, members);
    hipLaunchKernelGGL(voxel_sum_kernel, dim3(pb), dim3(256), 0, s, points, (const int32_t *)members, (const int32_t *)seg, (const int32_t *)S, n, centroid);
    ROREG_CHECK_LAUNCH("roreg_voxel_downsample");
    return 0;
}
