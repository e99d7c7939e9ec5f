// Exclusive scan of an int32 array in place, three launches (block sums, scan of the block sums by one workgroup, apply): the grid build
// of csrc/icp.hip and the voxel numbering of csrc/voxel.hip launch the same three kernels.  Integer sums: the result does not depend on
// any order.  Included inside a translation unit's anonymous namespace.
#pragma once

constexpr int SCAN_PER_THREAD = 16, SCAN_BLOCK = 256 * SCAN_PER_THREAD;

// exclusive scan of S[0..m) in place, three launches: block sums, scan of the block sums (one workgroup), apply
__device__ __forceinline__ int block_excl_scan(int v, int *sh, int tid, int *total) {
    sh[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = tid >= o ? sh[tid - o] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const int incl = sh[tid];
    if (total) *total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void icp_scan_sums_kernel(const int32_t *__restrict__ S, int64_t m, int32_t *__restrict__ bsum) {
    __shared__ int sh[256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)tid * SCAN_PER_THREAD;
    int v = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (base + k < m) v += S[base + k];
    int total;
    block_excl_scan(v, sh, tid, &total);
    if (tid == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void icp_scan_top_kernel(int32_t *__restrict__ bsum, int nb) {
    __shared__ int sh[256];
    const int tid = threadIdx.x;
    const int per = (nb + 255) / 256;
    const int b0 = tid * per;
    int v = 0;
    for (int k = 0; k < per; ++k)
        if (b0 + k < nb) v += bsum[b0 + k];
    int run = block_excl_scan(v, sh, tid, nullptr);
    for (int k = 0; k < per; ++k)
        if (b0 + k < nb) { const int c = bsum[b0 + k]; bsum[b0 + k] = run; run += c; }
}

__global__ __launch_bounds__(256) void icp_scan_apply_kernel(int32_t *__restrict__ S, int64_t m, const int32_t *__restrict__ bsum) {
    __shared__ int sh[256];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * SCAN_BLOCK + (int64_t)tid * SCAN_PER_THREAD;
    int c[SCAN_PER_THREAD];
    int v = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) { c[k] = base + k < m ? S[base + k] : 0; v += c[k]; }
    int run = bsum[blockIdx.x] + block_excl_scan(v, sh, tid, nullptr);
    for (int k = 0; k < SCAN_PER_THREAD; ++k)
        if (base + k < m) { S[base + k] = run; run += c[k]; }
}
