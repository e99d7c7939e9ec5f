// DBSCAN clustering of a dense cloud from its grid ("v6r").  No reference counterpart; tests/_cluster_oracle.py is the
// numpy restatement.  Coordinates are float32 values widened to float64, d2 = (dx dx + dy dy) + dz dz with no FMA, rows i and j are neighbours
// iff d2 <= eps^2.  A row is core iff its ball holds at least min_points rows (itself included); clusters are the connected components of the
// neighbour graph on core rows; a non-core row with a core neighbour takes the cluster of the first one in (d2, row) order; the rest is noise.
// Every output is an integer defined by comparisons alone, so any grid of the cloud and any schedule give the same bytes.
//
// Five steps, ten launches (nine at min_points = 1), no host synchronisation:
//   count    one record per lane in cell order (a wave's lanes walk the same cells): core[row], parent[row] = row if core, -1 if not;
//   link     every core row takes its lowest core neighbour as its parent (plain stores to its own word; at min_points = 1 every row is core
//            and the count launch does this itself), then shortens its own word to where that chain ends: a forest of flat trees, one per
//            local minimum of the row number, before the first atomic;
//   hook     every core row walks its ball again and unites its tree with that of every core neighbour of a lower row (union-find, below);
//   settle   core rows shorten their own parent word to their root; non-core rows pick their core neighbour and take its root;
//   number   flag the roots, exclusive scan (csrc/scan.h, three launches), labels = the root's number, sizes by integer atomicAdd.
//
// The union-find.  parent[x] <= x for every core row x at all times: it starts as x or a lower neighbour and is only ever lowered, inside the
// hook launch by atomicMin alone.  A root is a row with parent[x] == x.  Every step only writes SMALLER values into a word, so the lowest core
// row of a component never receives a parent: when the hook launch has ended it is the component's one root whatever order the hooks landed
// in.  No lane ever waits for another's write: every loop below walks strictly decreasing row numbers and ends by itself (the argument
// stands at each loop).
#include "common.h"
#include "icp_grid.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

#include "scan.h"

constexpr int CL_THREADS = 256;
constexpr int CL_BLOCKS = 2048;         // as icp_normals_kernel: 256 CUs x 8 workgroups of 256, the launch strides over the records
constexpr int CL_MAX_N = 1 << 30;

struct Layout {
    size_t parent, S, bsum, bytes;
};

Layout layout(int n) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nb = ((size_t)n + 1 + SCAN_BLOCK - 1) / SCAN_BLOCK;
    Layout L;
    L.parent = 0;
    L.S = L.parent + up((size_t)n * 4);
    L.bsum = L.S + up(((size_t)n + 1) * 4);
    L.bytes = L.bsum + up(nb * 4);
    return L;
}

// A relaxed agent-scope load: inside the hook launch other workgroups lower these words, and a plain load might be served from a line the
// CU's vector cache still holds.  A stale value is an older parent of the same row, which is still a row of its component and still <= it.
__device__ __forceinline__ int load_parent(const int32_t *parent, int x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The row at the end of x's parent chain, as far as this lane can see.  Terminates: every step goes to a strictly smaller non-negative row
// (anything else ends the walk at once), so it takes at most x steps and waits for nobody.
__device__ __forceinline__ int find_root(const int32_t *parent, int x) {
    for (;;) {
        const int p = load_parent(parent, x);
        if (p < 0 || p >= x) return x;
        x = p;
    }
}

// Unite the trees of core rows a and b; returns the lower of the two rows the union ended on (an ancestor of both, for the caller's next find).
// Each round hooks the larger of two rows under the smaller with atomicMin on the larger one's parent word, which returns what the word held:
//   old == hi: hi was a root and now hangs under lo -- done;
//   old <  hi: hi had a parent already.  The word now holds min(old, lo), so one of the links hi - old, hi - lo is not in the forest: the
//              rows old and lo still have to be united, and this lane goes on with exactly that pair.  Nothing is lost: whichever link the
//              word dropped, hi stays joined to one of the two and the pair to each other.
// Terminates: the next pair is (find(old), find(lo)) with old < hi and lo < hi, and find never goes up, so the larger row of the pair falls
// strictly from round to round and is bounded by 0.  The retry follows an atomicMin that RETURNED a smaller row; it never polls a word until
// somebody else changes it.
__device__ __forceinline__ int unite(int32_t *parent, int a, int b) {
    int ra = find_root(parent, a), rb = find_root(parent, b);
    while (ra != rb) {
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicMin(parent + hi, lo);
        if (old >= hi || old < 0) return lo;       // hooked (old == hi; the other two cannot happen to a core row's word)
        ra = find_root(parent, old);
        rb = find_root(parent, lo);
    }
    return ra;
}

// ALL_CORE: min_points == 1, every row is core (its ball holds itself): the walk that counts also finds the lowest neighbour, link's work.
template <bool ALL_CORE>
__global__ __launch_bounds__(CL_THREADS) void cluster_count_kernel(const void *__restrict__ grid, int n, double thr2, double reach, int min_points,
                                                                   uint8_t *__restrict__ core, int32_t *__restrict__ parent, int32_t *__restrict__ sizes) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS) {
        sizes[i] = 0;
        const float4 p = rec[i];
        const int row = __float_as_int(p.w);
        if (row < 0 || row >= n) continue;               // a row the cloud does not have: a damaged grid writes nothing
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        int count = 0, low = row;
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;        // exact: both are float32 values
            if ((dx * dx + dy * dy) + dz * dz <= thr2) {
                ++count;
                const int j = __float_as_int(q.w);
                if (ALL_CORE && j >= 0) low = min(low, j);
            }
        });
        const bool is_core = ALL_CORE || count >= min_points;
        core[row] = is_core ? 1 : 0;
        parent[row] = is_core ? low : -1;
    }
}

// parent[row] = the lowest core row in row's ball (itself at most), for core rows: a lane writes its own word and reads `core` alone.
__global__ __launch_bounds__(CL_THREADS) void cluster_link_kernel(const void *__restrict__ grid, int n, double thr2, double reach, const uint8_t *__restrict__ core,
                                                                  int32_t *__restrict__ parent) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS) {
        const float4 p = rec[i];
        const int row = __float_as_int(p.w);
        if (row < 0 || row >= n || !core[row]) continue;
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        int low = row;
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
            const int j = __float_as_int(q.w);
            if (j < 0 || j >= low || !core[j]) return;
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
            if ((dx * dx + dy * dy) + dz * dz <= thr2) low = j;
        });
        parent[row] = low;
    }
}

// A core lane lowers its OWN word to its grandparent until its parent is a root.  It runs in launches where no root receives a parent (before
// and after the hook launch), so a lane that reads another's word meanwhile sees an ancestor either way.  Terminates: the word's value falls
// strictly from step to step.
__device__ __forceinline__ void shorten_own(int32_t *parent, int row) {
    int q = load_parent(parent, row);
    for (;;) {
        if (q < 0 || q >= row) return;                   // row is its own root
        const int gq = load_parent(parent, q);
        if (gq < 0 || gq >= q) return;                   // q is a root: settled
        __hip_atomic_store(parent + row, gq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        q = gq;
    }
}

__global__ __launch_bounds__(CL_THREADS) void cluster_shorten_kernel(const uint8_t *__restrict__ core, int n, int32_t *parent) {
    for (int row = blockIdx.x * CL_THREADS + threadIdx.x; row < n; row += gridDim.x * CL_THREADS)
        if (core[row]) shorten_own(parent, row);
}

__global__ __launch_bounds__(CL_THREADS) void cluster_hook_kernel(const void *__restrict__ grid, int n, double thr2, double reach, int32_t *parent) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS) {
        const float4 p = rec[i];
        const int row = __float_as_int(p.w);
        if (row < 0 || row >= n) continue;
        if (load_parent(parent, row) < 0) continue;      // not core (a core row's word never turns negative)
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        int mine = load_parent(parent, row);             // a row this lane knows its own tree to hold, the lower the better
        if (mine < 0 || mine > row) mine = row;
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
            const int j = __float_as_int(q.w);
            if (j < 0 || j >= row) return;               // every edge is taken once, from its higher row
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
            if (!((dx * dx + dy * dy) + dz * dz <= thr2)) return;
            const int pj = load_parent(parent, j);
            if (pj < 0) return;                          // not core
            if (pj == mine || j == mine) return;         // j hangs under a row this lane's tree holds already
            mine = unite(parent, mine, pj);              // (pj is j or an ancestor of it)
        });
    }
}

// After the hook launch the forest stands still except for what this launch does: a core lane shortens its OWN word (shorten_own); a non-core
// lane writes its own word once, and nobody reads a non-core word here (`core` tells them apart).  Both loops walk strictly decreasing rows and
// end by themselves.
__global__ __launch_bounds__(CL_THREADS) void cluster_settle_kernel(const void *__restrict__ grid, int n, double thr2, double reach,
                                                                    const uint8_t *__restrict__ core, int32_t *parent) {
    const GridDesc g = *grid_desc(grid);
    if (g.n != n) return;
    const float4 *__restrict__ rec = grid_recs(grid);
    const int32_t *__restrict__ st = grid_starts(grid, n);
    const double inv = 1.0 / g.edge;
    for (int i = blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += gridDim.x * CL_THREADS) {
        const float4 p = rec[i];
        const int row = __float_as_int(p.w);
        if (row < 0 || row >= n) continue;
        if (core[row]) {
            shorten_own(parent, row);
            continue;
        }
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        double best = (double)INFINITY;
        int bj = -1;
        walk_ball(g, rec, st, inv, px, py, pz, reach, [&](const float4 q) {
            const int j = __float_as_int(q.w);
            if (j < 0 || j >= n || !core[j]) return;
            const double dx = (double)q.x - px, dy = (double)q.y - py, dz = (double)q.z - pz;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (!(d2 <= thr2)) return;
            if (bj < 0 || d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; }
        });
        if (bj >= 0) parent[row] = find_root(parent, bj);                // (else it stays -1: noise)
    }
}

// S[i] = 1 iff row i is a root, S[n] = 0: after the exclusive scan S[root] is the cluster's number and S[n] the number of clusters.
__global__ __launch_bounds__(CL_THREADS) void cluster_flag_kernel(const int32_t *__restrict__ parent, int n, int32_t *__restrict__ S) {
    for (int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x; i <= n; i += (int64_t)gridDim.x * CL_THREADS) S[i] = (i < n && parent[i] == (int)i) ? 1 : 0;
}

// labels in original row order; a cluster's size is summed with integer atomicAdd (order-free), one add per distinct label of a wave.
__global__ __launch_bounds__(CL_THREADS) void cluster_label_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ S, int n,
                                                                   int32_t *__restrict__ labels, int32_t *__restrict__ n_clusters, int32_t *__restrict__ sizes) {
    if (blockIdx.x == 0 && threadIdx.x == 0) n_clusters[0] = S[n];
    const int lane = threadIdx.x & 63;
    // (the trip count is the same for a wave's 64 lanes: the ballots below need them all)
    for (int64_t base = (int64_t)blockIdx.x * CL_THREADS + (threadIdx.x - lane); base < n; base += (int64_t)gridDim.x * CL_THREADS) {
        const int64_t i = base + lane;
        int lab = -1;
        if (i < n) {
            const int r = parent[i];
            if (r >= 0 && r < n) lab = S[r];
            labels[i] = lab;
        }
        unsigned long long todo = __ballot(lab >= 0 && lab < n);
        while (todo) {                                   // ends: every round clears at least the leader's bit
            const int leader = __ffsll((long long)todo) - 1;
            const int l = __shfl(lab, leader);
            const unsigned long long same = __ballot(lab == l) & todo;
            if (lane == leader) atomicAdd(sizes + l, __popcll(same));
            todo &= ~same;
        }
    }
}

void launch_scan(int32_t *S, int64_t m, int32_t *bsum, hipStream_t s) {
    const int64_t nb = (m + SCAN_BLOCK - 1) / SCAN_BLOCK;
    hipLaunchKernelGGL(icp_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, s, (const int32_t *)S, m, bsum);
    hipLaunchKernelGGL(icp_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, (int)nb);
    hipLaunchKernelGGL(icp_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, s, S, m, (const int32_t *)bsum);
}

}  // namespace

extern "C" size_t roreg_cluster_workspace(int n) {
    if (n < 0 || n > CL_MAX_N) return 0;
    return layout(n).bytes;
}

extern "C" int roreg_grid_dbscan(const void *grid, int n, double eps, int min_points, int32_t *labels, uint8_t *core, int32_t *n_clusters, int32_t *sizes,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(eps > 0.0 && std::isfinite(eps), "roreg_grid_dbscan: eps must be positive and finite");
    ROREG_REQUIRE(min_points >= 1, "roreg_grid_dbscan: min_points must be at least 1");
    ROREG_REQUIRE(n >= 0 && n <= CL_MAX_N, "roreg_grid_dbscan: bad sizes");
    if (n == 0) return 0;
    ROREG_REQUIRE(grid && labels && core && n_clusters && sizes && workspace, "roreg_grid_dbscan: bad arguments");
    const Layout L = layout(n);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "roreg_grid_dbscan: workspace too small");
    hipStream_t s = roreg::as_stream(stream);
    char *w = reinterpret_cast<char *>(workspace);
    int32_t *parent = reinterpret_cast<int32_t *>(w + L.parent), *S = reinterpret_cast<int32_t *>(w + L.S), *bsum = reinterpret_cast<int32_t *>(w + L.bsum);
    const double thr2 = eps * eps, reach = eps * (1.0 + 1e-9);
    const dim3 threads(CL_THREADS);
    const dim3 rows((unsigned)std::min<int64_t>(((int64_t)n + CL_THREADS - 1) / CL_THREADS, CL_BLOCKS));
    const dim3 rows1((unsigned)std::min<int64_t>(((int64_t)n + 1 + CL_THREADS - 1) / CL_THREADS, CL_BLOCKS));
    if (min_points == 1) {
        hipLaunchKernelGGL(cluster_count_kernel<true>, rows, threads, 0, s, grid, n, thr2, reach, min_points, core, parent, sizes);
    } else {
        hipLaunchKernelGGL(cluster_count_kernel<false>, rows, threads, 0, s, grid, n, thr2, reach, min_points, core, parent, sizes);
        hipLaunchKernelGGL(cluster_link_kernel, rows, threads, 0, s, grid, n, thr2, reach, (const uint8_t *)core, parent);
    }
    hipLaunchKernelGGL(cluster_shorten_kernel, rows, threads, 0, s, (const uint8_t *)core, n, parent);
    hipLaunchKernelGGL(cluster_hook_kernel, rows, threads, 0, s, grid, n, thr2, reach, parent);
    hipLaunchKernelGGL(cluster_settle_kernel, rows, threads, 0, s, grid, n, thr2, reach, (const uint8_t *)core, parent);
    hipLaunchKernelGGL(cluster_flag_kernel, rows1, threads, 0, s, (const int32_t *)parent, n, S);
    launch_scan(S, (int64_t)n + 1, bsum, s);
    hipLaunchKernelGGL(cluster_label_kernel, rows, threads, 0, s, (const int32_t *)parent, (const int32_t *)S, n, labels, n_clusters, sizes);
    ROREG_CHECK_LAUNCH("roreg_grid_dbscan");
    return 0;
}
