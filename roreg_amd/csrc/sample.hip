// Farthest-point sampling of dense clouds ("v6s").  No reference counterpart; tests/_fps_oracle.py is the numpy
// restatement and include/roreg_hip.h states the definition.  A strictly sequential loop of k steps, each a reduction over the whole cloud:
// one workgroup of 1024 lanes per task, persistent over the task's steps, many tasks per launch (roreg_fps_batch); and, for a single cloud so
// large that one compute unit is the bottleneck, one launch per step over many workgroups (roreg_fps_steps, at the end of this file).  No
// workgroup waits for another in either form, and both give the same bytes.
//
// The persistent form.
// State.  Lane t owns the rows t, t + 1024, t + 2048, ...  D[row] >= 0 is the row's squared distance to the selected set (+inf before the
// first selection); D[row] = -1 marks a row that is out: dead (a non-finite coordinate), taken, or past the cloud's end.  The sentinel is
// this file's flag for "excluded": a taken row's D is never used again by the definition, so nothing is lost by overwriting it.
//
// A step.  Every lane holds its best (D, row) from the previous update.  The wave reduces with __shfl_xor, its lane 0 stores the wave's best
// into LDS, ONE barrier, then every lane reduces the 16 wave results again (lanes l and l + 16 read the same word) and so holds the same
// winner: every exit condition is a function of words read from LDS after a barrier, all lanes leave the loop together and every barrier is
// reached by all 1024 lanes.  The wave results are double buffered by the step's parity: a wave stores into a buffer at step s + 2 only
// behind the barrier of step s + 1, which no wave passes before it has read the buffer at step s.  The order (D descending, row
// ascending) is total, so the winner does not depend on the shape of the reduction.
//
// Tiers (the host names one per task; include/roreg_hip.h): LDS = D in registers, coordinates staged once into LDS as three float arrays;
// REG = D in registers, coordinates read again every step; MEM = D in the workspace.  Register arrays are indexed by unrolled loop counters
// only (no scratch: the Makefile prints the resource report and fails on any).
#include "common.h"
#include <algorithm>
#include <cmath>
#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int FPS_THREADS = ROREG_FPS_THREADS;
constexpr int FPS_WAVES = FPS_THREADS / 64;
constexpr int FPS_LDS_ROWS = ROREG_FPS_LDS_MAX_N / FPS_THREADS;       // rows per lane, LDS tier
constexpr int FPS_REG_ROWS = ROREG_FPS_REG_MAX_N / FPS_THREADS;       // rows per lane, REG tier
constexpr int FPS_REG_CHUNK = 4;                                      // rows a lane loads before it computes: REG tier (8 spills) ...
constexpr int FPS_MEM_CHUNK = 8;                                      // ... and MEM tier
constexpr int FPS_MAX_N = 1 << 30;
static_assert(FPS_WAVES == 16 && FPS_LDS_ROWS * FPS_THREADS == ROREG_FPS_LDS_MAX_N && FPS_REG_ROWS * FPS_THREADS == ROREG_FPS_REG_MAX_N, "tier edges");
static_assert(FPS_REG_ROWS % FPS_REG_CHUNK == 0, "the REG tier walks whole chunks");
static_assert(sizeof(roreg_fps_task) == 64, "roreg_fps_task is 64 bytes");

struct Best {
    double d;
    int row;
};

// (D descending, row ascending): a total order
__device__ __forceinline__ bool better(double d, int row, const Best &b) { return d > b.d || (d == b.d && row < b.row); }

__device__ __forceinline__ void take(Best &b, double d, int row) {
    if (better(d, row, b)) {
        b.d = d;
        b.row = row;
    }
}

template <int FROM>
__device__ __forceinline__ void reduce_lanes(Best &b) {
#pragma unroll
    for (int off = FROM; off >= 1; off >>= 1) take(b, __shfl_xor(b.d, off), __shfl_xor(b.row, off));
}

struct Shared {
    float x[ROREG_FPS_LDS_MAX_N], y[ROREG_FPS_LDS_MAX_N], z[ROREG_FPS_LDS_MAX_N];
    double wave_d[2][FPS_WAVES];
    int wave_row[2][FPS_WAVES];
    roreg_fps_task task;
};
static_assert(sizeof(Shared) <= 163840, "one workgroup's LDS");

// the workgroup's winner from every lane's best, in every lane (one barrier)
__device__ __forceinline__ Best reduce_block(Shared &sh, Best b, int parity) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    reduce_lanes<32>(b);
    if (lane == 0) {
        sh.wave_d[parity][wave] = b.d;
        sh.wave_row[parity][wave] = b.row;
    }
    __syncthreads();
    Best w{sh.wave_d[parity][lane & (FPS_WAVES - 1)], sh.wave_row[parity][lane & (FPS_WAVES - 1)]};
    reduce_lanes<FPS_WAVES / 2>(w);
    return w;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// D of a row that is in (D >= 0) after the selection of row `win` at (cx, cy, cz); -1 for the selected row itself
__device__ __forceinline__ double updated(double D, int row, int win, float x, float y, float z, double cx, double cy, double cz) {
    const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    return row == win ? -1.0 : fmin(D, d2);
}

// The first-step candidate: `start` wins among the live rows (all at +inf) under the key -1, which the caller turns back into start.
__device__ __forceinline__ void first_candidate(Best &b, bool live, int row, int start) {
    if (live) take(b, (double)INFINITY, row == start ? -1 : row);
}

// The selection loop, shared by the tiers.  init(b): every lane sets its D and its first-step best.  coords(win, cx, cy, cz): the winner's
// coordinates, the same in every lane.  update(win, cx, cy, cz, b): D of the lane's rows and its next best.
template <class Init, class Coords, class Update>
__device__ __forceinline__ void select(Shared &sh, Init init, Coords coords, Update update) {
    const int k = sh.task.k, start = sh.task.start;
    const double stop2 = sh.task.stop2;
    int32_t *__restrict__ rows = sh.task.rows;
    double *__restrict__ dist2 = sh.task.dist2;
    Best b{-1.0, INT_MAX};
    init(b);
    int count = 0;
    for (int s = 0; s < k; ++s) {
        Best w = reduce_block(sh, b, s & 1);
        if (w.row == -1) w.row = start;
        if (w.d < 0.0 || (s >= 1 && w.d < stop2)) break;             // nothing left / closer than the stop distance: the same w in every lane
        if (threadIdx.x == 0) {
            rows[s] = w.row;
            dist2[s] = w.d;
        }
        count = s + 1;
        if (count == k) break;
        double cx, cy, cz;
        coords(w.row, cx, cy, cz);
        b = Best{-1.0, INT_MAX};
        update(w.row, cx, cy, cz, b);
    }
    for (int i = count + (int)threadIdx.x; i < k; i += FPS_THREADS) {
        rows[i] = -1;
        dist2[i] = 0.0;
    }
    if (threadIdx.x == 0) sh.task.count[0] = count;
}

// D in registers, R rows per lane.  IN_LDS: the coordinates are staged into sh.x / y / z once and read from there.
template <int R, bool IN_LDS>
__device__ __forceinline__ void run_registers(Shared &sh) {
    const int n = sh.task.n, start = sh.task.start, tid = threadIdx.x;
    const float *__restrict__ pts = sh.task.points;
    double D[R];
    auto load = [&](int row, float &x, float &y, float &z) {         // row < n
        if (IN_LDS) {
            x = sh.x[row]; y = sh.y[row]; z = sh.z[row];
        } else {
            const float *p = pts + (size_t)row * 3;
            x = p[0]; y = p[1]; z = p[2];
        }
    };
    select(
        sh,
        [&](Best &b) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = r * FPS_THREADS + tid;
                bool live = false;
                if (row < n) {
                    const float *p = pts + (size_t)row * 3;
                    const float x = p[0], y = p[1], z = p[2];
                    if (IN_LDS) {
                        sh.x[row] = x; sh.y[row] = y; sh.z[row] = z;
                    }
                    live = finite3(x, y, z);
                }
                D[r] = live ? (double)INFINITY : -1.0;
                first_candidate(b, live, row, start);
            }
            // (IN_LDS: the first reduce_block's barrier stands between these stores and the first read of another lane's row)
        },
        [&](int win, double &cx, double &cy, double &cz) {
            float x, y, z;
            load(win, x, y, z);
            cx = (double)x; cy = (double)y; cz = (double)z;
        },
        [&](int win, double cx, double cy, double cz, Best &b) {
            if (IN_LDS) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int row = r * FPS_THREADS + tid;            // < ROREG_FPS_LDS_MAX_N: inside the arrays whatever n is
                    if (D[r] >= 0.0) D[r] = updated(D[r], row, win, sh.x[row], sh.y[row], sh.z[row], cx, cy, cz);
                    if (D[r] > b.d) b = Best{D[r], row};              // rows ascend within a lane: the first of equal D stays
                }
            } else {
                // a chunk's loads go out together (the row clamped into the cloud, so they need no guard), then its arithmetic.  The lane
                // number goes through an empty asm once per step: the R row addresses are then values of this step and are computed where
                // they are used; as loop invariants of the step loop they were kept in 2 R registers and spilled.
                int t = tid;
                asm volatile("" : "+v"(t));
#pragma unroll
                for (int c = 0; c < R; c += FPS_REG_CHUNK) {
                    if (c * FPS_THREADS >= n) break;                  // (the same for every lane)
                    float x[FPS_REG_CHUNK], y[FPS_REG_CHUNK], z[FPS_REG_CHUNK];
#pragma unroll
                    for (int j = 0; j < FPS_REG_CHUNK; ++j) load(min((c + j) * FPS_THREADS + t, n - 1), x[j], y[j], z[j]);
#pragma unroll
                    for (int j = 0; j < FPS_REG_CHUNK; ++j) {
                        const int row = (c + j) * FPS_THREADS + t;
                        if (D[c + j] >= 0.0) D[c + j] = updated(D[c + j], row, win, x[j], y[j], z[j], cx, cy, cz);
                        if (D[c + j] > b.d) b = Best{D[c + j], row};
                    }
                }
            }
        });
}

// D in the workspace: lane t reads and writes the words of its own rows only.
__device__ __forceinline__ void run_memory(Shared &sh, double *__restrict__ D) {
    const int n = sh.task.n, start = sh.task.start, tid = threadIdx.x;
    const float *__restrict__ pts = sh.task.points;
    select(
        sh,
        [&](Best &b) {
            for (int64_t row = tid; row < n; row += FPS_THREADS) {
                const float *p = pts + (size_t)row * 3;
                const bool live = finite3(p[0], p[1], p[2]);
                D[row] = live ? (double)INFINITY : -1.0;
                first_candidate(b, live, (int)row, start);
            }
        },
        [&](int win, double &cx, double &cy, double &cz) {
            const float *p = pts + (size_t)win * 3;
            cx = (double)p[0]; cy = (double)p[1]; cz = (double)p[2];
        },
        [&](int win, double cx, double cy, double cz, Best &b) {
            int64_t base = tid;
            for (; base + (int64_t)(FPS_MEM_CHUNK - 1) * FPS_THREADS < n; base += (int64_t)FPS_MEM_CHUNK * FPS_THREADS) {       // whole chunks: every row < n
                float x[FPS_MEM_CHUNK], y[FPS_MEM_CHUNK], z[FPS_MEM_CHUNK];
                double d[FPS_MEM_CHUNK];
#pragma unroll
                for (int j = 0; j < FPS_MEM_CHUNK; ++j) {
                    const int64_t row = base + (int64_t)j * FPS_THREADS;
                    const float *p = pts + (size_t)row * 3;
                    x[j] = p[0]; y[j] = p[1]; z[j] = p[2];
                    d[j] = D[row];
                }
#pragma unroll
                for (int j = 0; j < FPS_MEM_CHUNK; ++j) {
                    const int64_t row = base + (int64_t)j * FPS_THREADS;
                    if (d[j] >= 0.0) {
                        d[j] = updated(d[j], (int)row, win, x[j], y[j], z[j], cx, cy, cz);
                        D[row] = d[j];
                    }
                    if (d[j] > b.d) b = Best{d[j], (int)row};
                }
            }
            for (int64_t row = base; row < n; row += FPS_THREADS) {
                const float *p = pts + (size_t)row * 3;
                double d = D[row];
                if (d >= 0.0) {
                    d = updated(d, (int)row, win, p[0], p[1], p[2], cx, cy, cz);
                    D[row] = d;
                }
                if (d > b.d) b = Best{d, (int)row};
            }
        });
}

__global__ __launch_bounds__(FPS_THREADS) void fps_batch_kernel(const roreg_fps_task *__restrict__ tasks, char *__restrict__ workspace, size_t workspace_bytes) {
    __shared__ Shared sh;
    if (threadIdx.x == 0) sh.task = tasks[blockIdx.x];
    __syncthreads();
    // everything below is a function of sh.task, read behind that barrier: the same in every lane
    const int n = sh.task.n, k = sh.task.k, tier = sh.task.tier;
    const int64_t off = sh.task.ws_off;
    bool ok = n > 0 && n <= FPS_MAX_N && k > 0;
    if (tier == ROREG_FPS_TIER_LDS) ok = ok && n <= ROREG_FPS_LDS_MAX_N;
    else if (tier == ROREG_FPS_TIER_REG) ok = ok && n <= ROREG_FPS_REG_MAX_N;
    else if (tier == ROREG_FPS_TIER_MEM) ok = ok && workspace && off >= 0 && (off & 7) == 0 && (size_t)off <= workspace_bytes && (size_t)n * 8 <= workspace_bytes - (size_t)off;
    else ok = false;
    if (!ok) {
        if (threadIdx.x == 0) sh.task.count[0] = 0;
        return;
    }
    if (tier == ROREG_FPS_TIER_LDS) run_registers<FPS_LDS_ROWS, true>(sh);
    else if (tier == ROREG_FPS_TIER_REG) run_registers<FPS_REG_ROWS, false>(sh);
    else run_memory(sh, reinterpret_cast<double *>(workspace + off));
}


// ---- the per-step launch form: one cloud over many workgroups -----------------------------------------------------------------------------
// For a single large cloud one compute unit is the bottleneck of the persistent form.  Here launch j = 0 sets D and leaves every workgroup's
// first candidate; launch j >= 1 starts by reducing the FS_BLOCKS-many candidates launch j - 1 left (every workgroup reduces all of them
// and so knows the winner of step s = j - 1: nothing waits on another workgroup, the launch boundary is the only ordering), workgroup 0
// writes the step's outputs, and every workgroup updates its rows against the winner and leaves its next candidate in the buffer of the
// other parity.  k + 1 launches, no host synchronisation: once the selection has ended (nothing left, or closer than the stop distance)
// the launch that sees it writes count and the tail of the outputs, and every workgroup leaves the candidate -2, which the launches behind
// it pass on and do nothing else.  Workgroup b's lane t owns the rows b 256 + t + i (blocks 256) in every launch.
constexpr int FS_THREADS = 256;
constexpr int FS_WAVES = FS_THREADS / 64;
constexpr int FS_ROWS = 4;                    // rows of a lane a launch loads before it computes; also the rows per lane the grid is sized for
constexpr int FS_MAX_BLOCKS = 1024;
constexpr double FS_ENDED = -2.0;

struct StepArgs {
    const float *points;
    int32_t *rows;
    double *dist2;
    int32_t *count;
    double stop2;
    double *D, *part_d;
    int32_t *part_row;
    int n, k, start, blocks;
};

int step_blocks(int n) { return (int)std::min<int64_t>(((int64_t)n + FS_THREADS * FS_ROWS - 1) / (FS_THREADS * FS_ROWS), FS_MAX_BLOCKS); }

struct StepLayout {
    size_t D, part_d, part_row, bytes;
};

StepLayout step_layout(int n) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t g = (size_t)std::max(step_blocks(n), 1);
    StepLayout L;
    L.D = 0;
    L.part_d = L.D + up((size_t)n * 8);
    L.part_row = L.part_d + up(2 * g * 8);
    L.bytes = L.part_row + up(2 * g * 4);
    return L;
}

// the workgroup's best from every lane's, in every lane (one barrier; sd / sr are this reduction's own)
__device__ __forceinline__ Best reduce_step_block(Best b, double *sd, int *sr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    reduce_lanes<32>(b);
    if (lane == 0) {
        sd[wave] = b.d;
        sr[wave] = b.row;
    }
    __syncthreads();
    Best w{sd[lane & (FS_WAVES - 1)], sr[lane & (FS_WAVES - 1)]};
    reduce_lanes<FS_WAVES / 2>(w);
    return w;
}

__global__ __launch_bounds__(FS_THREADS) void fps_step_kernel(StepArgs a, int j) {
    __shared__ double sd[2][FS_WAVES];
    __shared__ int sr[2][FS_WAVES];
    const int tid = threadIdx.x, G = a.blocks, n = a.n;
    const float *__restrict__ pts = a.points;
    double *__restrict__ D = a.D;
    double *pd_out = a.part_d + (size_t)(j & 1) * G;
    int32_t *pr_out = a.part_row + (size_t)(j & 1) * G;
    const int64_t first = (int64_t)blockIdx.x * FS_THREADS + tid, stride = (int64_t)G * FS_THREADS;
    Best b{-1.0, INT_MAX};
    if (j == 0) {
        for (int64_t row = first; row < n; row += stride) {
            const float *p = pts + (size_t)row * 3;
            const bool live = finite3(p[0], p[1], p[2]);
            D[row] = live ? (double)INFINITY : -1.0;
            first_candidate(b, live, (int)row, a.start);
        }
    } else {
        const double *pd_in = a.part_d + (size_t)((j - 1) & 1) * G;
        const int32_t *pr_in = a.part_row + (size_t)((j - 1) & 1) * G;
        Best w{-3.0, INT_MAX};                                       // below every candidate, FS_ENDED included
        for (int i = tid; i < G; i += FS_THREADS) take(w, pd_in[i], pr_in[i]);
        w = reduce_step_block(w, sd[0], sr[0]);                      // the same in every lane of every workgroup
        const int s = j - 1;
        if (w.row == -1) w.row = a.start;
        const bool ended_before = w.d == FS_ENDED, ends_here = !ended_before && (w.d < 0.0 || (s >= 1 && w.d < a.stop2));
        if (ended_before || ends_here) {
            if (ends_here) {
                if (blockIdx.x == 0 && tid == 0) a.count[0] = s;
                for (int64_t i = s + first; i < a.k; i += stride) {
                    a.rows[i] = -1;
                    a.dist2[i] = 0.0;
                }
            }
            if (tid == 0) {
                pd_out[blockIdx.x] = FS_ENDED;
                pr_out[blockIdx.x] = INT_MAX;
            }
            return;
        }
        if (blockIdx.x == 0 && tid == 0) {
            a.rows[s] = w.row;
            a.dist2[s] = w.d;
            if (j == a.k) a.count[0] = a.k;
        }
        if (j == a.k) return;
        const float *c = pts + (size_t)w.row * 3;
        const double cx = (double)c[0], cy = (double)c[1], cz = (double)c[2];
        int64_t base = first;
        for (; base + (int64_t)(FS_ROWS - 1) * stride < n; base += (int64_t)FS_ROWS * stride) {                      // whole groups: every row < n
            float x[FS_ROWS], y[FS_ROWS], z[FS_ROWS];
            double d[FS_ROWS];
#pragma unroll
            for (int q = 0; q < FS_ROWS; ++q) {
                const int64_t row = base + q * stride;
                const float *p = pts + (size_t)row * 3;
                x[q] = p[0]; y[q] = p[1]; z[q] = p[2];
                d[q] = D[row];
            }
#pragma unroll
            for (int q = 0; q < FS_ROWS; ++q) {
                const int64_t row = base + q * stride;
                if (d[q] >= 0.0) {
                    d[q] = updated(d[q], (int)row, w.row, x[q], y[q], z[q], cx, cy, cz);
                    D[row] = d[q];
                }
                if (d[q] > b.d) b = Best{d[q], (int)row};
            }
        }
        for (int64_t row = base; row < n; row += stride) {
            const float *p = pts + (size_t)row * 3;
            double d = D[row];
            if (d >= 0.0) {
                d = updated(d, (int)row, w.row, p[0], p[1], p[2], cx, cy, cz);
                D[row] = d;
            }
            if (d > b.d) b = Best{d, (int)row};
        }
    }
    b = reduce_step_block(b, sd[1], sr[1]);
    if (tid == 0) {
        pd_out[blockIdx.x] = b.d;
        pr_out[blockIdx.x] = b.row;
    }
}

}  // namespace

extern "C" size_t roreg_fps_workspace(int n) {
    if (n < 0 || n > FPS_MAX_N) return 0;
    return ((size_t)n * 8 + 255) & ~(size_t)255;
}

extern "C" int roreg_fps_batch(const roreg_fps_task *tasks_dev, int n_tasks, void *workspace, size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(n_tasks >= 0 && n_tasks <= (1 << 20), "roreg_fps_batch: bad sizes");
    if (n_tasks == 0) return 0;
    ROREG_REQUIRE(tasks_dev && (workspace || workspace_bytes == 0), "roreg_fps_batch: bad arguments");
    hipLaunchKernelGGL(fps_batch_kernel, dim3((unsigned)n_tasks), dim3(FPS_THREADS), 0, roreg::as_stream(stream), tasks_dev,
                       reinterpret_cast<char *>(workspace), workspace_bytes);
    ROREG_CHECK_LAUNCH("roreg_fps_batch");
    return 0;
}

extern "C" size_t roreg_fps_steps_workspace(int n) {
    if (n < 0 || n > FPS_MAX_N) return 0;
    return step_layout(n).bytes;
}

extern "C" int roreg_fps_steps(const float *points, int n, int k, int start, double stop2, int32_t *rows, double *dist2, int32_t *count, void *workspace,
                               size_t workspace_bytes, void *stream) {
    ROREG_REQUIRE(n >= 0 && n <= FPS_MAX_N && k >= 0 && count, "roreg_fps_steps: bad sizes");
    hipStream_t s = roreg::as_stream(stream);
    if (n == 0 || k == 0) {
        ROREG_REQUIRE(hipMemsetAsync(count, 0, sizeof(int32_t), s) == hipSuccess, "roreg_fps_steps: could not clear the count");
        return 0;
    }
    ROREG_REQUIRE(points && rows && dist2 && workspace && start >= 0 && start < n && stop2 >= 0.0, "roreg_fps_steps: bad arguments");
    const StepLayout L = step_layout(n);
    ROREG_REQUIRE(workspace_bytes >= L.bytes, "roreg_fps_steps: workspace too small");
    char *w = reinterpret_cast<char *>(workspace);
    StepArgs a{points, rows, dist2, count, stop2, reinterpret_cast<double *>(w + L.D), reinterpret_cast<double *>(w + L.part_d),
               reinterpret_cast<int32_t *>(w + L.part_row), n, k, start, step_blocks(n)};
    for (int j = 0; j <= k; ++j) hipLaunchKernelGGL(fps_step_kernel, dim3((unsigned)a.blocks), dim3(FS_THREADS), 0, s, a, j);
    ROREG_CHECK_LAUNCH("roreg_fps_steps");
    return 0;
}
