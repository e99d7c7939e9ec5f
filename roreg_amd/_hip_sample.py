"""ctypes binding of the farthest-point sampling kernel (csrc/sample.hip; include/roreg_hip.h "v6s"): part of the `roreg_amd.hip` namespace
(hip.py re-exports everything here).  No reference counterpart; tests/_fps_oracle.py restates the definition in numpy."""
import numpy as np
import torch

from ._abi import _FPS_TASK
from .hip import _check, _ptr, _stream, lib, upload

__all__ = ['FPS_MAX_N', 'FPS_THREADS', 'FPS_TIER_EDGES', 'FPS_TIERS', 'FPS_METHODS', 'FPS_STEPS_ROWS', 'fps_tier', 'fps_auto_steps', 'fps_batch', 'fps']

FPS_MAX_N = 1 << 30                    # csrc/sample.hip FPS_MAX_N
FPS_THREADS = 1024                     # == ROREG_FPS_THREADS: one workgroup per cloud
# == (ROREG_FPS_LDS_MAX_N, ROREG_FPS_REG_MAX_N): the greatest n of the tier that keeps the coordinates in LDS, and of the tier that keeps the
# running minima in registers and reads the coordinates again every step; above the second the minima live in the workspace
FPS_TIER_EDGES = (13312, 32768)
FPS_TIERS = ('lds', 'reg', 'mem')      # == ROREG_FPS_TIER_LDS / _REG / _MEM
# 'persistent': one workgroup per cloud, all clouds in one launch (roreg_fps_batch); 'steps': one cloud over many workgroups, one launch per
# step (roreg_fps_steps); the same bytes.  'auto': the clouds too large for the register tiers go through 'steps' when the call holds few of
# them (fps_auto_steps) -- few large clouds leave most of the device idle in the persistent form, many fill it.  Measured
# (tools/time_sample.py, profiles/fps_timing.txt): a step of the per-step form takes 5.2 - 6.2 us whatever n from 9,211 to 300,000 rows (it is
# bound by the launch), a step of the persistent form in the workspace tier 0.38 ns a row, and T clouds cost T times the first but once the
# second: the forms cross where T x 14,000 rows = n (T = 3 at 37,625 rows, 9 at 130,581, 18 at 300,000).
FPS_METHODS = ('auto', 'persistent', 'steps')
FPS_STEPS_ROWS = 16384


def fps_auto_steps(large_ns):
    """method 'auto': whether a call whose clouds above the register tiers have these row counts runs them through the per-step form"""
    return bool(large_ns) and len(large_ns) * FPS_STEPS_ROWS <= min(large_ns)


def fps_tier(n):
    """The tier a cloud of n rows runs in: the lowest that holds it."""
    return 0 if n <= FPS_TIER_EDGES[0] else 1 if n <= FPS_TIER_EDGES[1] else 2


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _fps_task(task, what):
    """(points, k[, start[, stop_dist]]) -> (points, n, k, start, stop2); ValueError otherwise, before any device call."""
    if not isinstance(task, (tuple, list)) or not 2 <= len(task) <= 4:
        raise ValueError(f'{what}: a task is (points, k[, start[, stop_dist]]), got {task!r}')
    pts, k = task[0], task[1]
    start = task[2] if len(task) > 2 else 0
    stop = task[3] if len(task) > 3 else None
    if not isinstance(pts, torch.Tensor) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3 or not pts.is_cuda or not pts.is_contiguous():
        raise ValueError(f'{what}: points must be a contiguous float32 [n,3] device tensor')
    n = int(pts.shape[0])
    if n > FPS_MAX_N:
        raise ValueError(f'{what}: {n} rows are more than the kernel numbers (2^30)')
    if not _is_int(k) or not 0 <= int(k) < 2 ** 31:
        raise ValueError(f'{what}: k must be an integer >= 0, got {k!r}')
    if not _is_int(start) or (n > 0 and not 0 <= int(start) < n):
        raise ValueError(f'{what}: start must be a row of the cloud (0 <= start < {n}), got {start!r}')
    stop2 = 0.0
    if stop is not None:
        ok = not isinstance(stop, (bool, str, bytes)) and isinstance(stop, (int, float, np.integer, np.floating))
        if not ok or not (float(stop) >= 0.0 and np.isfinite(float(stop))):
            raise ValueError(f'{what}: stop_dist must be a finite number >= 0 or None, got {stop!r}')
        stop2 = float(stop) * float(stop)
        if not np.isfinite(stop2):
            raise ValueError(f'{what}: the square of stop_dist {stop!r} is not finite')
    return pts, n, int(k), int(start) if n else 0, stop2


def fps_batch(tasks, tier=None, method='auto'):
    """tasks: [(points float32 [n,3] device tensor, k[, start = 0[, stop_dist = None]])] -> [(rows int32 [k], dist2 float64 [k], count int32 [1])]
    per task, device tensors: farthest-point sampling as include/roreg_hip.h "v6s" defines it.  rows are in selection order, -1 behind
    count; dist2[s] is the squared distance of row s to the rows before it when it was selected (dist2[0] = +inf, non-increasing), 0 behind
    count.  A non-finite row is never selected.  stop_dist: selection ends before the first row closer than that to the selected ones.  The
    same bytes on every run and from any batch.  One launch for all tasks, one workgroup per task, no read-back.
    method: FPS_METHODS above ('steps': every task with rows through the per-step launch form, k + 1 launches each).
    tier: None = by size (fps_tier), or 'lds' / 'reg' / 'mem' for every task (a tier at or above the task's own: the same bytes; for
    measurements and tests).  ValueError, before any device call: a bad shape or dtype, k < 0, start out of range, a negative or non-finite
    stop_dist, a tier that cannot hold a task."""
    parsed = [_fps_task(t, 'fps_batch') for t in tasks]
    if tier is not None and tier not in FPS_TIERS:
        raise ValueError(f'fps_batch: tier must be None or one of {FPS_TIERS}, got {tier!r}')
    if method not in FPS_METHODS:
        raise ValueError(f'fps_batch: method must be one of {FPS_METHODS}, got {method!r}')
    tiers = [fps_tier(n) if tier is None else FPS_TIERS.index(tier) for _, n, *_ in parsed]
    for (_, n, *_), t in zip(parsed, tiers):
        if t < fps_tier(n):
            raise ValueError(f'fps_batch: tier {FPS_TIERS[t]!r} does not hold a cloud of {n} rows')
    if not parsed:
        return []
    dev = parsed[0][0].device
    total_k = sum(p[2] for p in parsed)
    rows = torch.empty(total_k, dtype=torch.int32, device=dev)
    dist2 = torch.empty(total_k, dtype=torch.float64, device=dev)
    counts = torch.empty(len(parsed), dtype=torch.int32, device=dev)
    auto_steps = method == 'auto' and tier is None and fps_auto_steps([n for (_, n, k, *_), t in zip(parsed, tiers) if t == 2 and k])
    table = []
    ko = ws_n = 0
    out = []
    for q, ((pts, n, k, start, stop2), t) in enumerate(zip(parsed, tiers)):
        out.append((rows[ko:ko + k], dist2[ko:ko + k], counts[q:q + 1]))
        if n == 0 and k:                                          # the kernels write an empty cloud's count and nothing else
            out[-1][0].fill_(-1)
            out[-1][1].zero_()
        steps = n and k and (method == 'steps' or (auto_steps and t == 2))
        if steps:
            sw_n = lib().roreg_fps_steps_workspace(n)
            sw = torch.empty(sw_n, dtype=torch.uint8, device=dev)
            _check(lib().roreg_fps_steps(_ptr(pts), n, k, start, stop2, _ptr(out[-1][0]), _ptr(out[-1][1]), _ptr(out[-1][2]), _ptr(sw), sw_n, _stream()),
                   'roreg_fps_steps')
        else:
            table.append((pts.data_ptr() if n else 0, rows.data_ptr() + 4 * ko, dist2.data_ptr() + 8 * ko, counts.data_ptr() + 4 * q, stop2, ws_n, n, k, start, t))
            if t == 2 and n and k:
                ws_n += lib().roreg_fps_workspace(n)
        ko += k
    if table:
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev) if ws_n else None
        tdev = upload(np.array(table, _FPS_TASK).view(np.uint8).reshape(len(table), _FPS_TASK.itemsize))
        _check(lib().roreg_fps_batch(_ptr(tdev), len(table), _ptr(ws), ws_n, _stream()), 'roreg_fps_batch')
    return out


def fps(points, k, start=0, stop_dist=None, tier=None, method='auto'):
    """One task of fps_batch -> (rows int32 [k], dist2 float64 [k], count int32 [1]) device tensors."""
    return fps_batch([(points, k, start, stop_dist)], tier=tier, method=method)[0]
