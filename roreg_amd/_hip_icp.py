"""ctypes bindings of the dense ICP kernels (csrc/icp.hip; include/roreg_hip.h "v6c", "v6d", "v6g", "v6i", "v6p"): part of the `roreg_amd.hip` namespace (hip.py
re-exports everything here).  No reference counterpart: the reference stops at the keypoint transform."""
import ctypes

import numpy as np
import torch

from ._abi import _ICP_GICP_ROBUST_TASK, _ICP_GICP_TASK, _ICP_GRID_DESC, _ICP_LOSS, _ICP_PLANE_ROBUST_TASK, _ICP_PLANE_TASK, _ICP_TASK
from .hip import HipError, _check, _ptr, _stream, lib, upload

__all__ = ['ICP_CHUNK', 'ICP_EVAL_STATUS', 'ICP_LOSSES', 'ICP_STATUS', 'IcpGrid', 'icp_batch', 'icp_box', 'icp_cell_edge', 'icp_eval_batch', 'icp_gicp_batch', 'icp_grid_desc', 'icp_normals', 'icp_plane_batch', 'icp_work_list']

ICP_CHUNK = 1024                       # source points per workgroup and per slot (csrc/icp.hip ICP_CHUNK)
ICP_STATUS = ('converged', 'max_iter', 'no_support', 'nonfinite')
ICP_EVAL_STATUS = ('ok', 'nonfinite')
ICP_LOSSES = tuple(_ICP_LOSS)          # 'huber', 'cauchy', 'gm', 'tukey': the loss= of icp_plane_batch and icp_gicp_batch (v6p)


def icp_box(points):
    """Bounding box [2,3] float64 (host) of a device cloud [n,3] float32: one synchronising read-back."""
    if int(points.shape[0]) == 0:
        return np.zeros((2, 3))
    box = torch.stack((points.amin(0), points.amax(0))).double().cpu().numpy()
    if not np.isfinite(box).all():
        raise HipError('icp: the cloud has non-finite coordinates')
    return box


def icp_grid_desc(box, n, max_dist):
    """-> (descriptor (numpy record array of one _ICP_GRID_DESC), grid buffer bytes, build workspace bytes): host arithmetic only."""
    lo, hi = np.ascontiguousarray(box[0], np.float64), np.ascontiguousarray(box[1], np.float64)
    desc = np.zeros(1, _ICP_GRID_DESC)
    ws_n = ctypes.c_size_t(0)
    nbytes = lib().roreg_icp_grid_size(lo.ctypes.data, hi.ctypes.data, int(n), float(max_dist), desc.ctypes.data, ctypes.byref(ws_n))
    if nbytes == 0:
        raise HipError(f'roreg_icp_grid_size failed: {lib().roreg_last_error().decode()}')
    return desc, int(nbytes), int(ws_n.value)


def icp_cell_edge(box, n, max_dist):
    """The cell edge a cloud's grid takes for this search radius: the smallest max_dist * 2^s whose table stays within 2^24 cells."""
    return float(icp_grid_desc(box, n, max_dist)[0]['edge'][0])


class IcpGrid:
    """A cloud's uniform grid for one search radius: points float32 [n,3] on the device, sorted by cell (ascending original row inside a
    cell) + the cell starts, one device buffer.  Building it reads the bounding box back once (the table's size depends on it); the
    iteration itself never returns to the host.  The same object serves as a pair's target (its cells are searched) and as a pair's
    source (its records are the source points in cell order)."""

    def __init__(self, points, max_dist, box=None):
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
            raise HipError('IcpGrid: points must be float32 [n,3]')
        _ptr(points, torch.float32)
        self.points = points
        self.n = int(points.shape[0])
        self.max_dist = float(max_dist)
        desc, nbytes, ws_bytes = icp_grid_desc(icp_box(points) if box is None else box, self.n, self.max_dist)
        self.desc = desc
        self.edge = float(desc['edge'][0])
        self.dims = tuple(int(v) for v in desc['dims'][0])
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
        ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=points.device)
        _check(lib().roreg_icp_grid_build(_ptr(points) if self.n else None, desc.ctypes.data, _ptr(self.buf), _ptr(ws), ws_bytes, _stream()),
               'roreg_icp_grid_build')

    def records(self):
        """-> (xyz float32 [n,3], original rows int32 [n]) in cell order (views of the grid buffer)."""
        rec = self.buf[64:64 + 16 * self.n].view(torch.float32).view(self.n, 4)
        return rec[:, :3], rec[:, 3].contiguous().view(torch.int32)

    def cell_starts(self):
        cells = int(self.desc['cells'][0])
        return self.buf[64 + 16 * self.n:64 + 16 * self.n + 4 * (cells + 1)].view(torch.int32)


def icp_work_list(n_src):
    """The ragged work list of a batch: n_src[p] source points of pair p -> (slot0 int32 [n], work int32 [n_work,2] rows (pair, chunk),
    total slots).  Pair p owns ceil(n_src[p] / ICP_CHUNK) consecutive slots whatever else is in the batch.  The rows are eight interleaved
    streams (row 8 i + k belongs to stream k; workgroups b and b + 8 are observed to share an XCD): a pair's rows go to ONE stream, the
    least loaded when the pair is dealt, so that its target cells are fetched into one XCD's L2 (fewer than eight pairs: each pair takes
    an equal share of the streams, in contiguous chunk ranges).  Short streams are padded with (-1, -1).  Placement is speed only."""
    n_src = [int(v) for v in n_src]
    chunks = [-(-v // ICP_CHUNK) for v in n_src]
    slot0 = np.zeros(len(n_src), np.int32)
    if len(n_src) > 1:
        slot0[1:] = np.cumsum(chunks[:-1])
    total = int(sum(chunks))
    streams = [[] for _ in range(8)]
    load = [0] * 8
    share = max(8 // max(len(n_src), 1), 1)
    for p, c in enumerate(chunks):
        if c == 0:
            continue
        if share == 1:
            ks = [min(range(8), key=lambda k: (load[k], k))]
        else:
            ks = list(range(p * share, (p + 1) * share))
        bounds = np.linspace(0, c, len(ks) + 1).astype(np.int64)
        for k, b, e in zip(ks, bounds[:-1], bounds[1:]):
            if e > b:
                streams[k].append(np.stack((np.full(e - b, p, np.int32), np.arange(b, e, dtype=np.int32)), 1))
                load[k] += int(e - b)
    depth = max(load)
    work = np.full((depth, 8, 2), -1, np.int32)
    for k in range(8):
        if streams[k]:
            rows = np.concatenate(streams[k])
            work[:rows.shape[0], k] = rows
    return slot0, work.reshape(depth * 8, 2), total


class _Launch:
    """What every batch entry needs beside its outputs: the task table on the device, the ragged work list, the workspace (sized by the
    library's `workspace_entry`) and, where wanted, the assignment buffer with the slice of it that task q owns."""

    def __init__(self, dtype, n_src, row, workspace_entry, n, want_assign, dev):
        self.slot0, work, self.total = icp_work_list(n_src)
        table = np.zeros(len(n_src), dtype)
        for q in range(len(n_src)):
            table[q] = row(q, int(self.slot0[q]))
        self.tasks = upload(table.view(np.uint8).reshape(len(n_src), dtype.itemsize))
        self.n_work = int(work.shape[0])
        self.work = upload(work) if self.n_work else None
        self.ws_n = getattr(lib(), workspace_entry)(n, self.total)
        self.ws = torch.empty(max(self.ws_n, 8), dtype=torch.uint8, device=dev)
        self.assign = torch.empty(max(self.total * ICP_CHUNK, 1), dtype=torch.int32, device=dev) if want_assign else None

    def rows(self, q, m):
        return self.assign[int(self.slot0[q]) * ICP_CHUNK:int(self.slot0[q]) * ICP_CHUNK + m]


def _run_batch(entry, dtype, pairs, row, stats_w, max_dist, max_iter, tol_deg, tol_t, want_assign, want_stats):
    """The iteration of any method.  pairs: tuples (target IcpGrid, source IcpGrid, ..., T0), validated by the caller; row(pair, slot0)
    -> the pair's record of `dtype`; stats_w: the width of the entry's statistics row."""
    n = len(pairs)
    dev = pairs[0][-1].device if n else torch.device('cuda')
    T = torch.empty((n, 4, 4), dtype=torch.float64, device=dev)
    iters = torch.empty(n, dtype=torch.int32, device=dev); inl = torch.empty_like(iters); status = torch.empty_like(iters)
    rmse = torch.empty(n, dtype=torch.float64, device=dev)
    out = [T, iters, inl, rmse, status]
    if n == 0:
        return tuple(out + ([[]] if want_assign else []) + ([torch.empty((0, stats_w), dtype=torch.float64, device=dev)] if want_stats else []))
    L = _Launch(dtype, [p[1].n for p in pairs], lambda q, slot0: row(pairs[q], slot0), entry + '_workspace', n, want_assign, dev)
    stats = torch.empty((n, stats_w), dtype=torch.float64, device=dev) if want_stats else None
    _check(getattr(lib(), entry)(_ptr(L.tasks), n, _ptr(L.work), L.n_work, L.total, float(max_dist), int(max_iter), float(tol_deg), float(tol_t),
                                 _ptr(T), _ptr(iters), _ptr(inl), _ptr(rmse), _ptr(status), _ptr(L.assign), _ptr(stats), _ptr(L.ws), L.ws_n, _stream()), entry)
    if want_assign:
        out.append([L.rows(q, p[1].n) for q, p in enumerate(pairs)])
    if want_stats:
        out.append(stats)
    return tuple(out)


def icp_batch(pairs, max_dist, max_iter=30, tol_deg=1e-4, tol_t=1e-6, want_assign=False, want_stats=False):
    """pairs: [(target IcpGrid, source IcpGrid, T0 [4,4] f64 device tensor)].  (A grid built for another radius is correct too: the search walks
    whatever cells a ball of max_dist meets; the radius it was built for keeps that to at most 3, rarely 4, cells per axis.)  All pairs iterate in the same
    launches, max_iter rounds enqueued at once, termination per pair on the device ->
    (T [n,4,4] f64, iters int32 [n], inliers int32 [n], rmse f64 [n], status int32 [n] (ICP_STATUS)) device tensors, and with want_assign
    a list of int32 [n_src] device tensors (target original row per source original row of the last executed search, -1 = no inlier), with
    want_stats f64 [n,16] = (n, c_q, c_p, H) of the last executed iteration."""
    for tgt, src, T0 in pairs:
        _ptr(T0, torch.float64)
        if tuple(T0.shape) != (4, 4):
            raise HipError('icp_batch: T0 must be [4,4] float64')
    return _run_batch('roreg_icp_batch', _ICP_TASK, pairs, lambda p, slot0: (p[0].buf.data_ptr(), p[1].buf.data_ptr(), p[2].data_ptr(), p[1].n, slot0), 16,
                      max_dist, max_iter, tol_deg, tol_t, want_assign, want_stats)


def icp_normals(grid, radius, min_neighbors=6):
    """Surface normals of the grid's cloud from the points within `radius` of each point (itself included): -> f64 [n,4] device tensor in
    ORIGINAL row order = (nx, ny, nz, number of neighbours m); a row with m < min_neighbors or a collinear neighbourhood carries the zero
    vector.  Any grid of the cloud gives the same table (one built for `radius` walks the fewest cells)."""
    if not (float(radius) > 0.0 and np.isfinite(float(radius))) or int(min_neighbors) < 1:
        raise HipError('icp_normals: radius must be positive and finite, min_neighbors >= 1')
    out = torch.empty((grid.n, 4), dtype=torch.float64, device=grid.buf.device)
    if grid.n:
        _check(lib().roreg_icp_normals(_ptr(grid.buf), float(radius), int(min_neighbors), _ptr(out), _stream()), 'roreg_icp_normals')
    return out


def _losses(what, n, loss, scale):
    """loss / scale of a batch of n pairs -> None (no loss anywhere in the call), or [(kind, k)] per pair.  Either argument is one value for
    every pair or a sequence of n; a pair's loss may be None (weight 1, through the weighted kernel) beside pairs that have one."""
    per_pair = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * n
    losses, scales = per_pair(loss), per_pair(scale)
    if len(losses) != n or len(scales) != n:
        raise HipError(f'{what}: loss and scale are one value or one per pair')
    if all(v is None for v in losses):
        if any(v is not None for v in scales):
            raise HipError(f'{what}: a scale without a loss')
        return None
    out = []
    for name, k in zip(losses, scales):
        if name is None:
            out.append((0, 1.0))
            continue
        if name not in _ICP_LOSS:
            raise HipError(f'{what}: loss must be one of {ICP_LOSSES} or None, got {name!r}')
        if k is None or not (float(k) > 0.0 and np.isfinite(float(k))):          # (NaN fails the comparison)
            raise HipError(f'{what}: loss {name!r} needs a positive, finite scale, got {k!r}')
        out.append((_ICP_LOSS[name], float(k)))
    return out


def icp_plane_batch(pairs, max_dist, max_iter=30, tol_deg=1e-4, tol_t=1e-6, want_assign=False, want_stats=False, loss=None, scale=None):
    """Point-to-plane form of icp_batch.  pairs: [(target IcpGrid, source IcpGrid, target normals f64 [n_tgt,4] (icp_normals), T0 [4,4] f64
    device tensor)].  The same returns as icp_batch with inliers = the correspondences that are within max_dist AND have a valid target
    normal, rmse = the root mean square of their plane residuals; with want_stats f64 [n,32] = (n_valid, c (3), the 21 upper entries of A,
    b (6), sum e^2) of the last executed iteration.
    loss (one of ICP_LOSSES) and scale (k > 0, in the unit of the coordinates), one value for the batch or one per pair: A and b with every
    correspondence weighted by the loss's weight of its plane residual e / k (roreg_icp_plane_robust_batch, v6p); inliers, rmse and sum e^2
    stay unweighted, the stats row holds the weighted A and b.  loss=None is the unweighted entry, bit for bit."""
    robust = _losses('icp_plane_batch', len(pairs), loss, scale)
    for tgt, src, nrm, T0 in pairs:
        _ptr(T0, torch.float64); _ptr(nrm, torch.float64)
        if tuple(T0.shape) != (4, 4):
            raise HipError('icp_plane_batch: T0 must be [4,4] float64')
        if tuple(nrm.shape) != (tgt.n, 4) or nrm.data_ptr() % 32:
            raise HipError('icp_plane_batch: the normal table must be [n_tgt,4] float64, 32-byte aligned')
    row = lambda p, slot0: (p[0].buf.data_ptr(), p[1].buf.data_ptr(), p[2].data_ptr(), p[3].data_ptr(), p[1].n, slot0)
    if robust is None:
        return _run_batch('roreg_icp_plane_batch', _ICP_PLANE_TASK, pairs, row, 32, max_dist, max_iter, tol_deg, tol_t, want_assign, want_stats)
    tagged = [tuple(p[:3]) + (lk, p[3]) for p, lk in zip(pairs, robust)]          # (T0 last: _run_batch takes the device from it)
    return _run_batch('roreg_icp_plane_robust_batch', _ICP_PLANE_ROBUST_TASK, tagged, lambda p, slot0: row(p[:3] + (p[4],), slot0) + (p[3][1], p[3][0], 0), 32,
                      max_dist, max_iter, tol_deg, tol_t, want_assign, want_stats)


def icp_gicp_batch(pairs, max_dist, max_iter=30, tol_deg=1e-4, tol_t=1e-6, want_assign=False, want_stats=False, loss=None, scale=None):
    """Plane-to-plane (generalized) form of icp_batch.  pairs: [(target IcpGrid, source IcpGrid, target normals f64 [n_tgt,4], source normals
    f64 [n_src,4] (icp_normals, both in original row order), T0 [4,4] f64 device tensor[, epsilon])], 0 < epsilon <= 1 (default 1e-3): every
    residual d = p' - q is weighted by (C_q + R C_p R^T)^-1 with C = I - (1 - epsilon) n n^T; a zero normal row leaves the identity, so
    nothing is skipped.  The same returns as icp_batch with inliers = the distance inliers and rmse = sqrt(sum d^T M d / n), the whitened
    residual; with want_stats f64 [n,32] = (n, c (3), the 21 upper entries of A, b (6), sum d^T M d) of the last executed iteration.
    loss, scale: as icp_plane_batch's, on the residual r = sqrt(2 epsilon d^T M d) -- the point-to-plane distance in metres where both normals
    agree, so one scale means the same under both methods (roreg_icp_gicp_robust_batch, v6p); inliers, rmse and sum d^T M d stay unweighted."""
    robust = _losses('icp_gicp_batch', len(pairs), loss, scale)
    full = []
    for pair in pairs:
        if len(pair) not in (5, 6):
            raise HipError('icp_gicp_batch: a pair is (target grid, source grid, target normals, source normals, T0[, epsilon])')
        tgt, src, nt, ns, T0 = pair[:5]
        eps = float(pair[5]) if len(pair) == 6 else 1e-3
        if nt is None or ns is None or T0 is None:
            raise HipError('icp_gicp_batch: both normal tables and T0 are required')
        _ptr(T0, torch.float64); _ptr(nt, torch.float64); _ptr(ns, torch.float64)
        if tuple(T0.shape) != (4, 4):
            raise HipError('icp_gicp_batch: T0 must be [4,4] float64')
        if tuple(nt.shape) != (tgt.n, 4) or nt.data_ptr() % 32:
            raise HipError('icp_gicp_batch: the target normal table must be [n_tgt,4] float64, 32-byte aligned')
        if tuple(ns.shape) != (src.n, 4) or ns.data_ptr() % 32:
            raise HipError('icp_gicp_batch: the source normal table must be [n_src,4] float64, 32-byte aligned')
        if not (0.0 < eps <= 1.0):                     # (NaN fails both comparisons)
            raise HipError(f'icp_gicp_batch: epsilon must be in (0, 1], got {eps!r}')
        full.append((tgt, src, nt, ns, eps, T0))       # (T0 last: _run_batch takes the device from it)
    row = lambda p, slot0: (p[0].buf.data_ptr(), p[1].buf.data_ptr(), p[2].data_ptr(), p[3].data_ptr(), p[-1].data_ptr(), p[4], p[1].n, slot0)
    if robust is None:
        return _run_batch('roreg_icp_gicp_batch', _ICP_GICP_TASK, full, row, 32, max_dist, max_iter, tol_deg, tol_t, want_assign, want_stats)
    tagged = [p[:5] + (lk, p[5]) for p, lk in zip(full, robust)]
    return _run_batch('roreg_icp_gicp_robust_batch', _ICP_GICP_ROBUST_TASK, tagged, lambda p, slot0: row(p, slot0) + (p[5][1], p[5][0], 0), 32,
                      max_dist, max_iter, tol_deg, tol_t, want_assign, want_stats)


def icp_eval_batch(pairs, max_dist, want_assign=False):
    """Read-only evaluation of pairs [(target IcpGrid, source IcpGrid, T [4,4] f64 device tensor)] in both directions (v6g) ->
    (stats f64 [n,8] = (n01, n10, overlap0, overlap1, rmse01, rmse10, S01, S10), info f64 [n,6,6], status int32 [n] (ICP_EVAL_STATUS))
    device tensors, and with want_assign two lists of int32 device tensors: the target original row per source original row, and the
    source original row per target original row (-1 = nothing within max_dist).  A pair's bits depend on neither the batch nor the radius
    its target grid was built for; the source grid's record order fixes the summation order."""
    n = len(pairs)
    dev = pairs[0][2].device if n else torch.device('cuda')
    stats = torch.empty((n, 8), dtype=torch.float64, device=dev)
    info = torch.empty((n, 6, 6), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return (stats, info, status) + (([], []) if want_assign else ())
    for tgt, src, T in pairs:
        _ptr(T, torch.float64)
        if tuple(T.shape) != (4, 4):
            raise HipError('icp_eval_batch: T must be [4,4] float64')

    def row(q, slot0):                     # tasks 0..n-1 forward, n..2n-1 backward: the grids swapped, the same T (the kernel inverts it)
        tgt, src, T = pairs[q % n]
        a, b = (tgt, src) if q < n else (src, tgt)
        return (a.buf.data_ptr(), b.buf.data_ptr(), T.data_ptr(), b.n, slot0)

    L = _Launch(_ICP_TASK, [src.n for _, src, _ in pairs] + [tgt.n for tgt, _, _ in pairs], row, 'roreg_icp_eval_workspace', n, want_assign, dev)
    _check(lib().roreg_icp_eval_batch(_ptr(L.tasks), n, _ptr(L.work), L.n_work, L.total, float(max_dist), _ptr(stats), _ptr(info), _ptr(status),
                                      _ptr(L.assign), _ptr(L.ws), L.ws_n, _stream()), 'roreg_icp_eval_batch')
    if not want_assign:
        return stats, info, status
    return (stats, info, status, [L.rows(i, src.n) for i, (_, src, _) in enumerate(pairs)], [L.rows(n + i, tgt.n) for i, (tgt, _, _) in enumerate(pairs)])
