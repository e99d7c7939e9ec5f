"""ctypes binding of the grid k-nearest-neighbour kernel (csrc/grid_knn.hip; include/roreg_hip.h "v6q"): part of the `roreg_amd.hip` namespace
(hip.py re-exports everything here).  No reference counterpart; tests/_grid_knn_oracle.py restates the definition in numpy.  `grid` is the
cloud's hip.IcpGrid, built for any radius (one built for the query radius walks the fewest cells)."""
import numpy as np
import torch

from .hip import _check, _ptr, _stream, lib

__all__ = ['GRID_KNN_MAX_K', 'grid_knn']

GRID_KNN_MAX_K = 32                    # csrc/grid_knn.hip KNN_MAX_K: the longest list a lane keeps


def grid_knn(grid, k, radius, queries=None, self_rows=None, want_mean=False, check_finite=True):
    """The k nearest rows of the grid's cloud within `radius` of every query -> (idx int32 [m,k], d2 float64 [m,k], count int32 [m][, mean_dist
    float64 [m]]) device tensors.  queries=None: the cloud's own rows, each excluding itself, in ORIGINAL row order.  queries float32 [m,3]
    (device): any finite points; self_rows int32 [m] (device): the cloud row each query excludes (-1: none).  Candidates are the rows with
    d2 <= radius^2, ordered by (d2, row); count is their number (not capped at k); the lists are padded with -1 / +inf; mean_dist is the mean of
    the listed distances, +inf for an empty list.  The same bytes from any grid of the cloud.
    ValueError: k outside 1..32, a radius that is not positive and finite, wrong shapes or dtypes, non-finite queries (check_finite=False skips
    that test and its read-back: for queries known to be finite, such as rows of the cloud)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= GRID_KNN_MAX_K:
        raise ValueError(f'grid_knn: k must be an integer in 1..{GRID_KNN_MAX_K}, got {k!r}')
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f'grid_knn: radius must be a positive finite number, got {radius!r}') from None
    if not (r > 0.0 and np.isfinite(r)):
        raise ValueError(f'grid_knn: radius must be positive and finite, got {radius!r}')
    k = int(k)
    if queries is None:
        if self_rows is not None:
            raise ValueError('grid_knn: self_rows needs queries (the cloud\'s own rows exclude themselves)')
        m = grid.n
    else:
        if not torch.is_tensor(queries) or queries.dtype != torch.float32 or queries.dim() != 2 or queries.shape[1] != 3:
            raise ValueError('grid_knn: queries must be a float32 tensor [m,3]')
        m = int(queries.shape[0])
        if self_rows is not None and (not torch.is_tensor(self_rows) or self_rows.dtype != torch.int32 or tuple(self_rows.shape) != (m,)):
            raise ValueError('grid_knn: self_rows must be an int32 tensor [m]')
        if check_finite and m and not bool(torch.isfinite(queries).all()):
            raise ValueError('grid_knn: queries must be finite')
    dev = grid.buf.device
    idx = torch.empty((m, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((m, k), dtype=torch.float64, device=dev)
    count = torch.empty(m, dtype=torch.int32, device=dev)
    mean = torch.empty(m, dtype=torch.float64, device=dev) if want_mean else None
    if m and grid.n:                   # (the kernel writes every row)
        _check(lib().roreg_grid_knn(_ptr(grid.buf), grid.n, k, r, _ptr(queries, torch.float32), _ptr(self_rows, torch.int32), m, _ptr(idx), _ptr(d2),
                                    _ptr(count), _ptr(mean), _stream()), 'roreg_grid_knn')
    else:                              # an empty cloud: every ball is empty
        idx.fill_(-1); d2.fill_(float('inf')); count.zero_()
        if want_mean:
            mean.fill_(float('inf'))
    return (idx, d2, count, mean) if want_mean else (idx, d2, count)
