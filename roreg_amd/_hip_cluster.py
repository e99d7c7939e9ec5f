"""ctypes binding of the DBSCAN clustering kernels (csrc/cluster.hip; include/roreg_hip.h "v6r"): part of the `roreg_amd.hip` namespace
(hip.py re-exports everything here).  No reference counterpart; tests/_cluster_oracle.py restates the definition in numpy.  `grid` is the
cloud's hip.IcpGrid, built for any radius (one built for eps walks the fewest cells)."""
import numpy as np
import torch

from .hip import _check, _ptr, _stream, lib

__all__ = ['CLUSTER_MAX_N', 'grid_dbscan']

CLUSTER_MAX_N = 1 << 30                # csrc/cluster.hip CL_MAX_N


def _dbscan_args(eps, min_points, what='grid_dbscan'):
    """-> (eps float, min_points int); ValueError otherwise."""
    ok = not isinstance(eps, (bool, str, bytes)) and isinstance(eps, (int, float, np.integer, np.floating))
    if not ok or not (float(eps) > 0.0 and np.isfinite(float(eps))):
        raise ValueError(f'{what}: eps must be a positive finite number, got {eps!r}')
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or not 1 <= int(min_points) < 2 ** 31:
        raise ValueError(f'{what}: min_points must be an integer >= 1, got {min_points!r}')
    return float(eps), int(min_points)


def grid_dbscan(grid, eps, min_points):
    """DBSCAN of the grid's cloud -> (labels int32 [n], core uint8 [n], n_clusters int32 [1], sizes int32 [n]) device tensors in ORIGINAL row
    order.  Rows are neighbours iff d2 <= eps^2 (float64); a row is core iff its ball holds at least min_points rows, itself included;
    clusters are the connected components of the core rows, numbered by ascending lowest core row; a non-core row with a core neighbour takes
    the cluster of the first one in (d2, row) order; every other row is noise, label -1.  sizes[c] = the rows (core and border) of cluster c,
    0 behind the last cluster.  The same bytes from any grid of the cloud and on every run; no read-back.
    ValueError, before any device call: an eps that is not positive and finite, a min_points that is not an integer >= 1, a grid that is none."""
    eps, min_points = _dbscan_args(eps, min_points)
    if not hasattr(grid, 'buf') or not hasattr(grid, 'n'):
        raise ValueError(f'grid_dbscan: grid must be a hip.IcpGrid, got {type(grid).__name__}')
    n = int(grid.n)
    if n > CLUSTER_MAX_N:
        raise ValueError(f'grid_dbscan: {n} rows are more than the kernels number (2^30)')
    dev = grid.buf.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    n_clusters = torch.zeros(1, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        ws_n = lib().roreg_cluster_workspace(n)
        ws = torch.empty(max(ws_n, 8), dtype=torch.uint8, device=dev)
        _check(lib().roreg_grid_dbscan(_ptr(grid.buf), n, eps, min_points, _ptr(labels), _ptr(core), _ptr(n_clusters), _ptr(sizes), _ptr(ws), ws_n,
                                       _stream()), 'roreg_grid_dbscan')
    return labels, core, n_clusters, sizes
