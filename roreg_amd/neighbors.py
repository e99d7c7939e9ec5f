"""k nearest neighbours in a dense 3-D cloud on the device (csrc/grid_knn.hip; no reference counterpart: the
reference searches 5000 keypoints by brute force, which hip.knn_search keeps doing).

    from roreg_amd import neighbors
    res = neighbors.knn(points, 16, radius=0.1)          # -> KnnResult: the 16 nearest within 0.1 of every point, itself excluded
    res = neighbors.knn(points, 16)                      # the exact 16 nearest, whatever their distance
    res = neighbors.knn(points, 16, queries=other)       # of other points (nothing excluded)

Coordinates are rounded to float32 once, at upload; distances are float64, neighbours ordered by (d2, row)."""
from collections import namedtuple

import numpy as np
import torch

from . import hip

KnnResult = namedtuple('KnnResult', 'idx d2 count')
KnnResult.__doc__ = ('device tensors: idx int32 [m,k] (rows of the cloud, -1 behind the last neighbour), d2 float64 [m,k] (squared distances, +inf there), '
                     'count int32 [m]: with a radius the number of rows in the ball (NOT capped at k), without one the number of entries listed')


def _device_points(pts, device):
    from .icp import device_points
    return device_points(pts, device)


def start_radius(box, n, k):
    """The radius the escalation starts from: that of the ball which holds k points at the mean density of the cloud's bounding box (host
    arithmetic; speed only -- a surface fills its box thinly, so its rows are served in the first round and stray points in later ones)."""
    ext = np.asarray(box[1], np.float64) - np.asarray(box[0], np.float64)
    diag = float(np.sqrt((ext * ext).sum()))
    if not diag > 0.0:
        return 1.0
    r = (3.0 * k * float(np.prod(ext)) / (4.0 * np.pi * max(int(n), 1))) ** (1.0 / 3.0)
    return max(r, 1e-3 * diag)


def device_knn(pts, k, radius=None, queries=None, want_mean=False, start=None, box=None, info=None):
    """knn on device tensors (pts float32 [n,3], queries float32 [m,3] or None) -> (idx, d2, count, mean_dist or None).  info: a dict that
    receives 'rounds' and 'radii'."""
    n = int(pts.shape[0])
    own = queries is None
    m = n if own else int(queries.shape[0])
    if radius is not None:
        out = hip.grid_knn(hip.IcpGrid(pts, float(radius), box), k, radius, queries, None, want_mean)
        return tuple(out) + (() if want_mean else (None,))
    # Escalation: a row whose ball held at least `need` candidates has its true nearest already, so the rounds only revisit the rows that are
    # short, at twice the radius, until none is or the ball covers the box (then every row is a candidate of every query).
    need = min(int(k), n - 1 if own else n)
    if box is None:
        box = hip.icp_box(pts)
    lo, hi = np.array(box[0], np.float64), np.array(box[1], np.float64)
    if not own and m and n:
        qb = hip.icp_box(queries)
        lo, hi = np.minimum(lo, qb[0]), np.maximum(hi, qb[1])
    diag = float(np.sqrt(((hi - lo) ** 2).sum()))
    r_max = 1.001 * diag if diag > 0.0 else 1.0
    r = min(float(start) if start is not None else start_radius(box, n, k), r_max)
    if not (r > 0.0 and np.isfinite(r)):
        raise ValueError(f'knn: the starting radius must be positive and finite, got {start!r}')
    idx, d2, count, mean = hip.grid_knn(hip.IcpGrid(pts, r, box), k, r, queries, None, True, check_finite=not own)
    radii = [r]
    if need > 0 and m:
        short = (count < need).nonzero().reshape(-1)
        while int(short.shape[0]) and r < r_max:             # (the one read-back of a round)
            r = min(2.0 * r, r_max)
            radii.append(r)
            q = (pts if own else queries).index_select(0, short).contiguous()
            si, sd, sc, sm = hip.grid_knn(hip.IcpGrid(pts, r, box), k, r, q, short.to(torch.int32) if own else None, True, check_finite=False)
            idx[short] = si; d2[short] = sd; count[short] = sc; mean[short] = sm
            short = short[sc < need]
    if info is not None:
        info.update(rounds=len(radii), radii=radii)
    return idx, d2, torch.clamp(count, max=int(k)), (mean if want_mean else None)


def knn(points, k, radius=None, queries=None, device='cuda', start_radius=None, info=None):
    """The k nearest rows of a cloud [n,3] (host array or tensor) for each of its own rows (itself excluded; duplicates of it are listed) or for
    `queries` [m,3] -> KnnResult.  k: 1..32.  radius: only rows with d2 <= radius^2, one kernel call.  radius=None: the exact k nearest
    (min(k, n - 1) of them for the cloud's own rows), found by doubling the radius for the rows whose ball was short; start_radius: where that
    begins (default: from the cloud's density; the result does not depend on it); info: a dict that receives the number of rounds."""
    pts = _device_points(points, device)
    q = None if queries is None else _device_points(queries, device)
    if radius is None and start_radius is not None and not (float(start_radius) > 0.0 and np.isfinite(float(start_radius))):
        raise ValueError(f'knn: start_radius must be positive and finite, got {start_radius!r}')
    return KnnResult(*device_knn(pts, k, radius, q, False, start_radius, None, info)[:3])
