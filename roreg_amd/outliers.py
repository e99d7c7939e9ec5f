"""Outlier removal of dense clouds on the device (csrc/grid_knn.hip through roreg_amd/neighbors.py, csrc/cluster.hip through roreg_amd/cluster.py;
DESIGN.md sections 4.26 and 4.28; no reference counterpart): the step between voxel downsampling and normal estimation, as Open3D's
remove_statistical_outlier / remove_radius_outlier and PCL's StatisticalOutlierRemoval / RadiusOutlierRemoval define it, and a third filter by
DBSCAN cluster (Open3D's cluster_dbscan, PCL's EuclideanClusterExtraction) for what the first two cannot remove.

    from roreg_amd import outliers
    res = outliers.statistical(points, nb_neighbors=20, std_ratio=2.0)     # -> OutlierResult: res.points, res.rows, res.mask, res.score
    res = outliers.radius(points, radius=0.1, min_neighbors=8)
    res = outliers.cluster(points, eps=0.08, min_size=100, min_points=6)  # or largest=True: only the largest cluster
    icp.refine(p0, p1, T0, max_dist=0.07, voxel=0.025, outliers=dict(kind='statistical', nb_neighbors=16, std_ratio=1.0))

statistical: score_i = the mean distance to the exact min(nb_neighbors, n - 1) nearest other rows; keep iff score_i <= mean(score) + std_ratio *
std(score), the SAMPLE standard deviation (n - 1), both float64 on the device.  radius: keep iff at least min_neighbors other rows lie within
`radius`.  Both judge a row by its own neighbourhood, so a dense floating fragment (mixed pixels off a depth edge, a person who walked through
one scan) passes them whole.  cluster: DBSCAN at (eps, min_points) (roreg_amd.cluster); keep iff the row's label is >= 0 and its cluster has at
least min_size rows, or with largest=True iff it is in the largest cluster (ties to the lower label); score_i = the size of row i's cluster, 0
for noise.  icp.refine, icp.estimate_normals, fpfh.describe / register / register_scene, RegistrationEngine.attach_points and run_scene take
outliers=dict(kind='statistical' | 'radius' | 'cluster', ...) and filter after voxel=, before grids and normals."""
from collections import namedtuple

import numpy as np
import torch

from . import cluster as clustering
from . import hip
from . import neighbors

OutlierResult = namedtuple('OutlierResult', 'points rows mask score')
OutlierResult.__doc__ = ('device tensors: points float32 [m,3] the kept points, rows int64 [m] their rows in the cloud given, mask bool [n] (True: kept), '
                         'score float64 [n]: statistical = the mean distance to the nearest neighbours, radius = the number of rows in the ball, '
                         'cluster = the size of the row\'s cluster (0: noise)')
KINDS = ('statistical', 'radius', 'cluster')


def _number(v, what, name, integer=False, positive=True):
    ok = not isinstance(v, (bool, str, bytes)) and isinstance(v, (int, np.integer) if integer else (int, float, np.integer, np.floating))
    if not ok or not np.isfinite(float(v)) or (positive and not float(v) > 0.0) or float(v) < 0.0:
        raise ValueError(f"{what}: {name} must be a {'positive' if positive else 'non-negative'} finite {'integer' if integer else 'number'}, got {v!r}")
    return int(v) if integer else float(v)


def check_args(spec, what='outliers'):
    """outliers= of the layers -> None, or the normalised dict(kind=..., <every argument of that kind>); ValueError otherwise (no device call)."""
    if spec is None:
        return None
    if not isinstance(spec, dict) or spec.get('kind') not in KINDS:
        raise ValueError(f"{what}: outliers must be None or a dict with kind one of {KINDS}, got {spec!r}")
    kw = {k: v for k, v in spec.items() if k != 'kind'}
    if spec['kind'] == 'statistical':
        extra = set(kw) - {'nb_neighbors', 'std_ratio'}
        nb = _number(kw.get('nb_neighbors', 20), what, 'nb_neighbors', integer=True)
        if nb > hip.GRID_KNN_MAX_K:
            raise ValueError(f'{what}: nb_neighbors is limited to {hip.GRID_KNN_MAX_K} by the kernel (the list a lane keeps, csrc/grid_knn.hip), got {nb}')
        out = dict(kind='statistical', nb_neighbors=nb, std_ratio=_number(kw.get('std_ratio', 2.0), what, 'std_ratio', positive=False))
    elif spec['kind'] == 'cluster':
        extra = set(kw) - {'eps', 'min_points', 'min_size', 'largest'}
        if 'eps' not in kw:
            raise ValueError(f"{what}: kind 'cluster' needs eps")
        big = kw.get('largest', False)
        if not isinstance(big, (bool, np.bool_)):
            raise ValueError(f'{what}: largest must be True or False, got {big!r}')
        if (kw.get('min_size') is None) != bool(big):
            raise ValueError(f"{what}: kind 'cluster' takes exactly one of min_size and largest=True")
        out = dict(kind='cluster', eps=_number(kw['eps'], what, 'eps'), min_points=_number(kw.get('min_points', 1), what, 'min_points', integer=True),
                   min_size=None if big else _number(kw['min_size'], what, 'min_size', integer=True), largest=bool(big))
    else:
        extra = set(kw) - {'radius', 'min_neighbors'}
        if 'radius' not in kw or 'min_neighbors' not in kw:
            raise ValueError(f"{what}: kind 'radius' needs radius and min_neighbors")
        out = dict(kind='radius', radius=_number(kw['radius'], what, 'radius'), min_neighbors=_number(kw['min_neighbors'], what, 'min_neighbors', integer=True))
    if extra:
        raise ValueError(f"{what}: kind {spec['kind']!r} takes no {sorted(extra)}")
    return out


def describe(spec):
    """The one line that names a filter (run_distributed's results.log)."""
    s = check_args(spec)
    if s['kind'] == 'statistical':
        return f"statistical, {s['nb_neighbors']} neighbours, std ratio {s['std_ratio']:g}"
    if s['kind'] == 'cluster':
        keep = 'the largest cluster' if s['largest'] else f"clusters of at least {s['min_size']} points"
        return f"cluster eps {s['eps']:g}, min points {s['min_points']}, {keep}"
    return f"radius {s['radius']:g}, at least {s['min_neighbors']} neighbours"


def statistical_threshold(score, std_ratio):
    """score float64 [n] (device), n >= 2 -> T = mean + std_ratio * sample standard deviation, a float64 device scalar."""
    return score.mean() + float(std_ratio) * score.std(unbiased=True)


def _result(pts, mask, score):
    rows = mask.nonzero().reshape(-1)
    return OutlierResult(pts.index_select(0, rows).contiguous(), rows, mask, score)


def device_statistical(pts, nb_neighbors=20, std_ratio=2.0, start_radius=None, info=None):
    """statistical on a device cloud float32 [n,3] -> OutlierResult."""
    s = check_args(dict(kind='statistical', nb_neighbors=nb_neighbors, std_ratio=std_ratio), 'statistical')
    n = int(pts.shape[0])
    if n < 2:                                                    # no neighbour to measure against: kept whole
        return _result(pts, torch.ones(n, dtype=torch.bool, device=pts.device), torch.full((n,), float('inf'), dtype=torch.float64, device=pts.device))
    score = neighbors.device_knn(pts, s['nb_neighbors'], None, None, True, start_radius, None, info)[3]
    return _result(pts, score <= statistical_threshold(score, s['std_ratio']), score)


def device_radius(pts, radius, min_neighbors):
    """radius on a device cloud float32 [n,3] -> OutlierResult (score = the count as float64)."""
    s = check_args(dict(kind='radius', radius=radius, min_neighbors=min_neighbors), 'radius')
    count = hip.grid_knn(hip.IcpGrid(pts, s['radius']), 1, s['radius'])[2]
    return _result(pts, count >= s['min_neighbors'], count.to(torch.float64))


def device_cluster(pts, eps, min_size=None, min_points=1, largest=False):
    """cluster on a device cloud float32 [n,3] -> OutlierResult (score = the size of the row's cluster as float64, 0 for noise).  Nothing is
    read back before the mask exists."""
    s = check_args(dict(kind='cluster', eps=eps, min_size=min_size, min_points=min_points, largest=largest), 'cluster')
    labels, _, nc, sizes = clustering.device_dbscan(pts, s['eps'], s['min_points'])
    n = int(pts.shape[0])
    if n == 0:
        return _result(pts, torch.zeros(0, dtype=torch.bool, device=pts.device), torch.zeros(0, dtype=torch.float64, device=pts.device))
    lab = labels.long()
    size = torch.where(lab >= 0, sizes.index_select(0, lab.clamp(min=0)), torch.zeros_like(sizes))
    if s['largest']:                                             # sizes is 0 behind the last cluster: the keys below are distinct, ties go to the lower label
        best = torch.argmax((sizes.long() << 32) - torch.arange(n, device=pts.device))
        mask = (lab == best) & (nc > 0)
    else:
        mask = (lab >= 0) & (size >= s['min_size'])
    return _result(pts, mask, size.to(torch.float64))


def device_apply(pts, spec):
    """The layers' call: a device cloud and a checked outliers= dict (or None) -> (kept points, their rows int64 or None)."""
    if spec is None:
        return pts, None
    kw = {k: v for k, v in spec.items() if k != 'kind'}
    res = {'statistical': device_statistical, 'radius': device_radius, 'cluster': device_cluster}[spec['kind']](pts, **kw)
    return res.points, res.rows


def _upload(points, voxel, device, what):
    from . import voxel as voxel_grid
    from .icp import device_points
    if voxel is not None:
        voxel_grid.check_args(voxel, what=what)
    pts, first = device_points(points, device), None
    if voxel is not None:
        pts, vd = voxel_grid.device_downsample(pts, voxel)
        first = vd.first.long()
    return pts, first


def _original(res, first):
    return res if first is None else res._replace(rows=first.index_select(0, res.rows))


def statistical(points, nb_neighbors=20, std_ratio=2.0, voxel=None, device='cuda'):
    """A cloud [n,3] (host array or tensor) -> OutlierResult.  voxel=: the cloud is voxel-grid downsampled first (centroids; roreg_amd.voxel);
    mask and score are then per voxel and rows the lowest original row of every kept voxel.  A cloud of fewer than 2 points is kept whole.
    nb_neighbors is limited to 32 by the kernel."""
    check_args(dict(kind='statistical', nb_neighbors=nb_neighbors, std_ratio=std_ratio), 'statistical')
    pts, first = _upload(points, voxel, device, 'statistical')
    return _original(device_statistical(pts, nb_neighbors, std_ratio), first)


def radius(points, radius, min_neighbors, voxel=None, device='cuda'):
    """A cloud [n,3] -> OutlierResult: keep iff at least min_neighbors OTHER rows lie within `radius` (d2 <= radius^2 in float64; a duplicate
    of the point counts).  Any positive min_neighbors: the kernel's count is not capped."""
    check_args(dict(kind='radius', radius=radius, min_neighbors=min_neighbors), 'radius')
    pts, first = _upload(points, voxel, device, 'radius')
    return _original(device_radius(pts, radius, min_neighbors), first)


def cluster(points, eps, min_size=None, min_points=1, largest=False, voxel=None, device='cuda'):
    """A cloud [n,3] -> OutlierResult: DBSCAN at (eps, min_points) (roreg_amd.cluster.dbscan), then keep a row iff its label is >= 0 and its
    cluster has at least min_size rows; largest=True keeps only the largest cluster instead (ties to the lower label).  Exactly one of min_size
    and largest is given.  score = the size of the row's cluster, 0 for noise."""
    check_args(dict(kind='cluster', eps=eps, min_size=min_size, min_points=min_points, largest=largest), 'cluster')
    pts, first = _upload(points, voxel, device, 'cluster')
    return _original(device_cluster(pts, eps, min_size, min_points, largest), first)
