"""Density-based clustering (DBSCAN) of dense clouds on the device (csrc/cluster.hip; no reference counterpart): Open3D's
cluster_dbscan, sklearn's DBSCAN, and with min_points = 1 PCL's EuclideanClusterExtraction.

    from roreg_amd import cluster
    res = cluster.dbscan(points, eps=0.08, min_points=6)        # -> ClusterResult: res.labels, res.n_clusters, res.sizes, res.core
    main = points[cluster.largest(res).cpu().numpy()]            # the largest connected piece of a scan

Rows are neighbours iff d2 <= eps^2 (float64, coordinates rounded to float32 once, at upload).  A row is core iff its ball holds at least
min_points rows, itself included.  Clusters are the connected components of the core rows, numbered by ascending lowest core row; a non-core
row with a core neighbour belongs to the cluster of the first one in (d2, row) order; every other row is noise, label -1.  The result is a
function of the cloud alone: the same integers on every run.  roreg_amd.outliers builds its third filter (kind='cluster') on it."""
from collections import namedtuple

import torch

from . import hip
from ._hip_cluster import _dbscan_args

ClusterResult = namedtuple('ClusterResult', 'labels n_clusters sizes core')
ClusterResult.__doc__ = ('labels int32 [n] (device; -1: noise), n_clusters int, sizes int32 [n_clusters] (device; core and border rows of each cluster), '
                         'core bool [n] (device)')


def device_dbscan(pts, eps, min_points=1):
    """dbscan on a device cloud float32 [n,3] -> (labels int32 [n], core uint8 [n], n_clusters int32 [1], sizes int32 [n]) device tensors,
    nothing read back (hip.grid_dbscan on a grid built for eps)."""
    eps, min_points = _dbscan_args(eps, min_points, 'dbscan')
    return hip.grid_dbscan(hip.IcpGrid(pts, eps), eps, min_points)


def dbscan(points, eps, min_points=1, voxel=None, device='cuda'):
    """A cloud [n,3] (host array or tensor) -> ClusterResult.  voxel=: the cloud is voxel-grid downsampled first (centroids; roreg_amd.voxel) and
    labels, core and sizes are then per voxel, in the voxels' order.  Reads n_clusters back: the call's one synchronising copy."""
    from .outliers import _upload
    _dbscan_args(eps, min_points, 'dbscan')
    pts = _upload(points, voxel, device, 'dbscan')[0]
    labels, core, nc, sizes = device_dbscan(pts, eps, min_points)
    c = int(nc.item())
    return ClusterResult(labels, c, sizes[:c], core.bool())


def largest(result):
    """The boolean mask [n] (device) of the largest cluster of a ClusterResult, ties to the lower label; all False where there is no cluster."""
    if result.n_clusters == 0:
        return torch.zeros_like(result.labels, dtype=torch.bool)
    return result.labels == torch.argmax((result.sizes.long() << 32) - torch.arange(result.n_clusters, device=result.sizes.device))
