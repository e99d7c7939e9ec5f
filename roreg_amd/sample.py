"""Farthest-point sampling of dense clouds on the device (csrc/sample.hip; no reference counterpart): Open3D's
farthest_point_down_sample, the sampler of PointNet++ and Predator.  k rows that cover the cloud evenly: keypoints for the matchers.

    from roreg_amd import sample
    res = sample.farthest(points, 5000)                          # -> FarthestResult: res.rows, res.dist2, res.points
    res = sample.farthest(points, None, min_dist=0.1)            # until every point is within 0.1 of a sampled one
    many = sample.farthest_many([pts_a, pts_b, pts_c], 5000)     # all clouds in one launch, one workgroup each
    r = sample.coverage_radius(res)                              # every point of the cloud is within r of a sampled one

Row `start` first, then again and again the row farthest from the rows taken so far (float64 squared distances of the float32 coordinates,
among equal distances the lowest row); rows with a non-finite coordinate are never taken.  The first k' rows of a k-sample are the
k'-sample, and dist2 does not increase along it.  The result is a function of the cloud alone: the same integers on every run and in
whatever batch the cloud is sampled.  fpfh.register / register_scene (keypoints=) and register.Registrar (keypoint_method='farthest') build
on it."""
from collections import namedtuple
import math

import numpy as np
import torch

from . import hip
from . import outliers as outlier_filter

FarthestResult = namedtuple('FarthestResult', 'rows dist2 points')
FarthestResult.__doc__ = ('device tensors: rows int64 [m] in selection order (m <= k: the cloud may hold fewer live rows, min_dist may end the selection), '
                          'dist2 float64 [m]: the squared distance of each row to the rows before it when it was selected (dist2[0] = inf), '
                          'points float32 [n,3]: the cloud the rows index (after voxel= and outliers=)')


def check_args(k, start=0, min_dist=None, what='farthest'):
    """ValueError for what no cloud could make valid (no device call): k, start, min_dist."""
    if k is None and min_dist is None:
        raise ValueError(f'{what}: k=None needs min_dist (sample until the cloud is covered at that distance)')
    if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < 2 ** 31):
        raise ValueError(f'{what}: k must be None or an integer >= 0, got {k!r}')
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or int(start) < 0:
        raise ValueError(f'{what}: start must be a row of the cloud, got {start!r}')
    if min_dist is not None:
        ok = not isinstance(min_dist, (bool, str, bytes)) and isinstance(min_dist, (int, float, np.integer, np.floating))
        if not ok or not (float(min_dist) >= 0.0 and np.isfinite(float(min_dist))):
            raise ValueError(f'{what}: min_dist must be None or a finite number >= 0, got {min_dist!r}')


def _k_of(pts, k):
    return int(pts.shape[0]) if k is None else k


def device_farthest(pts, k, start=0, min_dist=None):
    """farthest on a device cloud float32 [n,3] -> (rows int32 [k], dist2 float64 [k], count int32 [1]) device tensors, nothing read back
    (hip.fps: rows are -1 and dist2 0 behind count).  pts a list of clouds: all of them in one launch -> a list of such triples."""
    check_args(k, start, min_dist, 'device_farthest')
    if isinstance(pts, (list, tuple)):
        return hip.fps_batch([(p, _k_of(p, k), start, min_dist) for p in pts])
    return hip.fps(pts, _k_of(pts, k), start, min_dist)


def _prepare(points, voxel, outliers, device, what):
    pts = outlier_filter._upload(points, voxel, device, what)[0]
    return outlier_filter.device_apply(pts, outliers)[0]


def farthest_many(clouds, k, start=0, min_dist=None, voxel=None, outliers=None, device='cuda'):
    """farthest of every cloud of a list, all in one launch (one workgroup per cloud: the clouds share the device) -> [FarthestResult].
    One read-back for the call: the counts."""
    outliers = outlier_filter.check_args(outliers, 'farthest')
    check_args(k, start, min_dist)
    pts = [_prepare(c, voxel, outliers, device, 'farthest') for c in clouds]
    if not pts:
        return []
    res = device_farthest(pts, k, start, min_dist)
    counts = torch.cat([r[2] for r in res]).cpu().tolist()
    return [FarthestResult(r[0][:c].long(), r[1][:c], p) for r, c, p in zip(res, counts, pts)]


def farthest(points, k, start=0, min_dist=None, voxel=None, outliers=None, device='cuda'):
    """A cloud [n,3] (host array or tensor) -> FarthestResult.  k: the number of rows (fewer come back when the cloud has fewer live rows or
    min_dist ends the selection); k=None with min_dist=r: as many as it takes until every point is within r of a sampled one.  start: the
    first row.  min_dist: rows closer than that to the sampled ones are not taken (a row at exactly min_dist is).  voxel= and outliers= apply
    first, as in outliers.statistical; rows then index the processed cloud, which the result's `points` returns.  Reads the count back: the
    call's one synchronising copy."""
    return farthest_many([points], k, start, min_dist, voxel, outliers, device)[0]


def coverage_radius(result):
    """The distance within which every live point of the cloud lies of some sampled row BEFORE the last one was added: sqrt(dist2[-1]), a
    float (inf for a sample of one row).  The sampled rows are at least that far from each other."""
    if int(result.dist2.shape[0]) == 0:
        raise ValueError('coverage_radius: the sample is empty')
    return math.sqrt(float(result.dist2[-1]))
