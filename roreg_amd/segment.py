"""RANSAC plane segmentation of dense clouds on the device (csrc/plane.hip; no reference counterpart): Open3D's
segment_plane, PCL's SACSegmentation with SACMODEL_PLANE, run for several planes in one call.  Floors, ceilings and walls of an indoor scan:
found, reported as equations, and taken away so that what stands on them falls apart into objects.

    from roreg_amd import segment, cluster
    res = segment.planes(points, dist=0.01, max_planes=6, min_inliers=2500)   # -> PlaneResult: res.labels, res.planes, res.fit, res.counts ...
    floor = segment.plane(points, dist=0.01)                                   # the one plane of greatest support
    rest = segment.off_planes(points, 0.01, max_planes=6, min_inliers=2500)    # -> outliers.OutlierResult: the rows on no plane
    objects = cluster.dbscan(rest.points, eps=0.05, min_points=4)

Round r draws n_hyp triples of the rows not yet on a plane, counts for each the rows within `dist` of the plane through it (float64, inclusive,
no square root: an exact integer) and gives the rows of the best plane (the lowest hypothesis among equal counts) label r; a best count below
min_inliers ends the segmentation.  The draws are a counter-based function of (seed, round, hypothesis), so the labels, counts, triples and raw
planes are a function of the cloud and the arguments alone: the same integers on every run.  Rows with a non-finite coordinate are on no plane."""
from collections import namedtuple

import torch

from . import hip
from . import outliers as outlier_filter

PlaneResult = namedtuple('PlaneResult', 'labels n_planes planes fit counts triples rms')
PlaneResult.__doc__ = ('labels int32 [n] (device; the plane of each row, -1: none), n_planes (int from planes(), int32 [1] device tensor from device_planes()), '
                       'planes float64 [k,4] (device): the winning triples\' planes (unit normal, offset: normal . x + offset = 0), fit float64 [k,4]: the '
                       'least-squares planes through each plane\'s rows, signed like planes, counts int32 [k], triples int32 [k,3]: the rows each plane was '
                       'drawn from, rms float64 [k]: the root-mean-square distance of a plane\'s rows to its fit; k = n_planes from planes(), max_planes from '
                       'device_planes() (rows behind n_planes are 0, triples -1)')


def check_args(dist, max_planes=1, min_inliers=3, n_hyp=1024, seed=0, what='planes'):
    """ValueError for what no cloud could make valid (no device call)."""
    return hip.plane_check_args(dist, n_hyp, max_planes, min_inliers, seed, what)


def normalised(raw):
    """raw float64 [k,4] (unnormalised normal, offset) -> the same planes with unit normals; rows of zeros stay zeros."""
    norm = raw[:, :3].square().sum(1, keepdim=True).sqrt()
    return torch.where(norm > 0, raw / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(raw))


def device_planes(pts, dist, max_planes=1, min_inliers=3, n_hyp=1024, seed=0):
    """planes on a device cloud float32 [n,3] -> PlaneResult of device tensors with max_planes rows each and n_planes int32 [1]; nothing is
    read back."""
    check_args(dist, max_planes, min_inliers, n_hyp, seed, 'device_planes')
    labels, n_planes, counts, triples, raw, fit, rms = hip.plane_segment(pts, dist, n_hyp, max_planes, min_inliers, seed)
    return PlaneResult(labels, n_planes, normalised(raw), fit, counts, triples, rms)


def _prepare(points, voxel, outliers, device, what):
    pts, first = outlier_filter._upload(points, voxel, device, what)
    return outlier_filter.device_apply(pts, outliers)[0], first


def planes(points, dist, max_planes=1, min_inliers=3, n_hyp=1024, seed=0, voxel=None, outliers=None, device='cuda'):
    """A cloud [n,3] (host array or tensor) -> PlaneResult cut to the planes found.  dist: the greatest distance of a row to its plane.
    max_planes: rounds at most.  min_inliers: a plane of fewer rows ends the segmentation.  n_hyp: triples drawn per round.  voxel= and
    outliers= apply first, as in sample.farthest; labels then index the processed cloud.  Reads the number of planes back: the call's one
    synchronising copy."""
    outliers = outlier_filter.check_args(outliers, 'planes')
    check_args(dist, max_planes, min_inliers, n_hyp, seed)
    pts = _prepare(points, voxel, outliers, device, 'planes')[0]
    res = device_planes(pts, dist, max_planes, min_inliers, n_hyp, seed)
    k = int(res.n_planes.item())
    return PlaneResult(res.labels, k, res.planes[:k], res.fit[:k], res.counts[:k], res.triples[:k], res.rms[:k])


def plane(points, dist, min_inliers=3, n_hyp=1024, seed=0, voxel=None, outliers=None, device='cuda'):
    """planes(..., max_planes=1): the plane of greatest support."""
    return planes(points, dist, 1, min_inliers, n_hyp, seed, voxel, outliers, device)


def device_split(pts, dist, max_planes=1, min_inliers=3, n_hyp=1024, seed=0, on=False):
    """off_planes (on=False) / on_planes (on=True) on a device cloud -> outliers.OutlierResult; nothing is read back before the mask exists."""
    res = device_planes(pts, dist, max_planes, min_inliers, n_hyp, seed)
    lab = res.labels.long()
    if int(pts.shape[0]) == 0 or max_planes == 0:
        score = torch.zeros(int(pts.shape[0]), dtype=torch.float64, device=pts.device)
    else:
        score = torch.where(lab >= 0, res.counts.index_select(0, lab.clamp(min=0)), torch.zeros_like(res.labels)).to(torch.float64)
    return outlier_filter._result(pts, (lab >= 0) if on else (lab < 0), score)


def off_planes(points, dist, max_planes=1, min_inliers=3, n_hyp=1024, seed=0, voxel=None, device='cuda'):
    """A cloud [n,3] -> outliers.OutlierResult (points, rows, mask, score) of the rows on NO plane of planes(points, dist, ...) (label -1; a row
    with a non-finite coordinate is on none).  score float64 [n]: the count of the row's plane, 0 off every plane.  voxel=: as in
    outliers.statistical (mask and score per voxel, rows the lowest original row of every kept voxel)."""
    check_args(dist, max_planes, min_inliers, n_hyp, seed, 'off_planes')
    pts, first = outlier_filter._upload(points, voxel, device, 'off_planes')
    return outlier_filter._original(device_split(pts, dist, max_planes, min_inliers, n_hyp, seed, on=False), first)


def on_planes(points, dist, max_planes=1, min_inliers=3, n_hyp=1024, seed=0, voxel=None, device='cuda'):
    """The complement of off_planes: the rows on some plane."""
    check_args(dist, max_planes, min_inliers, n_hyp, seed, 'on_planes')
    pts, first = outlier_filter._upload(points, voxel, device, 'on_planes')
    return outlier_filter._original(device_split(pts, dist, max_planes, min_inliers, n_hyp, seed, on=True), first)
