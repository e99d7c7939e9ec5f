"""Voxel-grid downsampling of a dense cloud on the device (csrc/voxel.hip): the step in front of a dense ICP refinement, and the reference's
own first upstream step (testset.py: ME.utils.sparse_quantize(xyz / voxel_size, return_index=True), np.floor(xyz / voxel_size)).

    from roreg_amd import voxel
    vc = voxel.downsample(points, 0.025)                 # -> VoxelCloud, centroid of every occupied voxel
    vc = voxel.downsample(points, 0.025, mode='first')   # the lowest original row of every voxel: vc.points == points[vc.first]

Coordinates are rounded to float32 once, at upload; a voxel's key is floor((double)x / voxel) per axis; voxels are numbered in ascending
order of their lowest original row, so nothing depends on how the device scheduled the work.  icp.refine, icp.estimate_normals and
RegistrationEngine.attach_points take voxel= and downsample where they upload."""
from collections import namedtuple

import numpy as np

from . import hip

VoxelCloud = namedtuple('VoxelCloud', 'points coords first counts inverse centroid')
VoxelCloud.__doc__ = ('host arrays: points float32 [m,3] (the centroid rounded once to float32, or points[first]), coords int32 [m,3], first int32 [m] '
                      '(lowest original row of each voxel, ascending), counts int32 [m], inverse int32 [n], centroid float64 [m,3]')
MODES = ('centroid', 'first')


def check_args(voxel, mode='centroid', what='downsample'):
    """-> voxel as a float; ValueError for a voxel that is not positive and finite or a mode that is not one of MODES (no device call)."""
    try:
        v = float(voxel)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: voxel must be a positive finite number, got {voxel!r}') from None
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError(f'{what}: voxel must be positive and finite, got {voxel!r}')
    if mode not in MODES:
        raise ValueError(f'{what}: mode must be one of {MODES}, got {mode!r}')
    return v


def device_downsample(points_dev, voxel, mode='centroid'):
    """points float32 [n,3] on the device -> (downsampled cloud float32 [m,3] on the device, hip.VoxelDev): what the consumers call where
    they upload a cloud."""
    import torch
    v = check_args(voxel, mode)
    vd = hip.voxel_downsample(points_dev, v)
    if mode == 'first':
        pts = points_dev.index_select(0, vd.first.long())
    else:
        pts = vd.centroid.to(torch.float32)              # one IEEE rounding of the float64 centroid
    return pts.contiguous(), vd


def downsample(points, voxel, mode='centroid', device='cuda'):
    """Host array or tensor [n,3] -> VoxelCloud on the host."""
    check_args(voxel, mode)
    from .icp import device_points
    pts, vd = device_downsample(device_points(points, device), voxel, mode)
    return VoxelCloud(*(t.cpu().numpy() for t in (pts, vd.coords, vd.first, vd.counts, vd.inverse, vd.centroid)))
