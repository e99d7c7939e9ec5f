"""ctypes binding of the voxel-grid downsampling kernels (csrc/voxel.hip; include/roreg_hip.h "v6e"): part of the `roreg_amd.hip` namespace
(hip.py re-exports everything here).  Reference counterpart: testset.py's ME.utils.sparse_quantize(xyz / voxel_size, return_index=True)."""
from collections import namedtuple

import numpy as np
import torch

from .hip import HipError, _check, _ptr, _stream, lib

__all__ = ['VOXEL_FLAGS', 'VoxelDev', 'voxel_downsample']

VOXEL_FLAGS = ('a non-finite coordinate', 'a voxel key outside [-2^20, 2^20)', 'the hash table overflowed')
VoxelDev = namedtuple('VoxelDev', 'coords first counts inverse centroid')
VoxelDev.__doc__ = ('device tensors: coords int32 [m,3], first int32 [m] (lowest original row of each voxel, ascending), counts int32 [m], '
                    'inverse int32 [n] (voxel number of every input row), centroid float64 [m,3]')


def voxel_downsample(points, voxel):
    """points float32 [n,3] on the device, voxel > 0 -> VoxelDev narrowed to the m occupied voxels, numbered in ascending order of their
    lowest original row.  Reads (m, flags) back: the call's one synchronising copy.  A non-finite coordinate or a key out of range raises."""
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise HipError('voxel_downsample: points must be float32 [n,3]')
    voxel = float(voxel)
    if not (voxel > 0.0 and np.isfinite(voxel)):
        raise HipError('voxel_downsample: voxel must be positive and finite')
    _ptr(points, torch.float32)
    n, dev = int(points.shape[0]), points.device
    inverse = torch.empty(n, dtype=torch.int32, device=dev)
    first = torch.empty(n, dtype=torch.int32, device=dev); counts = torch.empty_like(first)
    coords = torch.empty((n, 3), dtype=torch.int32, device=dev)
    centroid = torch.empty((n, 3), dtype=torch.float64, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws_n = lib().roreg_voxel_workspace(n)
    if ws_n == 0 and n:
        raise HipError(f'voxel_downsample: {n} rows are more than the table can number (2^30)')
    ws = torch.empty(max(ws_n, 8), dtype=torch.uint8, device=dev)
    _check(lib().roreg_voxel_downsample(_ptr(points) if n else None, n, voxel, _ptr(inverse), _ptr(first), _ptr(counts), _ptr(coords), _ptr(centroid),
                                        _ptr(info), _ptr(ws), ws_n, _stream()), 'roreg_voxel_downsample')
    m, flags = (int(v) for v in info.cpu().numpy())
    if flags:
        raise HipError('voxel_downsample: the cloud has ' + ', '.join(t for b, t in enumerate(VOXEL_FLAGS) if flags >> b & 1))
    return VoxelDev(coords[:m], first[:m], counts[:m], inverse, centroid[:m])
