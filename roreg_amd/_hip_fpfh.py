"""ctypes bindings of the FPFH kernels (csrc/fpfh.hip; include/roreg_hip.h "v6n"): part of the `roreg_amd.hip` namespace (hip.py re-exports
everything here).  No reference counterpart; tests/_fpfh_oracle.py restates the definition in numpy.  Every table is in the cloud's ORIGINAL
row order; `grid` is the cloud's hip.IcpGrid (built for any radius: one built for the FPFH radius walks the fewest cells)."""
import numpy as np
import torch

from .hip import HipError, _check, _ptr, _stream, lib

__all__ = ['FPFH_WIDTH', 'fpfh_orient', 'fpfh_spfh', 'fpfh_features']

FPFH_WIDTH = 33                        # csrc/fpfh_math.h WIDTH: 11 bins of each of the three pair features


def _radius(radius, what):
    r = float(radius)
    if not (r > 0.0 and np.isfinite(r)):
        raise HipError(f'{what}: radius must be positive and finite')
    return r


def _normal_table(grid, t, what):
    _ptr(t, torch.float64)
    if tuple(t.shape) != (grid.n, 4) or (grid.n and t.data_ptr() % 32):
        raise HipError(f'{what}: the normal table must be [n,4] float64, 32-byte aligned')


def fpfh_orient(grid, normals, viewpoint):
    """normals f64 [n,4] (hip.icp_normals' table) -> the same table with every valid normal pointing to the side of `viewpoint` (three
    numbers on the host): a row is negated iff n . (viewpoint - x) < 0; a zero row stays zero, column 3 is copied."""
    _normal_table(grid, normals, 'fpfh_orient')
    c = np.ascontiguousarray(np.asarray(viewpoint, np.float64).reshape(-1))
    if c.shape != (3,) or not np.isfinite(c).all():
        raise HipError('fpfh_orient: the viewpoint must be three finite numbers')
    out = torch.empty((grid.n, 4), dtype=torch.float64, device=grid.buf.device)
    if grid.n:
        _check(lib().roreg_fpfh_orient(_ptr(grid.buf), grid.n, _ptr(normals), c.ctypes.data, _ptr(out), _stream()), 'roreg_fpfh_orient')
    return out


def fpfh_spfh(grid, oriented, radius):
    """oriented f64 [n,4] (fpfh_orient) -> (counts int32 [n,33], m int32 [n]): the bins of the pair features of every neighbour within
    `radius` that has a valid normal, and the number of such pairs.  Integers: the same bytes from any grid of the cloud."""
    r = _radius(radius, 'fpfh_spfh')
    _normal_table(grid, oriented, 'fpfh_spfh')
    dev = grid.buf.device
    counts = torch.empty((grid.n, FPFH_WIDTH), dtype=torch.int32, device=dev)
    m = torch.empty(grid.n, dtype=torch.int32, device=dev)
    if grid.n:
        ws_n = lib().roreg_fpfh_spfh_workspace(grid.n)
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        _check(lib().roreg_fpfh_spfh(_ptr(grid.buf), grid.n, _ptr(oriented), r, _ptr(counts), _ptr(m), _ptr(ws), ws_n, _stream()), 'roreg_fpfh_spfh')
    return counts, m


def fpfh_features(grid, counts, m, radius):
    """counts int32 [n,33], m int32 [n] (fpfh_spfh) -> (features f32 [n,33], valid uint8 [n]): every point's own histogram plus the
    1 / d2-weighted histograms of its neighbours within `radius`, each third normalised to 100 + 100.  valid = m > 0; an invalid row is zero."""
    r = _radius(radius, 'fpfh_features')
    _ptr(counts, torch.int32); _ptr(m, torch.int32)
    if tuple(counts.shape) != (grid.n, FPFH_WIDTH) or tuple(m.shape) != (grid.n,):
        raise HipError('fpfh_features: counts must be [n,33] int32 and m [n] int32')
    dev = grid.buf.device
    out = torch.empty((grid.n, FPFH_WIDTH), dtype=torch.float32, device=dev)
    valid = torch.empty(grid.n, dtype=torch.uint8, device=dev)
    if grid.n:
        ws_n = lib().roreg_fpfh_features_workspace(grid.n)
        ws = torch.empty(ws_n, dtype=torch.uint8, device=dev)
        _check(lib().roreg_fpfh_features(_ptr(grid.buf), grid.n, _ptr(counts), _ptr(m), r, _ptr(out), _ptr(valid), _ptr(ws), ws_n, _stream()),
               'roreg_fpfh_features')
    return out, valid
