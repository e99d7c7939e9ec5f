"""ctypes binding of the sparse-convolution kernels (csrc/sparse_conv.hip; include/roreg_hip.h "v6j") and of the group-feature assembly behind
them (csrc/group_feature.hip, "v6l"): part of the `roreg_amd.hip` namespace (hip.py re-exports everything here).  Reference counterpart: MinkowskiEngine's coordinate manager and convolutions under backbone/fcgf."""
from collections import namedtuple

import torch

from .hip import HipError, _check, _ptr, _stream, lib

__all__ = ['SPARSE_FLAGS', 'SPARSE_ITEM_LIMIT', 'SPARSE_AXIS_LIMIT', 'StrideMap', 'sparse_stride_map', 'sparse_kernel_map', 'sparse_conv', 'sparse_l2norm',
           'group_feature_assemble', 'check_group_feature_info']

SPARSE_ITEM_LIMIT, SPARSE_AXIS_LIMIT = 1 << 15, 1 << 15
SPARSE_FLAGS = ('', 'a coordinate outside [-2^15, 2^15) or an item outside [0, 2^15)', 'the hash table overflowed')
StrideMap = namedtuple('StrideMap', 'coords parent cuts')
StrideMap.__doc__ = ('device tensors: coords int32 [m,4] at twice the tensor stride, numbered in ascending order of their lowest fine row; parent int32 [n] '
                     '(coarse row of every fine row); cuts int32 [items + 1] (segment starts of the items among the coarse rows)')


def _coords(c, what):
    if c.dtype != torch.int32 or c.dim() != 2 or c.shape[1] != 4 or c.shape[0] < 1:
        raise HipError(f'{what}: coordinates must be int32 [n,4] rows (item, x, y, z), n >= 1')
    return _ptr(c, torch.int32)


def _workspace(n, dev, what):
    ws_n = lib().roreg_sparse_map_workspace(n)
    if ws_n == 0:
        raise HipError(f'{what}: {n} rows are more than the table can number (2^30)')
    return torch.empty(ws_n, dtype=torch.uint8, device=dev), ws_n


def _refuse(flags, what):
    if flags:
        raise HipError(f'{what}: the coordinates have ' + ', '.join(t for b, t in enumerate(SPARSE_FLAGS) if flags >> b & 1))


def sparse_stride_map(coords, cuts, ts):
    """coords int32 [n,4] at tensor stride ts, cuts int32 [items + 1] on the device -> StrideMap at 2 ts.  Reads (m, flags) back: the call's one
    synchronising copy.  A coordinate or an item outside the key's range raises HipError (nothing aliases)."""
    _coords(coords, 'sparse_stride_map')
    if cuts.dtype != torch.int32 or cuts.dim() != 1 or cuts.shape[0] < 2:
        raise HipError('sparse_stride_map: cuts must be int32 [items + 1]')
    n, items, dev = int(coords.shape[0]), int(cuts.shape[0]) - 1, coords.device
    coarse = torch.empty((n, 4), dtype=torch.int32, device=dev)
    parent = torch.empty(n, dtype=torch.int32, device=dev)
    ccuts = torch.empty(items + 1, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws, ws_n = _workspace(n, dev, 'sparse_stride_map')
    _check(lib().roreg_sparse_stride_map(_ptr(coords), n, int(ts), _ptr(cuts), items, _ptr(coarse), _ptr(parent), _ptr(ccuts), _ptr(info), _ptr(ws), ws_n,
                                         _stream()), 'roreg_sparse_stride_map')
    m, flags = (int(v) for v in info.cpu().numpy())
    _refuse(flags, 'sparse_stride_map')
    return StrideMap(coarse[:m], parent, ccuts)


def sparse_kernel_map(coords_in, coords_out, k, step):
    """-> int32 [n_out, k^3]: the row of coords_in at coords_out[u] + offset(kappa) * step, or -1.  step = ts for a stride-1 or stride-2
    convolution (offsets in units of the input's tensor stride), -ts_fine for the transposed one (in = coarse, out = fine)."""
    _coords(coords_in, 'sparse_kernel_map'); _coords(coords_out, 'sparse_kernel_map')
    k, step = int(k), int(step)
    if k not in (1, 3, 5, 7) or step == 0:
        raise HipError(f'sparse_kernel_map: kernel size {k} (odd, 1..7) / step {step}')
    n_in, n_out, dev = int(coords_in.shape[0]), int(coords_out.shape[0]), coords_in.device
    M = torch.empty((n_out, k ** 3), dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    ws, ws_n = _workspace(n_in, dev, 'sparse_kernel_map')
    _check(lib().roreg_sparse_kernel_map(_ptr(coords_in), n_in, _ptr(coords_out), n_out, k, step, _ptr(M), _ptr(info), _ptr(ws), ws_n, _stream()),
           'roreg_sparse_kernel_map')
    _refuse(int(info[1].item()), 'sparse_kernel_map')
    return M


def _window(t, width, what):
    """A [rows, width] view of a contiguous 2-D float32 buffer (a column window) -> (address, row stride)."""
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_cuda or t.shape[1] != width or t.stride(1) != 1 or t.stride(0) < width:
        raise HipError(f'sparse_conv: {what} must be a float32 [rows, {width}] device tensor or a column window of one')
    return t.data_ptr(), int(t.stride(0))


def sparse_conv(x, W, M, scale=None, shift=None, residual=None, relu=False, out=None):
    """y = sum_kappa x[M[:, kappa]] @ W[kappa] in float32 fmaf chains, then relu?(y * scale + shift + residual).  x [n_in, Cin], residual and out
    [n_out, Cout] may be column windows (`buf[:, a:b]`) of wider buffers; W [K, Cin, Cout] or [Cin, Cout]; M int32 [n_out, K]."""
    if W.dim() == 2:
        W = W[None]
    K, Cin, Cout = (int(v) for v in W.shape)
    if M.dtype != torch.int32 or M.dim() != 2 or M.shape[1] != K:
        raise HipError(f'sparse_conv: the map must be int32 [n_out, {K}]')
    n_out, n_in = int(M.shape[0]), int(x.shape[0])
    xp, ldx = _window(x, Cin, 'x')
    if out is None:
        out = torch.empty((n_out, Cout), dtype=torch.float32, device=x.device)
    if out.shape[0] != n_out or (residual is not None and residual.shape[0] != n_out):
        raise HipError('sparse_conv: out and residual have one row per row of the map')
    op, ldo = _window(out, Cout, 'out')
    rp, ldr = _window(residual, Cout, 'residual') if residual is not None else (None, 0)
    for v in (scale, shift):
        if v is not None and (v.dtype != torch.float32 or v.numel() != Cout):
            raise HipError(f'sparse_conv: scale and shift must be float32 [{Cout}]')
    if scale is not None and shift is None:
        raise HipError('sparse_conv: scale comes with a shift')
    _check(lib().roreg_sparse_conv(xp, ldx, Cin, n_in, _ptr(M), n_out, K, _ptr(W, torch.float32), Cout, _ptr(scale), _ptr(shift), rp, ldr, int(bool(relu)),
                                   op, ldo, _stream()), 'roreg_sparse_conv')
    return out


def sparse_l2norm(x):
    """x float32 [n, C] -> x / |x| per row (no epsilon, as the reference's normalize_feature)."""
    if x.dtype != torch.float32 or x.dim() != 2:
        raise HipError('sparse_l2norm: x must be float32 [n, C]')
    out = torch.empty_like(x)
    _check(lib().roreg_sparse_l2norm(_ptr(x), int(x.shape[0]), int(x.shape[1]), _ptr(out), _stream()), 'roreg_sparse_l2norm')
    return out


def group_feature_assemble(feats, cuts, nn, g0, out, info=None):
    """out[n, f, g0 + r] = feats[cuts[r] + nn[r, n], f] in one launch; every other column of `out` is left alone.  feats float32 [M,F]; cuts int32
    [R + 1] (device: the items' segments among feats' rows); nn int64 [R,N] (item-local rows, hip.nn_search's output stacked); out [N,F,60] float32
    or bfloat16 (round to nearest even: the bits of `.to(torch.bfloat16)`).
    info None: the call reads the kernel's flag back (its one synchronising copy) and raises HipError if an nn entry lies outside its item; such a
    row is never read.  info = an int32 [1] device tensor the caller zeroed: the flag accumulates there across calls and the caller checks it
    (check_group_feature_info) before it uses `out`."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (feats, cuts, nn, out)):
        raise HipError('group_feature_assemble: feats, cuts, nn and out are device tensors')
    if feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[0] < 1 or not 1 <= feats.shape[1] <= 32:
        raise HipError('group_feature_assemble: feats must be float32 [M,F], M >= 1, 1 <= F <= 32')
    M, F = (int(v) for v in feats.shape)
    if nn.dtype != torch.int64 or nn.dim() != 2 or nn.shape[0] < 1 or nn.shape[1] < 1:
        raise HipError('group_feature_assemble: nn must be int64 [R,N], R >= 1, N >= 1')
    R, N = (int(v) for v in nn.shape)
    g0 = int(g0)
    if g0 < 0 or g0 + R > 60:
        raise HipError(f'group_feature_assemble: columns {g0} .. {g0 + R - 1} are not among the 60 of the group')
    if cuts.dtype != torch.int32 or cuts.dim() != 1 or cuts.shape[0] != R + 1:
        raise HipError(f'group_feature_assemble: cuts must be int32 [{R + 1}] (one segment per row of nn)')
    if out.dtype not in (torch.float32, torch.bfloat16) or tuple(out.shape) != (N, F, 60):
        raise HipError(f'group_feature_assemble: out must be float32 or bfloat16 [{N},{F},60], got {out.dtype} {tuple(out.shape)}')
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int32, device=feats.device)
    elif info.dtype != torch.int32 or info.numel() != 1 or not info.is_cuda:
        raise HipError('group_feature_assemble: info must be an int32 [1] device tensor')
    _check(lib().roreg_group_feature_assemble(_ptr(feats), M, F, _ptr(cuts), _ptr(nn), R, N, g0, _ptr(out), int(out.dtype == torch.bfloat16), _ptr(info),
                                              _stream()), 'roreg_group_feature_assemble')
    if own:
        check_group_feature_info(info)
    return out


def check_group_feature_info(info):
    """Reads group_feature_assemble's flag back (a synchronising copy) and refuses the assembled feature if it is set."""
    if int(info.item()):
        raise HipError('group_feature_assemble: an nn entry names a row outside its item (nothing was read there; the feature is not usable)')
