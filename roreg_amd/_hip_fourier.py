"""ctypes bindings of the group-Fourier (irrep-domain) path of the group convolutions and of the split-operand dense / conv layers
(csrc/fourier.hip, group_conv.hip): part of the `roreg_amd.hip` namespace (hip.py re-exports everything here).  Module state that callers
set on `hip` (hip.PROFILE) is read through the module, never copied."""
import os
from ctypes import c_void_p

import numpy as np
import torch

from . import hip as _core
from .hip import HipError, _check, _feat, _ptr, _stream, lib

__all__ = ['DenseSplitLayer', 'IRREP_DIMS', 'IRREP_OFFSETS', '_bf16_split3', '_keypoint_of_columns', '_ptr_array', '_res_ptr', '_tile_cache', 'bf16_split3_frags', 'bf16_split3_pack', 'bound_exp', 'coef_pitch', 'coef_size', 'coef_views', 'dense_split', 'ensure_fourier', 'f16_scale_exp', 'f16_split2_frags', 'f16_split2_pack', 'frag_pack', 'ft_nonlin', 'ft_nonlin_gathered', 'ft_nonlin_packed', 'gemm_persistent', 'gemm_thin', 'gf_finish', 'gf_finish_rows', 'gf_finish_usable', 'group_conv_split_pack', 'irrep_gemm', 'irrep_gemm_rows', 'next_bound', 'next_bound_spatial', 'pack_coefs_f16x2', 'row_bound', 'unpack_coefs_f16x2', 'words_to_planes']


_fourier_ready = False
IRREP_DIMS = (1, 3, 3, 4, 5)
IRREP_OFFSETS = (0, 1, 10, 19, 35, 60)


def ensure_fourier():
    global _fourier_ready
    if not _fourier_ready:
        from .fourier import group_fourier
        F = np.ascontiguousarray(group_fourier().F, np.float32)
        _check(lib().roreg_set_fourier_tables(F.ctypes.data), 'roreg_set_fourier_tables')
        _fourier_ready = True


def _ptr_array(views):
    arr = (c_void_p * 5)(*[c_void_p(v.data_ptr()) for v in views])
    return arr


def coef_pitch(B):
    """Keypoint pitch of the coefficient buffers: B rounded up to the 32-keypoint tile of ft_nonlin (pad keypoints hold zeros)."""
    return (int(B) + 31) // 32 * 32


def coef_size(C, B):
    return 60 * C * coef_pitch(B)


def coef_views(buf, C, B):
    """Five per-irrep GEMM operands [d*C, d*Bp] of a flat coefficient buffer of 60*C*Bp floats (Bp = coef_pitch(B))."""
    Bp = coef_pitch(B)
    return [buf[IRREP_OFFSETS[r] * C * Bp:IRREP_OFFSETS[r + 1] * C * Bp].view(IRREP_DIMS[r] * C, IRREP_DIMS[r] * Bp) for r in range(5)]


_tile_cache = {}


def _x_planes_kernel(x_planes):
    """irrep_gemm's x_planes -> the library's: False / 0 the word layout; the integers 1 / 2 name the 32x32x16 / 16x16x32 LDS-DMA kernel; True (or
    anything else that is set) the one hip.MFMA16 selects."""
    if not x_planes:
        return 0
    if x_planes is not True and x_planes in (1, 2):
        return int(x_planes)
    return 2 if _core.MFMA16 else 1


def irrep_gemm(X_buf, Wpacks, C, O, B, split=None, add=None, f16x2=None, x_bound=None, next_bound=None, x_planes=False):
    """coefficients [60*C*Bp] -> [60*O*Bp] through the five per-irrep GEMMs (Bp = coef_pitch(B): the GEMMs run on the padded width).
    split: the five 3xbf16-split weight tensors (f32-accurate GEMM on the bf16 matrix cores) or None for the f32-input MFMA kernel.
    add: optional coefficient buffer [60*O*Bp] summed onto the result in the epilogue (residual short cut in the irrep domain).
    f16x2 = (five fp16x2 weight tensors, w_exp): X_buf holds the fp16 hi/lo words ft_nonlin(split='f16x2', out_bound=x_bound) wrote under the
    per-keypoint bound x_bound [Bp]; next_bound = (u [O], v [O]) (NextBound of the following nonlinearity) additionally returns the
    per-keypoint bound [Bp] of the NEXT transform's coefficients: -> (out, bound).
    x_planes: X_buf is in the half-block layout (ft_nonlin(..., planes=True): per 32-column block 32 fp16 hi values, then 32 lo values, columns in the order 0, 16, 1, 17, ...): the activations reach LDS by LDS-DMA; O % 256 == 0 only.  True: the kernel hip.MFMA16 selects
    (default: 16x16x32 MFMAs); the integers 1 / 2 name the 32x32x16 / 16x16x32 kernel (tests)."""
    Bp = coef_pitch(B)
    if X_buf.numel() != 60 * C * Bp or (add is not None and add.numel() != 60 * O * Bp):
        raise HipError(f'irrep_gemm: coefficient buffers must hold 60*C*{Bp} floats (B={B} padded to the 32-keypoint pitch)')
    out = torch.empty(60 * O * Bp, dtype=torch.float32, device=X_buf.device)
    tile_m = 256 if (f16x2 is not None and O % 256 == 0 and not os.environ.get('ROREG_TILE_M128')) else 128          # 256-row tiles = 8-wave workgroups (fp16 x 2 kernel)
    key = (O, Bp, tile_m)
    t = _tile_cache.get(key)
    if t is None:
        n = lib().roreg_irrep_gemm_tiles_m(O, Bp, tile_m, None)
        host = np.empty((n, 3), np.int32)
        lib().roreg_irrep_gemm_tiles_m(O, Bp, tile_m, host.ctypes.data)
        t = torch.from_numpy(host).cuda()
        _tile_cache[key] = t
    xv = coef_views(X_buf, C, B); ov = coef_views(out, O, B)
    av = _ptr_array(coef_views(add, O, B)) if add is not None else None
    if _core.PROFILE is not None:
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e0.record()
    bound_out = None
    if f16x2 is not None:
        wl, w_exp = f16x2
        if x_bound is None or x_bound.numel() != Bp:
            raise HipError(f'irrep_gemm: the fp16 x 2 GEMM needs x_bound with one value per (padded) keypoint ({Bp})')
        nu = nv = None
        if next_bound is not None:
            nu, nv = next_bound
            if nu.numel() != O or nv.numel() != O:
                raise HipError('irrep_gemm: next_bound must hold one (u, v) per output channel')
            bound_out = torch.zeros(Bp, dtype=torch.float32, device=X_buf.device)
        _check(lib().roreg_irrep_gemm_f16x2(_ptr_array(xv), _ptr_array(ov), av, _ptr_array(wl), _ptr(x_bound, torch.float32), int(w_exp),
                                            _ptr(nu, torch.float32), _ptr(nv, torch.float32), _ptr(bound_out), C, O, Bp,
                                            _ptr(t, torch.int32), int(t.shape[0]), tile_m, _x_planes_kernel(x_planes), _stream()), 'roreg_irrep_gemm_f16x2')
    elif split is not None:
        _check(lib().roreg_irrep_gemm_split(_ptr_array(xv), _ptr_array(ov), av, _ptr_array(split), C, O, Bp, _ptr(t, torch.int32), int(t.shape[0]),
                                            _stream()), 'roreg_irrep_gemm_split')
    else:
        _check(lib().roreg_irrep_gemm(_ptr_array(xv), _ptr_array(ov), av, _ptr_array(Wpacks), C, O, Bp, _ptr(t, torch.int32), int(t.shape[0]), _stream()),
               'roreg_irrep_gemm')
    if _core.PROFILE is not None:
        e1.record(); _core.PROFILE.append((('irrep_gemm_f16x2' if f16x2 is not None else 'irrep_gemm_split' if split is not None else 'irrep_gemm', Bp, C, O), e0, e1))
    return (out, bound_out) if next_bound is not None else out


class _GemmSwitch:
    """A run-time switch of the GEMM launch (an entry point of the library that sets a value and returns the previous one): calling it gives the
    context manager that sets the switch on entry and puts the previous setting back on exit."""

    def __init__(self, entry, coerce, doc, on=None):
        self.entry, self.coerce, self.__doc__, self.on = entry, coerce, doc, on

    def __call__(self, on=True):
        return _GemmSwitch(self.entry, self.coerce, self.__doc__, self.coerce(on))

    def __enter__(self):
        self.prev = getattr(lib(), self.entry)(self.on)

    def __exit__(self, *exc):
        getattr(lib(), self.entry)(self.prev)
        return False


gemm_persistent = _GemmSwitch('roreg_gemm_persistent', int,      # 0 / False: one workgroup per tile; 1 / True: persistent; 2: half tiles, two workgroups per CU
                              """`with hip.gemm_persistent(True | False):` -- how the 16x16x32 LDS-DMA GEMM is launched inside the block (roreg_gemm_persistent): persistent
    workgroups that claim tiles, or one workgroup per tile.  Same bits either way -- tests and A/B measurements.""")
gemm_thin = _GemmSwitch('roreg_gemm_thin', lambda on: int(bool(on)),
                        """`with hip.gemm_thin(True | False):` -- whether the thin layers (C == 32 or O == 32, fp16 x 2, word layout, no residual) run on their own
    kernels inside the block (roreg_gemm_thin; the default) or on the generic one.  Same bits either way -- tests and A/B measurements.""")

gf_finish = _GemmSwitch('roreg_gf_finish_route', lambda on: int(bool(on)),
                        """`with hip.gf_finish(True | False):` -- whether the engine ends the extractor with Conv_out in per-keypoint rows + gf_finish_kernel (roreg_gf_finish_route;
    the default, ROREG_GF_FINISH=0 in the environment turns it off) or with the four kernels ft_nonlin, gf_finalize, inv_descriptor, feat_coefs.  Same bits either
    way -- tests and A/B measurements.""")


def gf_finish_usable(gemm_mode, *dtypes):
    """Whether the one-pass end of the extractor applies: the switch is on, the extractor and feat_coefs both run fp16 x 2, the thin kernels are on
    and every tensor involved is stored in float32."""
    return (gemm_mode == 'f16x2' and _core.GEMM_MODE == 'f16x2' and all(d == torch.float32 for d in dtypes)
            and lib().roreg_gemm_thin(-1) == 1 and lib().roreg_gf_finish_route(-1) == 1)


def irrep_gemm_rows(X_buf, C, B, f16x2, x_bound):
    """Conv_out's GEMM (O = 32, fp16 x 2, word-layout operand, as irrep_gemm) with the result in per-keypoint rows: float32 [Bp, 60, 32], element
    [b, q, o] = coefficient q (irrep offset + i d + l) of channel o -- the values irrep_gemm returns, bit for bit, at other addresses."""
    Bp = coef_pitch(B)
    wl, w_exp = f16x2
    if X_buf.numel() != 60 * C * Bp or x_bound is None or x_bound.numel() != Bp:
        raise HipError(f'irrep_gemm_rows: X_buf must hold 60*C*{Bp} words and x_bound {Bp} values')
    out = torch.empty((Bp, 60, 32), dtype=torch.float32, device=X_buf.device)
    _check(lib().roreg_irrep_gemm_f16x2_rows(_ptr_array(coef_views(X_buf, C, B)), _ptr(out), _ptr_array(wl), _ptr(x_bound, torch.float32), int(w_exp), C, Bp,
                                             _stream()), 'roreg_irrep_gemm_f16x2_rows')
    return out


def gf_finish_rows(T3r, x, b_out, roles=None):
    """T3r [Bp,60,32] (irrep_gemm_rows), x [B,32,60] float32, b_out [32] -> (eqv [B,32,60], inv [B,32], eqv_ft [B,32,60]), float32: normalise((IFT(T3) + b_out) + x),
    its invariant descriptor and its group-Fourier coefficients in one kernel; roles = (scale [128], shift [128], out [B,4]) of role_max: columns 2 and 3
    of `out` are written as well."""
    ensure_fourier()
    B = int(x.shape[0])
    if x.shape[1:] != (32, 60) or x.dtype != torch.float32 or not x.is_contiguous() or T3r.shape != (coef_pitch(B), 60, 32) or b_out.numel() != 32:
        raise HipError('gf_finish_rows: T3r [Bp,60,32], x [B,32,60] contiguous float32, b_out [32]')
    eqv = torch.empty((B, 32, 60), dtype=torch.float32, device=x.device)
    eft = torch.empty((B, 32, 60), dtype=torch.float32, device=x.device)
    inv = torch.empty((B, 32), dtype=torch.float32, device=x.device)
    scale = shift = role = None
    if roles is not None:
        scale, shift, role = _core._role_args(roles, B)
        scale, shift = scale[64:], shift[64:]
    _check(lib().roreg_gf_finish(_ptr(T3r, torch.float32), _ptr(x, torch.float32), _ptr(b_out, torch.float32), _ptr(scale), _ptr(shift), _ptr(eqv), _ptr(inv),
                                 _ptr(role), _ptr(eft), B, _stream()), 'roreg_gf_finish')
    return eqv, inv, eft


def row_bound(x, bn=None, roles=None):
    """x [B,C,60] group-domain tensor -> float32 [Bp]: sqrt(60) * max_{c,g} |act(x[b])| (act = ReLU(BN(.)) with bn = (scale, shift), else the
    identity), a bound on every coefficient of FT(act(x[b])); 0 for the pad keypoints.  The x_bound of a layer fed from the group domain.
    roles = (scale [128], shift [128], out [B,4]) of hip.role_max (x = a cloud's `before` features, C = 32, no bn): columns 0 and 1 of `out` are
    written by the same kernel."""
    B, C = int(x.shape[0]), int(x.shape[1])
    out = torch.empty(coef_pitch(B), dtype=torch.float32, device=x.device)
    scale, shift = bn if bn is not None else (None, None)
    xp, bf = _feat(x)
    if roles is not None:
        if bn is not None or C != 32:
            raise HipError('row_bound: roles go with the 32-channel input features and no BatchNorm')
        r_scale, r_shift, role = _core._role_args(roles, B)
        _check(lib().roreg_row_bound_roles(xp, bf, _ptr(out), _ptr(r_scale), _ptr(r_shift), _ptr(role), B, _stream()), 'roreg_row_bound_roles')
        return out
    _check(lib().roreg_row_bound(xp, bf, _ptr(scale), _ptr(shift), _ptr(out), B, C, _stream()), 'roreg_row_bound')
    return out


def _keypoint_of_columns(d, Bp):
    """keypoint index of every GEMM column of an irrep of dimension d (columns are blocked by 32 keypoints)."""
    n = torch.arange(d * Bp, device='cuda')
    return ((n // 32) // d) * 32 + (n % 32)


def bound_exp(bound):
    """e with bound * 2^e < 2^14, as the kernels derive it (tensor in, int32 tensor out)."""
    _, ex = torch.frexp(bound.float())
    e = torch.where((bound > 0) & torch.isfinite(bound), 14 - ex, torch.zeros_like(ex))
    return e.clamp(-100, 100)


def pack_coefs_f16x2(X_buf, C, B, bound=None):
    """float32 coefficient buffer -> (fp16 hi/lo words in the layout roreg_ft_nonlin(split=2) writes, per-keypoint bound [Bp]).
    Test / tooling helper (torch ops): the product path gets its split operands from ft_nonlin directly."""
    Bp = coef_pitch(B)
    views = coef_views(X_buf, C, B)
    if bound is None:
        bound = torch.zeros(Bp, dtype=torch.float32, device=X_buf.device)
        for r, v in enumerate(views):
            kp = _keypoint_of_columns(IRREP_DIMS[r], Bp)
            bound.scatter_reduce_(0, kp, v.abs().amax(0), 'amax')
    e = bound_exp(bound)
    out = torch.empty_like(X_buf)
    for r, (v, o) in enumerate(zip(views, coef_views(out, C, B))):
        kp = _keypoint_of_columns(IRREP_DIMS[r], Bp)
        y = torch.ldexp(v, e[kp][None, :])
        hi = y.half()
        lo = (y - hi.float()).half()
        w = (hi.view(torch.int16).to(torch.int32) & 0xffff) | (lo.view(torch.int16).to(torch.int32) << 16)
        o.copy_(w.view(torch.float32))
    return out, bound


def words_to_planes(X_words, C, B):
    """The fp16 hi/lo word layout -> the half-block layout of ft_nonlin(planes=True) (test helper, torch ops): every 32-column block of a row
    holds its 32 hi values (16 bit each, in the column order 0, 16, 1, 17, ...: word w pairs columns w and w + 16), then its 32 lo values in
    the same order, in the 128 bytes the 32 words occupied."""
    w = X_words.contiguous().view(torch.int32).view(-1, 2, 16)                        # [block][column // 16][column % 16]
    hi = (w & 0xffff).to(torch.int16).transpose(1, 2); lo = (w >> 16).to(torch.int16).transpose(1, 2)         # [block][w][pair member]
    return torch.cat([hi.reshape(-1, 32), lo.reshape(-1, 32)], 1).contiguous().view(torch.float32).view(-1)


def unpack_coefs_f16x2(X_words, bound, C, B):
    """Inverse of the split: fp16 hi/lo words + per-keypoint bound -> float32 coefficients (hi + lo) * 2^-e.  Test helper."""
    Bp = coef_pitch(B)
    e = bound_exp(bound)
    out = torch.empty_like(X_words)
    for r, (v, o) in enumerate(zip(coef_views(X_words, C, B), coef_views(out, C, B))):
        kp = _keypoint_of_columns(IRREP_DIMS[r], Bp)
        w = v.view(torch.int32)
        hi = (w & 0xffff).to(torch.int16).view(torch.float16).float()
        lo = (w >> 16).to(torch.int16).view(torch.float16).float()
        o.copy_(torch.ldexp(hi + lo, -e[kp][None, :]))
    return out


def next_bound_spatial(bn, bias):
    """(u, v) device float32 [O] for a GEMM epilogue whose output goes back to the GROUP domain through ReLU(scale_o (IFT(T)_o + bias_o) + shift_o)
    (roreg_ft_nonlin_packed): |IFT(T)(g)| <= sqrt(60) max_q |T_q|, so |value| <= max_{o,q} (sqrt(60) |scale_o| |T_oq| + |scale_o| |bias_o| + |shift_o|);
    the 2^-9 margin covers the float32 rounding of the transform."""
    scale, shift = bn
    sc = scale.detach().double().abs().cpu(); sh = shift.detach().double().abs().cpu()
    b = bias.detach().double().cpu()
    k = 1.0 + 2.0 ** -9
    u = (np.sqrt(60.0) * k) * sc
    v = k * (sc * b.abs() + sh) + 1e-30
    return u.float().cuda().contiguous(), v.float().cuda().contiguous()


def ft_nonlin_packed(B, C, coef_in, bias, bn, out_bound, g_map=None, Lout=60, Lvalid=60, raw_g=None):
    """IFT + bias + BatchNorm + ReLU -> (words int32 [B,C,Lout] = fp16 hi | lo << 16 under the block scale of out_bound, raw [B,C] float32 = the
    pre-activation value of group element raw_g or None): the operand of hip.group_conv_packed."""
    ensure_fourier()
    dev = coef_in.device
    if coef_in.numel() != coef_size(C, B) or out_bound.numel() != coef_pitch(B):
        raise HipError('ft_nonlin_packed: coef_in / out_bound sizes')
    words = torch.empty((B, C, Lout if g_map is not None else 60), dtype=torch.int32, device=dev)
    raw = torch.empty((B, C), dtype=torch.float32, device=dev) if raw_g is not None else None
    scale, shift = bn if bn is not None else (None, None)
    _check(lib().roreg_ft_nonlin_packed(_ptr(coef_in, torch.float32), _ptr(bias), _ptr(scale), _ptr(shift), _ptr(words), _ptr(g_map, torch.int32),
                                        int(Lout), int(Lvalid), B, C, _ptr(out_bound, torch.float32), _ptr(raw), int(raw_g or 0), _stream()),
           'roreg_ft_nonlin_packed')
    return words, raw


def next_bound(bn, bias, bias2=None):
    """(u, v) device float32 [O] of the bound a GEMM epilogue propagates to the next transform (include/roreg_hip.h, roreg_irrep_gemm_f16x2):
    the next nonlinearity is x = ReLU(scale_o (IFT(T)_o + bias_o) + shift_o); with an orthonormal 60 x 60 transform
    |FT(x)_q| <= sqrt(60) max_g |x(g)| and |IFT(T)(g)| <= sqrt(60) max_q |T_q|, so  |FT(x)| <= max_{o,q} (60 |scale_o| |T_oq| + sqrt(60) (|scale_o| |bias_o| + |shift_o|)).
    A 2^-9 margin covers the float32 rounding of the transforms themselves."""
    scale, shift = bn
    sc = scale.detach().double().abs().cpu(); sh = shift.detach().double().abs().cpu()
    b = bias.detach().double().cpu() + (bias2.detach().double().cpu() if bias2 is not None else 0.0)
    k = 1.0 + 2.0 ** -9
    u = (60.0 * k) * sc
    v = (np.sqrt(60.0) * k) * (sc * b.abs() + sh) + 1e-30
    return u.float().cuda().contiguous(), v.float().cuda().contiguous()


def ft_nonlin(B, C, coef_in=None, x_spatial=None, bias=None, bias2=None, bn=None, resid_spatial=None, spatial_out=False,
              g_map=None, Lout=60, Lvalid=60, split=False, out_bound=None, want_rowmax=False, planes=False):
    """split='f16x2' with coefficient output: out_bound [Bp] (row_bound() or the producing GEMM's propagated bound) is required and the
    result holds fp16 hi/lo words for irrep_gemm(f16x2=...) instead of floats.  want_rowmax (group-domain output): also return the
    per-keypoint max |out[b]| [B] (the block scale of the fp16 x 2 convolution that follows)."""
    ensure_fourier()
    dev = (coef_in if coef_in is not None else x_spatial).device
    if spatial_out:
        out = torch.empty((B, C, Lout if g_map is not None else 60), dtype=torch.float32, device=dev); xout = None; osp = _ptr(out)
    else:
        out = torch.empty(coef_size(C, B), dtype=torch.float32, device=dev); xout = _ptr(out); osp = None
    scale, shift = bn if bn is not None else (None, None)
    if want_rowmax and not spatial_out:
        raise HipError('ft_nonlin: want_rowmax goes with spatial_out')
    amax = torch.zeros(B, dtype=torch.float32, device=dev) if want_rowmax else None
    if coef_in is not None and coef_in.numel() != coef_size(C, B):
        raise HipError(f'ft_nonlin: coef_in must hold 60*C*{coef_pitch(B)} floats')
    if out_bound is not None and out_bound.numel() != coef_pitch(B):
        raise HipError(f'ft_nonlin: out_bound must hold one value per (padded) keypoint ({coef_pitch(B)})')
    xs, bf_x = _feat(x_spatial); rs, bf_r = _feat(resid_spatial)
    if x_spatial is not None and resid_spatial is not None and bf_x != bf_r:
        raise HipError('ft_nonlin: x_spatial and resid_spatial must share one dtype')
    _check(lib().roreg_ft_nonlin(_ptr(coef_in, torch.float32), xs, _ptr(bias),
                                 _ptr(bias2), _ptr(scale), _ptr(shift), rs, xout, osp,
                                 _ptr(g_map, torch.int32), int(Lout), int(Lvalid), B, C, 2 if split == 'f16x2' else (1 if split else 0),
                                 _ptr(out_bound, torch.float32), _ptr(amax), bf_x or bf_r, 1 if planes else 0, _stream()), 'roreg_ft_nonlin')
    return (out, amax) if want_rowmax else out


def ft_nonlin_gathered(g, bn=None, planes=False):
    """ft_nonlin(B, 128, x_spatial=x, bn=bn, split='f16x2', out_bound=g.bound, planes=planes) for the x [B,128,60] that g (hip.GatheredRows, from
    LtBatch.prepare_rows) would assemble to, read from the clouds' own tensors: the same words, no x."""
    ensure_fourier()
    _core.ensure_tables()
    B = g.shape[0]
    out = torch.empty(coef_size(128, B), dtype=torch.float32, device=g.rows.device)
    scale, shift = bn if bn is not None else (None, None)
    if g.bound.numel() != coef_pitch(B) or g.dr.numel() != B:
        raise HipError('ft_nonlin_gathered: rows / dr / bound sizes')
    _check(lib().roreg_ft_nonlin_gathered(_ptr(g.rows, torch.int64), _ptr(g.dr, torch.int64), 1 if g.bf16 else 0, _ptr(scale), _ptr(shift), _ptr(out), B,
                                          _ptr(g.bound, torch.float32), 1 if planes else 0, _stream()), 'roreg_ft_nonlin_gathered')
    return out


def _bf16_split3(x):
    """float32 array -> three uint16 arrays of bf16 bits: round-to-nearest-even pieces, each taken from the exact float32 remainder."""
    out = []
    rem = np.ascontiguousarray(x, np.float32)
    for _ in range(3):
        u = rem.view(np.uint32)
        r = ((u >> 16) & 1) + 0x7fff
        hi = ((u + r) >> 16).astype(np.uint16)
        out.append(hi)
        rem = rem - (hi.astype(np.uint32) << 16).view(np.float32)
    return out


def f16_scale_exp(absmax):
    """e with absmax * 2^e in [2^13, 2^14): the block-scaling exponent of the fp16 x 2 operand split."""
    return 14 - int(np.frexp(float(absmax))[1]) if absmax > 0 else 0


def _f16_split2(W, w_exp):
    """float32 array -> two uint16 arrays of fp16 bits: hi = fp16(w * 2^w_exp), lo = fp16(w * 2^w_exp - hi) (the remainder is exact in float32)."""
    Ws = np.ldexp(np.ascontiguousarray(W, np.float32), w_exp).astype(np.float32)
    hi = Ws.astype(np.float16)
    return [hi.view(np.uint16), (Ws - hi.astype(np.float32)).astype(np.float16).view(np.uint16)]


def frag_pack(pieces):
    """The fragment order every split kernel reads its weights in: uint16 arrays [O, K, *rest] (K % 16 == 0), one per piece -> int16 array
    [piece][*rest][K/16][2][O][8]; element [p][*r][kb][h][o][e] is piece p of W[o, 16*kb + 8*h + e, *r] (one 16-byte load per MFMA fragment)."""
    P = np.stack(pieces)
    O, K = P.shape[1:3]
    P = P.reshape(len(pieces), O, K // 16, 2, 8, *P.shape[3:])
    return np.ascontiguousarray(P.transpose(0, *range(5, P.ndim), 2, 3, 1, 4)).view(np.int16)


def f16_split2_frags(W, w_exp):
    """host stage of the fp16 x 2 packers: W float32 [O, K, *rest] -> int16 array [2][*rest][K/16][2][O][8]"""
    return frag_pack(_f16_split2(W, w_exp))


def bf16_split3_frags(W):
    """host stage of the bf16 x 3 packers: W float32 [O, K, *rest] -> int16 array [3][*rest][K/16][2][O][8]"""
    return frag_pack(_bf16_split3(W))


def f16_split2_pack(Wm, w_exp):
    """Wm float32 [Mpad, K] (K % 16 == 0) -> int16 device tensor [2][K/16][2][Mpad][8] of fp16 bits: hi = fp16(w * 2^w_exp),
    lo = fp16(w * 2^w_exp - hi), in the fragment order of irrep_gemm_split_kernel<NP=2>."""
    return torch.from_numpy(f16_split2_frags(Wm, w_exp)).cuda()


def bf16_split3_pack(Wm):
    """Wm float32 [Mpad, K] (K % 16 == 0) -> int16 device tensor [3][K/16][2][Mpad][8]: the three bf16 pieces of every weight in the
    fragment order of irrep_gemm_split_kernel."""
    return torch.from_numpy(bf16_split3_frags(Wm)).cuda()


class DenseSplitLayer:
    """out[b][o] = bias[o] + sum_k W[o][k] * act_k(x[b][k]) (+ residual) in kernel-ready form: W float32 [O,K] (K % 16 == 0) as the
    three bf16 planes [3][K/16][2][round_up(O,256)][8]; act = BatchNorm(eval)+ReLU given as per-k scale/shift, or None."""

    @staticmethod
    def pack(W):
        """host stage: (bf16 x 3 planes, fp16 x 2 planes (hi, lo) under the power-of-two scale 2^w_exp, w_exp) of W with O padded to 256 by zero rows"""
        O, K = np.shape(W)
        Wp = np.zeros(((O + 255) // 256 * 256, K), np.float32); Wp[:O] = W
        w_exp = f16_scale_exp(float(np.abs(Wp).max()))
        return bf16_split3_frags(Wp), f16_split2_frags(Wp, w_exp), w_exp

    def __init__(self, W, bias, scale=None, shift=None):
        self.O, self.K = np.shape(W)
        ws, ws2, self.w_exp = self.pack(W)
        self.ws = torch.from_numpy(ws).cuda()
        self.ws2 = torch.from_numpy(ws2).cuda()
        self.act_smax = float(np.abs(scale).max()) if scale is not None else 1.0
        self.act_tmax = float(np.abs(shift).max()) if shift is not None else 0.0
        self.bias = torch.from_numpy(np.ascontiguousarray(bias, np.float32)).cuda()
        self.scale = torch.from_numpy(np.ascontiguousarray(scale, np.float32)).cuda() if scale is not None else None
        self.shift = torch.from_numpy(np.ascontiguousarray(shift, np.float32)).cuda() if shift is not None else None


def _res_ptr(t):
    """data pointer of a residual operand that may be a strided VIEW (its first element is what the kernel indexes from)"""
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda:
        raise HipError('dense_split: residual must be a float32 device tensor')
    return c_void_p(t.data_ptr())


def dense_split(x, layer, residual=None, in_rowmax=None, want_rowmax=False, residual_stride=1):
    """x [B, K] float32 (device, contiguous) -> [B, O].  residual: element (b, o) at residual.flat[(b*O + o) * residual_stride] (pass a
    [B, O, L] tensor's column c as residual=t[:, :, c:] -- a view, no copy -- with residual_stride=L).  in_rowmax (device float32 [B], the tracked max |x[b]| per row): use the fp16 x 2
    kernel (per-row block scale); want_rowmax: also return the tracked per-row max |out[b]| (device float32 [B]) for the next layer."""
    B, K = x.shape
    if K != layer.K:
        raise HipError(f'dense_split: K mismatch ({K} vs {layer.K})')
    out = torch.empty((B, layer.O), dtype=torch.float32, device=x.device)
    if in_rowmax is not None:
        if in_rowmax.numel() != B:
            raise HipError(f'dense_split: in_rowmax must hold one value per row ({B}), got {in_rowmax.numel()}')
        amax = torch.zeros(B, dtype=torch.float32, device=x.device) if want_rowmax else None
        _check(lib().roreg_dense_f16x2(_ptr(x, torch.float32), _ptr(layer.ws2), layer.w_exp, _ptr(layer.bias), _ptr(layer.scale), _ptr(layer.shift),
                                       layer.act_smax, layer.act_tmax, _ptr(in_rowmax, torch.float32), _res_ptr(residual), int(residual_stride), _ptr(out),
                                       _ptr(amax), B, K, layer.O, _stream()), 'roreg_dense_f16x2')
        return (out, amax) if want_rowmax else out
    _check(lib().roreg_dense_split(_ptr(x, torch.float32), _ptr(layer.ws), _ptr(layer.bias), _ptr(layer.scale), _ptr(layer.shift),
                                   _res_ptr(residual), int(residual_stride), _ptr(out), B, K, layer.O, _stream()), 'roreg_dense_split')
    return out


def group_conv_split_pack(W):
    """W [Cout,Cin,1,KS] / [Cout,Cin,KS] float32 -> int16 device tensor [3][KS][Cin/16][2][Cout][8] (group_conv_split_kernel's
    fragment order: piece p of W[o, 16*(c/16) + 8*h + e, k])."""
    Wn = W.detach().to('cpu', torch.float32).contiguous().numpy()
    return torch.from_numpy(bf16_split3_frags(Wn.reshape(Wn.shape[0], Wn.shape[1], -1))).cuda()
