"""The end of the extractor in one pass per keypoint (irrep_gemm_thin_m_rows_kernel + gf_finish_kernel, csrc/fourier.hip) against the four launches it
replaces -- ft_nonlin, gf_finalize, inv_descriptor, feat_coefs: the same arithmetic per (keypoint, channel) column, so every comparison is bit for bit
(torch.equal on the int32 views: NaN positions included).  fp16 x 2, float32 storage.  GPU only."""
import functools

import numpy as np
import pytest
import torch

from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu

# one keypoint; both sides of a 32-column block; several thin-M workgroups per irrep with a ragged last one
BATCHES = [1, 31, 33, 300]


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _gf():
    """(FourierGF of a seeded GF_test, role tables (scale [128], shift [128]))"""
    from roreg_amd import hip
    from roreg_amd.network import name2network
    from roreg_amd.network.gf_fourier import FourierGF
    assert hip.GEMM_MODE == 'f16x2'
    net = name2network['GF_test'](default_config())
    synth.seeded_state_dict(net, 77)
    f = FourierGF(net.PartI_net)
    f.gemm = 'f16x2'
    f._plan()
    g = torch.Generator(device='cuda'); g.manual_seed(5)
    return f, (torch.randn(128, device='cuda', generator=g), torch.randn(128, device='cuda', generator=g))


@functools.lru_cache(maxsize=None)
def _features(B):
    g = torch.Generator(device='cuda'); g.manual_seed(100 + B)
    return torch.randn((B, 32, 60), device='cuda', generator=g)


def _rows_of(T3, B):
    """operand layout [60*32*Bp] -> per-keypoint rows [Bp,60,32]: q = irrep offset + i d + l is the element at row (l, o), column block i (an index permutation)"""
    from roreg_amd import hip
    Bp = hip.coef_pitch(B)
    parts = [v.view(d, 32, Bp // 32, d, 32).permute(2, 4, 3, 0, 1).reshape(Bp, d * d, 32) for d, v in zip(hip.IRREP_DIMS, hip.coef_views(T3, 32, B))]
    return torch.cat(parts, 1).contiguous()


def _four_kernels(T3, x, bias, roles):
    """(eqv, inv, role table, eqv_ft) of the four launches from T3 in the operand layout"""
    from roreg_amd import hip
    B = x.shape[0]
    role = torch.full((B, 4), -1.0, device='cuda') if roles is not None else None
    r = (roles[0], roles[1], role) if roles is not None else None
    raw = hip.ft_nonlin(B, 32, coef_in=T3, bias=bias, resid_spatial=x, spatial_out=True, split='f16x2')
    eqv, _ = hip.gf_finalize(raw, want_inv=False)
    return eqv, hip.inv_descriptor(eqv, roles=r), role, hip.feat_coefs(eqv)


def _one_kernel(T3r, x, bias, roles):
    from roreg_amd import hip
    role = torch.full((x.shape[0], 4), -1.0, device='cuda') if roles is not None else None
    eqv, inv, eft = hip.gf_finish_rows(T3r, x, bias, roles=(roles[0], roles[1], role) if roles is not None else None)
    return eqv, inv, role, eft


def _assert_same(new, old, what):
    for name, a, b in zip(('eqv', 'inv', 'role', 'eqv_ft'), new, old):
        if a is None and b is None:
            continue
        if name == 'role':
            assert bool((a[:, :2] == -1.0).all()), (what, 'role columns 0 and 1 belong to row_bound')
            a, b = a[:, 2:], b[:, 2:]
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (what, name, int((_bits(a) != _bits(b)).sum()))


@pytest.mark.parametrize('B', BATCHES)
def test_thin_m_rows_are_the_operand_layout_permuted(group, B):
    """thin M with the rows flag against thin M without it, from the extractor's own Conv_out operand"""
    from roreg_amd import hip
    f, _ = _gf()
    X3, b3 = f._conv_out_operand(_features(B))
    with hip.gemm_thin(True):
        T3 = hip.irrep_gemm(X3, None, 256, 32, B, f16x2=f.l_out.wsplit2, x_bound=b3)
    T3r = hip.irrep_gemm_rows(X3, 256, B, f.l_out.wsplit2, b3)
    assert float(T3.abs().max()) > 0 and torch.equal(_bits(T3r), _bits(_rows_of(T3, B)))


@pytest.mark.parametrize('roles', [True, False])
@pytest.mark.parametrize('B', BATCHES)
def test_route_is_bitwise_the_four_kernels(group, B, roles):
    """FourierGF.forward_finished against gf_finalize(forward_raw), inv_descriptor, feat_coefs under hip.gf_finish(False); the role table's four columns"""
    from roreg_amd import hip
    f, bn = _gf()
    x = _features(B)
    tables = [torch.full((B, 4), -1.0, device='cuda') for _ in range(2)] if roles else [None, None]
    new = f.forward_finished(x, roles=(bn[0], bn[1], tables[0]) if roles else None)
    with hip.gf_finish(False):
        assert not hip.gf_finish_usable('f16x2', torch.float32)
        r = (bn[0], bn[1], tables[1]) if roles else None
        eqv, _ = hip.gf_finalize(f.forward_raw(x, roles=r), want_inv=False)
        old = (eqv, hip.inv_descriptor(eqv, roles=r), hip.feat_coefs(eqv))
    assert hip.gf_finish_usable('f16x2', torch.float32) and not hip.gf_finish_usable('f16x2', torch.bfloat16) and not hip.gf_finish_usable('bf16x3', torch.float32)
    for name, a, b in zip(('eqv', 'inv', 'eqv_ft'), new, old):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (name, int((_bits(a) != _bits(b)).sum()))
    assert bool(torch.isfinite(new[0]).all()) and float(new[0].abs().max()) > 0
    if roles:
        assert torch.equal(_bits(tables[0]), _bits(tables[1])) and bool((tables[0] >= 0).all())


@pytest.mark.parametrize('zero_bias', [False, True])
@pytest.mark.parametrize('B', [33, 300])
def test_planted_keypoints(group, B, zero_bias):
    """T3 planted in the operand layout: an all-zero keypoint with a zero x row (with a zero bias its norm is 0: the 1e-4 clamp of the channel norm and a
    zero column maximum in both transforms; inv = 0 / 1e-5), a NaN in one keypoint (it must stay in that keypoint and sit at the same positions), and
    channel magnitudes spanning 2^20 inside the keypoints (every column carries its own block scale)."""
    from roreg_amd import hip
    f, bn = _gf()
    Bp = hip.coef_pitch(B)
    g = torch.Generator(device='cuda'); g.manual_seed(900 + B)
    T3 = torch.randn(hip.coef_size(32, B), device='cuda', generator=g)
    x = _features(B).clone()
    cscale = torch.ldexp(torch.ones(32, device='cuda'), torch.arange(32, device='cuda').float() * (20.0 / 31.0) // 1 - 10)       # 2^-10 .. 2^10 over the channels
    zero_kp, nan_kp = (0, B - 1), 17
    for d, v in zip(hip.IRREP_DIMS, hip.coef_views(T3, 32, B)):
        v5 = v.view(d, 32, Bp // 32, d, 32)                                   # [l][o][b / 32][i][b % 32]
        v5.mul_(cscale[None, :, None, None, None])
        for b in zero_kp:
            v5[:, :, b // 32, :, b % 32] = 0.0
    x[list(zero_kp)] = 0.0
    hip.coef_views(T3, 32, B)[3].view(4, 32, Bp // 32, 4, 32)[2, 7, nan_kp // 32, 1, nan_kp % 32] = float('nan')
    bias = torch.zeros(32, device='cuda') if zero_bias else f.l_out.bias
    new = _one_kernel(_rows_of(T3, B), x, bias, bn)
    old = _four_kernels(T3, x, bias, bn)
    _assert_same(new, old, (B, zero_bias))
    eqv, inv, role, eft = new
    nan_rows = torch.isnan(eqv).flatten(1).any(1).nonzero().flatten().tolist()
    assert nan_rows == [nan_kp] and torch.isnan(eft).flatten(1).any(1).nonzero().flatten().tolist() == [nan_kp]
    if zero_bias:
        for b in zero_kp:
            assert int(_bits(eqv[b]).abs().max()) == 0 and int(_bits(inv[b]).abs().max()) == 0 and int(_bits(eft[b]).abs().max()) == 0
    live = [b for b in range(B) if b not in zero_kp and b != nan_kp]
    n = eqv[live].double().pow(2).sum(1).sqrt()
    assert float((n - 1).abs().max()) < 1e-5                                  # unit norm over the channels at every group element


def test_engine_takes_the_route_and_the_switch_turns_it_off(group):
    """both extraction sites of RegistrationEngine: the same CloudState bits with the switch on and off, and the old route for bfloat16 storage"""
    from roreg_amd import hip
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.network import name2network
    cfg = default_config()
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    eng = RegistrationEngine(cfg, gf, et)
    feats = [_features(33).cpu().numpy(), _features(31).cpu().numpy()]
    keys = [np.zeros((33, 3)), np.zeros((31, 3))]
    calls = []
    real = hip.gf_finish_rows
    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    hip.gf_finish_rows = counted
    try:
        on = eng.extract_many(feats, keys) + [eng.extract(feats[0], keys[0])]
        assert len(calls) == 2
        with hip.gf_finish(False):
            off = eng.extract_many(feats, keys) + [eng.extract(feats[0], keys[0])]
        assert len(calls) == 2
        eng.set_descriptor_dtype('bf16')
        assert eng.extract(feats[0], keys[0]).eqv.dtype == torch.bfloat16 and len(calls) == 2
    finally:
        hip.gf_finish_rows = real
    for a, b in zip(on, off):
        for name in ('eqv', 'inv', 'eqv_ft', 'role'):
            ta, tb = getattr(a, name), getattr(b, name)
            assert (ta is None) == (tb is None)
            if ta is not None:
                assert torch.equal(_bits(ta), _bits(tb)), name
