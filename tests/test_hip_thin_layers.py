"""The extractor's thin layers on their own GEMM kernels (irrep_gemm_thin_k_kernel: C == 32; irrep_gemm_thin_m_kernel: O == 32) against the generic
fp16 x 2 kernel they replace: the same MFMA sequence per output element, so every comparison is bit for bit (hip.gemm_thin(True) against
hip.gemm_thin(False)), and against a float64 product of the unpacked operands so that the generic kernel is not the only witness.  GPU only."""
import functools

import numpy as np
import pytest
import torch

from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu

# one column block; valid < padded (pad columns must come out exact zeros); a workgroup with a single block behind a full one; two full
# workgroups plus a block (256 columns per workgroup at d = 1)
BATCHES = [32, 70, 288, 544]
THIN_K = [(32, 256), (32, 64), (32, 32)]
THIN_M = [(256, 32), (64, 32)]            # (64, 32): 4 d K16 steps, a loop no longer than the look-ahead at d = 1


@functools.lru_cache(maxsize=None)
def _layer(C, Oc):
    from roreg_amd.network.gf_fourier import _Layer
    torch.manual_seed(1000 * C + Oc)
    return _Layer(torch.nn.Conv2d(C, Oc, (1, 13)))


@functools.lru_cache(maxsize=None)
def _operands(C, Oc, B):
    """(packed words, per-keypoint bound, next-bound tables, float64 reference per irrep): per-keypoint magnitudes spread over 2^+-20 so that
    neighbouring columns carry different output scales, every tenth keypoint all zero, one channel 2^12 larger than the rest, pad keypoints 0."""
    from roreg_amd import hip
    L = _layer(C, Oc)
    g = torch.Generator(device='cuda'); g.manual_seed(7 * C + 3 * Oc + B)
    Bp = hip.coef_pitch(B)
    X = torch.randn(hip.coef_size(C, B), device='cuda', generator=g)
    kscale = torch.ldexp(torch.ones(Bp, device='cuda'), torch.randint(-20, 21, (Bp,), device='cuda', generator=g).float())
    kscale[::10] = 0.0
    kscale[B:] = 0.0
    for r, v in enumerate(hip.coef_views(X, C, B)):
        d = hip.IRREP_DIMS[r]
        v.mul_(kscale[hip._keypoint_of_columns(d, Bp)][None, :])
        v.view(d, C, d * Bp)[:, 5, :] *= 4096.0
    Xp, xb = hip.pack_coefs_f16x2(X, C, B)
    nb = (torch.rand(Oc, device='cuda', generator=g) + 0.5, torch.rand(Oc, device='cuda', generator=g))
    Xu = hip.unpack_coefs_f16x2(Xp, xb, C, B)
    ref = [L.dense[r][:hip.IRREP_DIMS[r] * Oc].astype(np.float64) @ v.double().cpu().numpy() for r, v in enumerate(hip.coef_views(Xu, C, B))]
    return Xp, xb, nb, ref


def _run(C, Oc, B, thin, bound, add=None):
    from roreg_amd import hip
    L = _layer(C, Oc)
    Xp, xb, nb, _ = _operands(C, Oc, B)
    with hip.gemm_thin(thin):
        out = hip.irrep_gemm(Xp, None, C, Oc, B, f16x2=L.wsplit2, x_bound=xb, next_bound=nb if bound else None, add=add)
    return out if bound else (out, None)


def _check(C, Oc, B, bound):
    from roreg_amd import hip
    T1, b1 = _run(C, Oc, B, True, bound)
    T0, b0 = _run(C, Oc, B, False, bound)
    Bp = hip.coef_pitch(B)
    for r, (v1, v0) in enumerate(zip(hip.coef_views(T1, Oc, B), hip.coef_views(T0, Oc, B))):
        assert torch.equal(v1.view(torch.int32), v0.view(torch.int32)), (r, C, Oc, B)
        pad = hip._keypoint_of_columns(hip.IRREP_DIMS[r], Bp) >= B
        assert int(v1[:, pad].view(torch.int32).abs().max() if bool(pad.any()) else 0) == 0, (r, 'pad columns')
    if bound:
        assert torch.equal(b1.view(torch.int32), b0.view(torch.int32))
    # the float64 product of the unpacked operands: 2e-6 of the tensor's scale, the bar of the fp16 x 2 GEMM in test_hip_fourier.py
    ref = _operands(C, Oc, B)[3]
    scale = max(float(np.abs(q).max()) for q in ref)
    for r, v1 in enumerate(hip.coef_views(T1, Oc, B)):
        err = float(np.abs(v1.double().cpu().numpy() - ref[r]).max())
        assert err <= 2e-6 * scale, (r, err / scale)


@pytest.mark.parametrize('bound', [False, True])
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('C,Oc', THIN_K)
def test_thin_k_is_bitwise_the_generic_kernel(group, C, Oc, B, bound):
    _check(C, Oc, B, bound)


@pytest.mark.parametrize('bound', [False, True])
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('C,Oc', THIN_M)
def test_thin_m_is_bitwise_the_generic_kernel(group, C, Oc, B, bound):
    _check(C, Oc, B, bound)


def test_switch_is_a_query_outside_zero_and_one(group):
    from roreg_amd import hip
    L = hip.lib()
    was = L.roreg_gemm_thin(-1)
    assert was in (0, 1) and L.roreg_gemm_thin(1 - was) == was and L.roreg_gemm_thin(7) == 1 - was
    assert L.roreg_gemm_thin(was) == 1 - was and L.roreg_gemm_thin(-1) == was


@pytest.mark.parametrize('C,Oc', [(32, 256), (256, 32)])
def test_residual_is_bitwise_the_generic_kernel(group, C, Oc):
    """add= keeps the generic kernel's o * oscale + res order (the thin kernels leave layers with a residual to it)."""
    from roreg_amd import hip
    B = 288
    add = torch.randn(hip.coef_size(Oc, B), device='cuda', generator=torch.Generator(device='cuda').manual_seed(11))
    T1, b1 = _run(C, Oc, B, True, True, add=add)
    T0, b0 = _run(C, Oc, B, False, True, add=add)
    assert torch.equal(T1.view(torch.int32), T0.view(torch.int32)) and torch.equal(b1.view(torch.int32), b0.view(torch.int32))


@pytest.mark.parametrize('C,Oc', [(32, 256), (256, 32)])
def test_a_keypoint_does_not_depend_on_its_batch(group, C, Oc):
    """The first 32 keypoints' columns are the same bits alone (B = 32) and inside B = 288."""
    from roreg_amd import hip
    L = _layer(C, Oc)
    Xp, xb, nb, _ = _operands(C, Oc, 288)
    small = torch.empty(hip.coef_size(C, 32), device='cuda')
    for d, vs, vb in zip(hip.IRREP_DIMS, hip.coef_views(small, C, 32), hip.coef_views(Xp, C, 288)):
        vs.copy_(vb[:, :32 * d])                                  # columns are blocked by 32 keypoints: the first block of every irrep
    with hip.gemm_thin(True):
        Ts, bs = hip.irrep_gemm(small, None, C, Oc, 32, f16x2=L.wsplit2, x_bound=xb[:32].contiguous(), next_bound=nb)
        Tb, bb = hip.irrep_gemm(Xp, None, C, Oc, 288, f16x2=L.wsplit2, x_bound=xb, next_bound=nb)
    for d, vs, vb in zip(hip.IRREP_DIMS, hip.coef_views(Ts, Oc, 32), hip.coef_views(Tb, Oc, 288)):
        assert torch.equal(vs.view(torch.int32), vb[:, :32 * d].contiguous().view(torch.int32))
    assert torch.equal(bs.view(torch.int32), bb[:32].contiguous().view(torch.int32))


def test_extractor_end_to_end_switch_on_equals_off(group):
    from roreg_amd import hip
    from roreg_amd.network import name2network
    net = name2network['GF_test'](default_config())
    synth.seeded_state_dict(net, 77)
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((100, 32, 60)).astype(np.float32)).cuda()
    net.PartI_net.mode = 'fourier'
    net(x[:8])                                                     # builds the FourierGF plan
    f = net.PartI_net._fourier
    with hip.gemm_thin(True):
        on = f.forward_raw(x)
    with hip.gemm_thin(False):
        off = f.forward_raw(x)
    assert torch.equal(on.view(torch.int32), off.view(torch.int32))
