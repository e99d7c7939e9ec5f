"""CPU half of the streaming-kernel tests: every family of tests/_pointwise_cases.py meets the condition the GPU tests
(tests/test_hip_pointwise.py) rely on, and the references of tests/_pointwise_oracle.py agree with oracle/ref_numpy.py on ordinary data."""
import numpy as np
import pytest
import torch

import _pointwise_cases as C
import _pointwise_oracle as PO
from conftest import load_golden
from oracle import ref_numpy as O

f32, f64 = np.float32, np.float64
TINY = np.finfo(f32).tiny


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == f32 else np.uint16)


# ---- gf_finalize ----------------------------------------------------------------------------------------------------------------------------
def test_gf_references_equal_the_oracles_closing_lines(monkeypatch):
    """oracle/ref_numpy.py gf_forward with the network replaced by y = 0 (eqv = 0 + x) is its closing normalisation alone."""
    monkeypatch.setattr(O, 'group_conv', lambda x, *a: x)
    monkeypatch.setattr(O, 'residual_comb_conv', lambda x, *a: x)
    monkeypatch.setattr(O, 'comb_conv', lambda x, *a: np.zeros_like(x))
    x = C.gf('randn', 5)
    want = O.gf_forward(x, {'PartI_net.Conv_in.0.weight': None, 'PartI_net.Conv_in.0.bias': None}, None)
    e32, i32 = PO.gf_finalize_f32(x)
    assert np.array_equal(bits(e32), bits(want['eqv'])) and np.array_equal(bits(i32), bits(want['inv']))
    e64, i64 = PO.gf_finalize_f64(x)
    assert PO.max_err(want['eqv'], e64) < 2e-7 and PO.max_err(want['inv'], i64) < 2e-7
    assert np.abs(np.sqrt((e64 * e64).sum(1)) - 1).max() < 1e-12 and np.abs(np.sqrt((i64 * i64).sum(1)) - 1).max() < 1e-12


def test_gf_cases_reach_the_clamp_the_underflow_and_the_cancellation():
    with np.errstate(all='ignore'):
        x = C.gf('scaled')
        n2 = (x * x).sum(1)
        assert np.abs(x).max() <= 1e18 and np.isfinite(n2).all() and n2.dtype == f32
        s = np.sqrt(n2.astype(f64)).mean(1)
        assert s.min() < 1e-11 and s.max() > 1e12 and (np.sqrt(n2) < C.CLAMP).any() and (np.sqrt(n2) > 1).any()
        x = C.gf('underflow')
        assert (x != 0).all() and ((x * x) == 0).all()                          # every float32 square is zero: the norm is the clamp
        e64, _ = PO.gf_finalize_f64(x)
        assert np.array_equal(e64, x.astype(f64) / f64(C.CLAMP))                # and the float64 reference clamps there too
    x = C.gf('near_clamp')
    r = np.sqrt((x.astype(f64) ** 2).sum(1)) / f64(C.CLAMP)
    for fac in C.NEAR_CLAMP_FACTORS:
        assert (np.abs(r - fac) < 1e-6).sum() >= x.shape[0] * C.G // len(C.NEAR_CLAMP_FACTORS) - 1, fac
    assert ((r < 1) & (r > 1 - 2e-6)).sum() > 300 and ((r > 1) & (r < 1 + 2e-6)).sum() > 300
    e64, _ = PO.gf_finalize_f64(x)
    assert np.abs(np.sqrt((e64 ** 2).sum(1)) - np.minimum(r, 1.0)).max() < 1e-12   # below the clamp the output's norm is r, not 1: a 1e-5 clamp would give 1
    x = C.gf('zeros')
    assert not x[list(C.ZERO_KEYPOINTS)].any() and all(not x[b, :, g].any() for b, g in C.ZERO_COLUMNS)
    e32, i32 = PO.gf_finalize_f32(x)
    assert np.isfinite(e32).all() and not e32[list(C.ZERO_KEYPOINTS)].any() and not i32[list(C.ZERO_KEYPOINTS)].any()
    x = C.gf('cancel').astype(f64)
    ratio = np.abs(x.mean(-1)) / np.sqrt((x * x).mean(-1))
    assert 2e-4 < np.median(ratio) < 2e-3 and ratio.max() < 1e-2
    x = C.gf('subnormal')
    assert (x != 0).all() and (np.abs(x) < TINY).all()
    out = x / C.CLAMP
    assert out.dtype == f32 and (np.abs(out) < TINY).sum() > 10000 and (np.abs(out) >= TINY).sum() > 10000
    sub16 = np.abs(C.bf16_values(out)) < TINY
    assert sub16.sum() > 10000                                                  # bfloat16 subnormals among the stored values


def test_gf_poisoned_block_differs_in_its_two_keypoints_only():
    clean, bad = C.gf_poisoned()
    assert clean.shape == (5, 32, 60) and np.isfinite(clean).all()
    diff = (bits(clean) != bits(bad)).reshape(5, -1).sum(1)
    assert diff.tolist() == [0, 1, 0, 1, 0] and np.isposinf(bad[C.POISON_INF]) and np.isnan(bad[C.POISON_NAN])
    e32, i32 = PO.gf_finalize_f32(bad)
    b, f, g = C.POISON_INF                      # inf / inf at the element, finite / inf = 0 in the rest of its column; the same in inv
    assert np.isnan(e32[b, f, g]) and np.isnan(e32[b]).sum() == 1 and not np.delete(e32[b, :, g], f).any()
    assert np.isnan(i32[b, f]) and np.isnan(i32[b]).sum() == 1 and not np.delete(i32[b], f).any()
    b, f, g = C.POISON_NAN                      # clamp_min keeps a NaN norm: the whole column, and all of inv
    assert np.isnan(e32[b, :, g]).all() and np.isnan(e32[b]).sum() == 32 and np.isnan(i32[b]).all()
    assert not np.isnan(e32[[0, 2, 4]]).any() and not np.isnan(i32[[0, 2, 4]]).any()


@pytest.mark.parametrize('route', ['clamp', 'unit'])
def test_planted_ties_are_exact_in_float32_and_cover_both_parities_and_signs(route):
    x, pos, t = C.ties_clamp() if route == 'clamp' else C.ties_unit()
    tb = bits(t)
    assert (tb & 0xFFFF == 0x8000).all() and (np.abs(t) > 0.05).all() and (np.abs(t) < 1).all()
    census = C.tie_census(t)
    for parity in (0, 1):
        assert census[parity, 0] + census[parity, 1] >= 64, census
    assert min(census.values()) >= 16, census                                     # both signs at both parities
    n = np.sqrt((x.astype(f64) ** 2).sum(1))
    if route == 'clamp':
        assert (n[n > 0] < f64(C.CLAMP) * 0.9991).all() and (x[pos] == (t * C.CLAMP).astype(f32)).all()
    else:
        assert np.abs(n - 1).max() < 2e-7 and ((x * x).sum(1) == 1).all() and np.array_equal(x[pos], t)
    e32, _ = PO.gf_finalize_f32(x)
    assert np.array_equal(bits(e32[pos]), tb)                                     # every planted position of the float32 output holds T exactly
    rne, cut = PO.bf16_bits(t), PO.bf16_bits_truncated(t)
    assert np.array_equal(rne.astype(np.int64) - cut, (tb >> 16) & 1)             # a tie goes to the even neighbour: up exactly where bit 16 is set
    assert np.array_equal(rne, bits(torch.from_numpy(t.copy()).to(torch.bfloat16).view(torch.int16).numpy().astype(np.uint16)))


def test_bf16_integer_rounding_is_torchs():
    x = np.concatenate([C.gf('randn', 5).ravel(), C.gf('subnormal').ravel() / C.CLAMP, C.ties_unit()[0].ravel()]).astype(f32)
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(PO.bf16_bits(x), want.view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(bits(C.bf16_values(x)), bits(want.float().numpy()))


# ---- det_score -------------------------------------------------------------------------------------------------------------------------------
def test_det_reference_equals_the_oracle_in_float64_and_the_float32_oracle_is_as_noisy_as_stated(group):
    z = load_golden('rd_forward')
    want = PO.det_score_f64(z['enc'], group.P)
    assert np.abs(O.rd_scores_from_encoding(z['enc'].astype(f64), group.P).astype(f64) - want).max() < 1e-6       # (the oracle casts its result to float32)
    assert np.abs(z['scores'] - want).max() < 5e-5
    for name, lo, hi, size in (('randn', 3e-6, 3e-5, 8.0), ('scaled', 3e-6, 3e-5, 8.0), ('onehot', 3e-6, 3e-5, 8.0), ('invariant', 1e-5, 1e-4, 7e-6)):
        x = C.det(name)
        s64 = PO.det_score_f64(x, group.P)
        err = np.abs(O.rd_scores_from_encoding(x, group.P).astype(f64) - s64).max()
        assert lo < err < hi, (name, err)
        assert 0.5 * size < np.median(s64) < 2 * size, (name, np.median(s64))
    x = C.det('scaled').astype(f64)
    assert np.abs(PO.det_score_f64(x, group.P) - PO.det_score_f64(x / np.abs(x).max((1, 2), keepdims=True), group.P)).max() < 1e-12   # scale-invariant
    x = C.det('onehot').astype(f64)
    n = np.sqrt((x * x).sum(1))
    assert (np.sort(n, 1)[:, -1] > 1e5 * np.sort(n, 1)[:, -2]).all()


def test_det_dead_column_gives_nan_for_its_keypoint_only(group):
    clean, dead = C.det_dead()
    assert (bits(clean) != bits(dead)).reshape(4, -1).sum(1).tolist() == [0, 0, 16, 0]
    with np.errstate(all='ignore'):
        s = O.rd_scores_from_encoding(dead, group.P)
        s64 = PO.det_score_f64(dead, group.P)
    assert np.isnan(s).tolist() == [False, False, True, False] and np.isnan(s64).tolist() == [False, False, True, False]


# ---- inv_descriptor --------------------------------------------------------------------------------------------------------------------------
def inv_inputs():
    for name in C.INV_VALUE_CASES:
        yield name, C.inv(name)
        yield name + ' as bfloat16', C.bf16_values(C.inv(name))
    for n in C.INV_SIZES:
        yield f'spread {n}', C.inv('spread', n)


def test_inv_model_is_numpys_bits_and_only_in_numpys_order():
    z = load_golden('pipeline_mutual_yohoo')
    assert np.array_equal(bits(PO.inv_descriptor_model(z['yoho_0'])), bits(O.inv_descriptor(z['yoho_0']).astype(f32)))
    for name, x in inv_inputs():
        want = O.inv_descriptor(x)
        assert want.dtype == f32, name
        assert np.array_equal(bits(PO.inv_descriptor_model(x)), bits(want)), name
        live = np.repeat(x.reshape(x.shape[0], -1).any(1)[:, None], 32, 1)
        if live.sum() < 64 * 32:
            continue                                                            # (the tail sizes: too few values for a share)
        seq = PO.inv_descriptor_model(x, order='sequential')
        share = (bits(seq) != bits(want))[live].mean()
        assert share >= 0.25, (name, share)
        # `sum / 60` in float32: the correctly rounded float32 quotient IS the float64 quotient cast back (s is a multiple of 2^-18 of the
        # quotient's binade, 60 x a float32 rounding boundary an odd multiple of 2^-22 of it: the quotient stays 2^-28 of the binade away from
        # every boundary, the float64 rounding moves it by 2^-53), so only the multiplication by float32(1 / 60), the form gf_finalize's mean
        # takes, can differ -- and it does
        assert np.array_equal(bits(PO.inv_descriptor_model(x, divide='f32')), bits(want)), name
        share = (bits(PO.inv_descriptor_model(x, divide='recip')) != bits(want))[live].mean()
        assert share >= 0.05, (name, share)
    x = C.inv('zeros')
    assert not O.inv_descriptor(x)[list(C.INV_ZERO_KEYPOINTS)].any() and O.inv_descriptor(x)[1].any()
    x = C.inv('cancel').astype(f64)
    assert np.median(np.abs(x.sum(-1)) / np.abs(x).sum(-1)) < 2e-2 and (np.sign(x[..., 0::2]) != np.sign(x[..., 1::2])).all()
    x = np.abs(C.inv('spread').astype(f64))
    assert np.median(x.max(-1) / x.min(-1)) > 2.0 ** 30


# ---- quat_to_trans ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [False, True])
@pytest.mark.parametrize('M', C.QUAT_SIZES)
def test_quat_cases_and_the_normalisation_model(group, M, rows):
    c = C.quat(M, rows)
    q = c['q']
    assert q.shape == (M, 4) and np.isfinite(q).all() and c['anchor'].shape == (M,)
    qn = PO.quat_normalize_model(q)
    q64 = q.astype(f64)
    assert np.abs(qn - q64 / np.sqrt((q64 * q64).sum(1))[:, None]).max() < 2e-7
    assert (np.sign(qn[:, 0]) == np.sign(q[:, 0])).all()
    if M >= 60:
        assert set(c['anchor'].tolist()) == set(range(60))
        n = np.sqrt((q64 * q64).sum(1))
        assert n.min() < 1e-13 and n.max() > 1e13 and (q[:, 0] < 0).sum() > M // 4 and (q[:, 0] > 0).sum() > M // 4
    for k in (c['keys0'], c['keys1']):
        assert k.dtype == f64 and k.shape == ((C.QUAT_TABLE if rows else M), 3)
        assert (k[0::2] >= 0).all() and (k[0::2] <= 3).all() and (M < 60 or np.abs(k[1::2]).max() > 900)
    if rows:
        for r in (c['rows0'], c['rows1']):
            assert r.dtype == np.int64 and r.min() >= 0 and r.max() < C.QUAT_TABLE and (M == 1 or np.unique(r).shape[0] < M) and (M == 1 or (np.diff(r) < 0).any())
    else:
        assert c['rows0'] is None and c['rows1'] is None
    # the bar can be met: the kernel's stated order in numpy float64 against rt_pre's matmuls
    k0 = c['keys0'] if not rows else c['keys0'][c['rows0']]
    k1 = c['keys1'] if not rows else c['keys1'][c['rows1']]
    want = O.rt_pre(qn, c['anchor'], group.R.astype(f32), k0, k1)
    assert (np.abs(PO.quat_to_trans_model(qn, c['anchor'], group.R.astype(f32), k0, k1) - want) <= PO.trans_bar(k0, k1)).all()
