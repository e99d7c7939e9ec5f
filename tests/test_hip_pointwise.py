"""The per-keypoint streaming kernels (roreg_amd/csrc/pointwise.hip) called through their bindings, one kernel at a time, against the
references of tests/_pointwise_oracle.py on the families of tests/_pointwise_cases.py (whose conditions tests/test_pointwise_oracle.py asserts
on the CPU).

Bars.  gf_finalize and det_score: 4 x the maximum error of the SAME formula evaluated in numpy float32, both measured against float64 on the
case at hand (gf_finalize: never below 2^-22 of the output scale); each test prints the kernel's and numpy's error before it asserts.
The bfloat16 store, inv_descriptor and the normalised quaternion: bit for bit.  Local transforms: 8 double ulps at max(1, |k0|, |k1|)."""
import functools

import numpy as np
import pytest
import torch

import _pointwise_cases as C
import _pointwise_oracle as PO
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
GF_CASES = [('randn', B) for B in C.TAILS] + [(name, 64) for name in C.GF_VALUE_CASES]
DET_CASES = [('randn', B) for B in C.DET_SIZES] + [(name, 64) for name in C.DET_VALUE_CASES]
INV_CASES = [('spread', N) for N in C.INV_SIZES] + [(name, 64) for name in C.INV_VALUE_CASES]


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).cuda()            # (a copy: the cases are read-only arrays)


def bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def gf_device(x, want_inv=True, bf16=False):
    """-> (eqv: float32 ndarray, or the uint16 patterns of the bfloat16 store; inv float32 or None)."""
    from roreg_amd import hip
    e, i = hip.gf_finalize(cu(x), want_inv=want_inv, out_dtype=torch.bfloat16 if bf16 else torch.float32)
    assert e.shape == x.shape and (i is None) == (not want_inv)
    e = e.view(torch.int16).cpu().numpy().view(np.uint16) if bf16 else e.cpu().numpy()
    return e, None if i is None else i.cpu().numpy()


def torch_bf16_bits(e32):
    """float32 ndarray -> uint16 patterns of torch's float32 -> bfloat16 conversion on the host."""
    return torch.from_numpy(np.ascontiguousarray(e32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def gf_input(name, B):
    if name == 'ties_clamp':
        return C.ties_clamp()[0]
    if name == 'ties_unit':
        return C.ties_unit()[0]
    return C.gf(name, B)


@functools.lru_cache(maxsize=None)
def gf_refs(name, B):
    x = gf_input(name, B)
    return PO.gf_finalize_f64(x), PO.gf_finalize_f32(x)


# ---- 1. gf_finalize, float32 store ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,B', GF_CASES)
def test_gf_finalize_float32_within_4x_numpys_float32_error(name, B):
    x = gf_input(name, B)
    (e64, i64), (e32, i32) = gf_refs(name, B)
    e, i = gf_device(x)
    figures = {}
    for what, got, ref32, ref64 in (('eqv', e, e32, e64), ('inv', i, i32, i64)):
        assert got.dtype == f32 and got.shape == ref64.shape and not np.isnan(got).any(), what
        figures[what] = (PO.max_err(got, ref64), PO.max_err(ref32, ref64))
        print(f'gf_finalize {name} B={B} {what}: kernel {figures[what][0]:.3e}  numpy float32 {figures[what][1]:.3e}  bar {PO.bar(figures[what][1]):.3e}')
    for what, (kernel, numpy32) in figures.items():
        assert kernel <= PO.bar(numpy32), (name, what, kernel, numpy32)
    e_alone, none = gf_device(x, want_inv=False)
    assert none is None and same_bits(e_alone, e)                                # the inv half does not touch eqv
    if name == 'zeros':
        zk = list(C.ZERO_KEYPOINTS)
        assert not bits(e[zk]).any() and not bits(i[zk]).any()                   # exact +0.0
        for b, g in C.ZERO_COLUMNS:
            assert not bits(e[b, :, g]).any() and e[b].any()
    if name == 'underflow':
        assert same_bits(e, x / C.CLAMP)                                         # the clamp alone: one correctly rounded division
    if name == 'subnormal':
        assert same_bits(e, x / C.CLAMP)                                         # subnormal operands and quotients kept, not flushed
        assert (np.abs(e) < np.finfo(f32).tiny).sum() > 10000 and e.all()


def test_gf_finalize_non_finite_keypoints_stay_in_their_own_wave():
    clean, bad = C.gf_poisoned()
    e0, i0 = gf_device(clean)
    e1, i1 = gf_device(bad)
    for b in (0, 2, 4):
        assert same_bits(e1[b], e0[b]) and same_bits(i1[b], i0[b]), b
    e32, i32 = PO.gf_finalize_f32(bad)
    assert np.array_equal(np.isnan(e1), np.isnan(e32)) and np.array_equal(np.isnan(i1), np.isnan(i32))
    assert np.array_equal(e1 == 0, e32 == 0) and np.array_equal(i1 == 0, i32 == 0)
    b, f, g = C.POISON_INF
    keep = np.ones(60, bool); keep[g] = False
    assert same_bits(e1[b][:, keep], e0[b][:, keep])                             # the +inf's keypoint outside its column
    assert np.isnan(e1[C.POISON_INF]) and np.isnan(e1[C.POISON_NAN]) and np.isnan(e1[C.POISON_NAN[0], :, C.POISON_NAN[2]]).all()
    eb, ib = gf_device(bad, bf16=True)                                           # the bfloat16 store of the same block: NaN where the float32 store is
    nan = np.isnan(e1)
    assert np.array_equal((eb & 0x7FFF) > 0x7F80, nan) and np.array_equal(eb[~nan], PO.bf16_bits(e1)[~nan])
    assert np.array_equal(np.isnan(ib), np.isnan(i1)) and np.array_equal(bits(ib)[~np.isnan(i1)], bits(i1)[~np.isnan(i1)])


# ---- 2. gf_finalize, bfloat16 store ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,B', GF_CASES + [('ties_clamp', 16), ('ties_unit', 16)])
def test_gf_finalize_bfloat16_store_is_the_float32_store_rounded_to_nearest_even(name, B):
    x = gf_input(name, B)
    e, i = gf_device(x)
    eb, ib = gf_device(x, bf16=True)
    want = torch_bf16_bits(e)
    assert np.array_equal(want, PO.bf16_bits(e))                                 # (torch's conversion is the integer formula)
    differ = eb != want
    print(f'gf_finalize bf16 {name} B={B}: {int(differ.sum())} of {differ.size} stored values differ from round-to-nearest-even of the float32 store')
    assert not differ.any(), (name, int(differ.sum()), e[differ][:4], eb[differ][:4], want[differ][:4])
    assert same_bits(ib, i)                                                      # inv comes from the float32 values either way
    assert np.array_equal(gf_device(x, want_inv=False, bf16=True)[0], eb)


@pytest.mark.parametrize('route', ['clamp', 'unit'])
def test_gf_finalize_lands_on_planted_ties_and_rounds_them_to_even(route):
    x, pos, t = C.ties_clamp() if route == 'clamp' else C.ties_unit()
    e, _ = gf_device(x)
    got = e[pos]
    miss = bits(got) != bits(t)
    print(f'gf_finalize ties {route}: {int(miss.sum())} of {t.size} planted positions miss their tie in the float32 store')
    assert not miss.any(), (route, int(miss.sum()), got[miss][:4], t[miss][:4])  # no FMA in the norm, correctly rounded sqrt and divide
    gb = bits(got)
    assert (gb & 0xFFFF == 0x8000).all() and (np.abs(got) > 0.05).all() and (np.abs(got) < 1).all()
    census = C.tie_census(got)
    for parity in (0, 1):
        assert census[parity, 0] + census[parity, 1] >= 64, census
    assert min(census.values()) >= 16, census
    eb, _ = gf_device(x, bf16=True)
    up = eb[pos].astype(np.int64) - PO.bf16_bits_truncated(got)
    assert np.array_equal(up, (gb >> 16) & 1), (route, int((up != ((gb >> 16) & 1)).sum()))      # up exactly where bit 16 is set
    assert (eb[pos] & 1 == 0).all()


# ---- 3. det_score ----------------------------------------------------------------------------------------------------------------------------
def det_device(x):
    from roreg_amd import hip
    s = hip.det_score(cu(x)).cpu().numpy()
    assert s.shape == (x.shape[0],) and s.dtype == f32
    return s


@pytest.mark.parametrize('name,B', DET_CASES)
def test_det_score_within_4x_the_float32_oracles_error(group, name, B):
    x = C.det(name, B)
    s64 = PO.det_score_f64(x, group.P)
    numpy32 = PO.max_err(O.rd_scores_from_encoding(x, group.P), s64)
    kernel = PO.max_err(det_device(x), s64)
    print(f'det_score {name} B={B}: kernel {kernel:.3e}  numpy float32 {numpy32:.3e}  bar {4 * numpy32:.3e}  (median score {np.median(s64):.3e})')
    assert kernel <= 4 * numpy32, (name, B, kernel, numpy32)


def test_det_score_dead_keypoint_is_nan_alone(group):
    clean, dead = C.det_dead()
    s0, s1 = det_device(clean), det_device(dead)
    assert np.isnan(s1).tolist() == [False, False, True, False] and not np.isnan(s0).any()
    keep = [0, 1, 3]
    assert same_bits(s1[keep], s0[keep])


# ---- 4. inv_descriptor -----------------------------------------------------------------------------------------------------------------------
def inv_device(x, bf16=False, roles=False):
    from roreg_amd import hip
    t = cu(x).to(torch.bfloat16) if bf16 else cu(x)
    if not roles:
        return hip.inv_descriptor(t).cpu().numpy()
    rng = np.random.default_rng(5)
    scale, shift = cu(rng.uniform(0.5, 1.5, 128).astype(f32)), cu(rng.normal(0, 0.1, 128).astype(f32))
    role = torch.zeros((x.shape[0], 4), dtype=torch.float32, device='cuda')
    return hip.inv_descriptor(t, roles=(scale, shift, role)).cpu().numpy()


@pytest.mark.parametrize('name,N', INV_CASES)
def test_inv_descriptor_has_numpys_bits_where_the_order_decides_them(name, N):
    x = C.inv(name, N)
    want = O.inv_descriptor(x)
    got = inv_device(x)
    assert same_bits(got, want), (name, N, int((bits(got) != bits(want)).sum()))
    assert same_bits(inv_device(x, roles=True), want)
    xb = C.bf16_values(x)                                                        # the same values as stored in bfloat16: the oracle is fed the rounded ones
    want = O.inv_descriptor(xb)
    got = inv_device(xb, bf16=True)
    assert same_bits(got, want), (name, N, 'bfloat16', int((bits(got) != bits(want)).sum()))
    assert same_bits(inv_device(xb, bf16=True, roles=True), want)
    if name == 'zeros':
        zk = list(C.INV_ZERO_KEYPOINTS)
        assert not bits(got[zk]).any() and got[1].any()


# ---- 5. quat_to_trans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows', [False, True])
@pytest.mark.parametrize('M', C.QUAT_SIZES)
def test_quat_to_trans_quaternion_bits_and_transform_to_8_ulps(group, M, rows):
    from roreg_amd import hip
    c = C.quat(M, rows)
    T, qn = hip.quat_to_trans(cu(c['q']), cu(c['anchor']), cu(c['keys0']), cu(c['keys1']), rows0=cu(c['rows0']), rows1=cu(c['rows1']), want_quat=True)
    T, qn = T.cpu().numpy(), qn.cpu().numpy()
    want_q = PO.quat_normalize_model(c['q'])
    assert same_bits(qn, want_q), (M, rows, int((bits(qn) != bits(want_q)).sum()))
    k0 = c['keys0'][c['rows0']] if rows else c['keys0']
    k1 = c['keys1'][c['rows1']] if rows else c['keys1']
    want = O.rt_pre(qn, c['anchor'], group.R.astype(f32), k0, k1)
    err = np.abs(T - want) / PO.trans_bar(k0, k1) * 8.0
    print(f'quat_to_trans M={M} rows={rows}: worst element {err.max():.2f} double ulps at max(1, |k0|, |k1|)  (bar 8)')
    assert T.shape == (M, 3, 4) and (np.abs(T - want) <= PO.trans_bar(k0, k1)).all(), (M, rows, err.max())
    T_alone = hip.quat_to_trans(cu(c['q']), cu(c['anchor']), cu(c['keys0']), cu(c['keys1']), rows0=cu(c['rows0']), rows1=cu(c['rows1'])).cpu().numpy()
    assert same_bits(T_alone, T)
