"""The nearest-neighbour searches (roreg_amd/csrc/nn_search.hip) called through their bindings, one form at a time, against oracle/ref_numpy.py
(pdist, knn, mutual_check: the float32 restatement of the reference's formula) on the families of tests/_knn_cases.py, whose conditions
tests/test_knn_cases.py asserts on the CPU.  No tolerance anywhere: indices are compared as integers, distances through their bit patterns.

Which kernel a shape reaches (restated in _knn_cases, asserted on the CPU): nn_search at F = 3 / 32 -- the sliced kernel, one target per
slice up to n = 2048 / ceil(m/256), three per slice and a short last slice at (256, 4100) and (2305, 500); knn_search at F = 3 / 32, k <= 8 --
the single-pass kernel up to n = 32, slices + merge above (n = 33: 17 + 16); every other width, and k = 9..32 -- the generic kernel."""
import functools

import numpy as np
import pytest
import torch

import _knn_cases as C
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

f32 = np.float32


def cu(a):
    return None if a is None else torch.from_numpy(np.array(a, order='C')).cuda()            # (a copy: the cases are read-only arrays)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def dist_type(squared):
    return 'SquareL2' if squared else 'L2'


def assert_same(idx, dist, oi, od, what):
    """Device (idx, dist) tensors against the oracle's: integers equal, distances bit for bit."""
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    oi, od = oi.reshape(idx.shape), od.reshape(dist.shape)
    assert idx.dtype == np.int64 and dist.dtype == f32
    wrong = idx != oi
    assert not wrong.any(), (what, int(wrong.sum()), np.argwhere(wrong)[:4].tolist(), idx[wrong][:4], oi[wrong][:4])
    assert np.array_equal(bits(dist), bits(od)), (what, int((bits(dist) != bits(od)).sum()))


@functools.lru_cache(maxsize=None)
def oracle(family, F, m, n, k, form, squared):
    S, T = C.make(family, F, m, n, k, form)
    return O.knn(T, S, k, dist_type=dist_type(squared))


# ---- 1. nn_search -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('family,F,m,n', C.NN_CASES)
def test_nn_search_equals_the_oracle(family, F, m, n, squared):
    from roreg_amd import hip
    S, T = C.make(family, F, m, n)
    od, oi = oracle(family, F, m, n, 1, 'nn', squared)
    s, t = cu(S), cu(T)
    idx, d = hip.nn_search(s, t, want_dist=True, squared=squared)
    assert_same(idx, d, oi, od, (family, F, m, n, squared))
    assert torch.equal(hip.nn_search(s, t, squared=squared), idx)                            # the distance output does not touch the indices
    if family != 'duplicates' and m > 3 and n > 2:                                           # (the duplicates are placed by index in the whole array)
        r0, r1 = C.row_lists(m, n)
        od, oi = O.knn(T[r1], S[r0], 1, dist_type=dist_type(squared))
        idx, d = hip.nn_search(s, t, src_rows=cu(r0), tgt_rows=cu(r1), want_dist=True, squared=squared)
        assert_same(idx, d, oi, od, (family, F, m, n, squared, 'row lists'))


@pytest.mark.parametrize('family,F,m,n', [c for c in C.NN_CASES if c[0] in ('root_ties', 'root_shrink')])
def test_nn_search_distance_types_disagree_exactly_where_the_oracles_do(family, F, m, n):
    from roreg_amd import hip
    S, T = C.make(family, F, m, n)
    s, t = cu(S), cu(T)
    differ = (hip.nn_search(s, t) != hip.nn_search(s, t, squared=True)).cpu().numpy()
    want = oracle(family, F, m, n, 1, 'nn', False)[1] != oracle(family, F, m, n, 1, 'nn', True)[1]
    print(f'nn_search root_ties F={F} m={m} n={n}: L2 and SquareL2 differ in {int(differ.sum())} rows on the device, {int(want.sum())} in the oracle')
    assert want.sum() >= 8 and np.array_equal(differ, want)


# ---- 2. knn_search ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('family,F,m,n,k', C.KNN_CASES + C.KNN_GENERIC_CASES)
def test_knn_search_equals_the_oracle(family, F, m, n, k, squared):
    from roreg_amd import hip
    S, T = C.make(family, F, m, n, k, 'knn')
    od, oi = oracle(family, F, m, n, k, 'knn', squared)
    s, t = cu(S), cu(T)
    idx, d = hip.knn_search(s, t, k, want_dist=True, squared=squared)
    assert idx.shape == (m, k) and d.shape == (m, k)
    assert_same(idx, d, oi, od, (family, F, m, n, k, squared))
    assert torch.equal(hip.knn_search(s, t, k, squared=squared), idx)
    if family == 'lattice' and k == 5:                                                       # more targets tie at the 5th place than the list holds
        D = O.pdist(S, T, dist_type(squared))
        assert ((D == od.reshape(m, k)[:, 4:5]).sum(1) > 5).sum() >= 5


# ---- 3. knn_search_seg ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 5, 8])
@pytest.mark.parametrize('F', [3, 32])
def test_knn_search_segmented_equals_the_oracle_per_cloud(F, k):
    from roreg_amd import hip
    sizes, clouds = C.seg_clouds(F, k)
    got = hip.knn_search_seg(cu(np.concatenate(clouds)), hip.Segments(sizes), k).cpu().numpy()
    assert got.shape == (sum(sizes), k) and got.dtype == np.int64
    o = 0
    for q, c in enumerate(clouds):
        want = O.knn(c, c, k)[1].reshape(len(c), k)
        wrong = got[o:o + len(c)] != want
        assert not wrong.any(), (F, k, q, len(c), int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
        o += len(c)
    big = clouds[1]                                                                          # a one-segment call is knn_search
    one = hip.knn_search_seg(cu(big), hip.Segments([len(big)]), k)
    assert torch.equal(one, hip.knn_search(cu(big), cu(big), k)) and np.array_equal(one.cpu().numpy(), O.knn(big, big, k)[1].reshape(len(big), k))


# ---- 4. pdist ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('F', [3, 32] + list(C.GENERIC_FS))
def test_pdist_has_the_oracles_bits_at_ragged_shapes(F, squared):
    from roreg_amd import hip
    for m in C.PDIST_MS:
        for n in C.PDIST_NS:
            S, T = C.randn(F, m, n, seed=1)
            got = hip.pdist(cu(S), cu(T), squared=squared).cpu().numpy()
            want = O.pdist(S, T, dist_type(squared))
            assert got.shape == (m, n) and np.array_equal(bits(got), bits(want)), (F, m, n, squared)
    S, T = C.make('root_ties', F, 5, 65) if F >= 3 else C.randn(F, 5, 65)
    assert np.array_equal(bits(hip.pdist(cu(S), cu(T), squared=squared).cpu().numpy()), bits(O.pdist(S, T, dist_type(squared))))


# ---- 5. mutual_matches on indices no search set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('samples', [False, True])
@pytest.mark.parametrize('m', C.MUTUAL_MS)
def test_mutual_matches_skips_indices_out_of_range(m, samples):
    """nn01 / nn10 hold -1, the other side's length and 4294967295 among valid entries: such a source is unmatched.  (The kernel compares an
    entry with the range before it uses it; nothing here is an index into anything.)"""
    from roreg_amd import hip
    n = m - 7
    nn01, nn10 = C.mutual_inputs(m, n)
    want = C.mutual_in_range(nn01, nn10)
    s0 = s1 = None
    if samples:
        rng = np.random.default_rng(m)
        s0, s1 = rng.permutation(m + 10)[:m], rng.permutation(n + 10)[:n]
        want = np.stack([s0[want[:, 0]], s1[want[:, 1]]], 1)
    out, cnt = hip.mutual_matches(cu(nn01), cu(nn10), cu(s0), cu(s1))
    c = int(cnt.item())
    got = out[:c].cpu().numpy()
    assert c == want.shape[0] and np.array_equal(got, want)
    if not samples:
        assert (np.diff(got[:, 0]) > 0).all() and len(set(got[:, 0] // 1024)) >= max(1, m // 1024)       # increasing, across the passes


# ---- 6. the batched matcher on the tie families -----------------------------------------------------------------------------------------------
# (the small root_ties shapes straddle the matcher's 128 tile edge -- a lone pad row or column decides -- or have a one-row side)
@pytest.mark.parametrize('family,m,n', [('root_ties', 257, 300), ('lattice', 559, 343), ('root_ties', 127, 129), ('root_ties', 128, 128),
                                        ('root_ties', 129, 127), ('root_ties', 1, 300), ('root_ties', 300, 1)])
def test_mutual_match_batch_on_tie_families_equals_the_oracle(family, m, n):
    from roreg_amd import hip
    A, B = C.make(family, 32, m, n)
    mbuf, cnt = hip.mutual_match_batch([(cu(A), cu(B), None, None), (cu(B), cu(A), None, None)])
    cnt = cnt.cpu().numpy(); mbuf = mbuf.cpu().numpy()
    for q, (S, T) in enumerate(((A, B), (B, A))):
        want = O.mutual_check(O.knn(T, S, 1)[1], O.knn(S, T, 1)[1])
        print(f'mutual_match_batch {family} direction {q}: {cnt[q]} matches on the device, {want.shape[0]} in the oracle')
        assert cnt[q] == want.shape[0] and np.array_equal(mbuf[q, :cnt[q]], want), (family, q)


# ---- 7. non-finite distances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('finite', ['third', 'two'])
@pytest.mark.parametrize('F,m,n', C.OVERFLOW_NN)
def test_nn_search_rows_of_infinite_distances_answer_index_0(F, m, n, finite, squared):
    from roreg_amd import hip
    S, T = C.overflow(F, m, n, finite)
    with np.errstate(over='ignore'):
        od, oi = O.knn(T, S, 1, dist_type=dist_type(squared))
    all_inf = np.zeros(m, bool); all_inf[0::4] = True
    assert (oi[all_inf] == 0).all() and np.isinf(od[all_inf]).all() and np.isfinite(od[~all_inf]).all()
    idx, d = hip.nn_search(cu(S), cu(T), want_dist=True, squared=squared)
    assert_same(idx, d, oi, od, (F, m, n, finite, squared))


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('finite', ['third', 'two'])
@pytest.mark.parametrize('F,m,n,k', C.OVERFLOW_KNN)
def test_knn_search_rows_of_infinite_distances_list_the_first_indices(F, m, n, k, finite, squared):
    from roreg_amd import hip
    S, T = C.overflow(F, m, n, finite)
    with np.errstate(over='ignore'):
        od, oi = O.knn(T, S, k, dist_type=dist_type(squared))
    od, oi = od.reshape(m, k), oi.reshape(m, k)
    assert (oi[0::4] == np.arange(k)).all() and np.isinf(od[0::4]).all() and np.isfinite(od[1::4, 0]).all()
    idx, d = hip.knn_search(cu(S), cu(T), k, want_dist=True, squared=squared)
    assert_same(idx, d, oi, od, (F, m, n, k, finite, squared))


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('F', [3, 7, 32])
def test_pdist_overflow_and_nan_where_the_oracle_has_them(F, squared):
    from roreg_amd import hip
    for S, T in (C.overflow(F, 9, 65, 'third'), C.nan(F, 6, 65)):
        with np.errstate(over='ignore'):
            want = O.pdist(S, T, dist_type(squared))
        got = hip.pdist(cu(S), cu(T), squared=squared).cpu().numpy()
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
        assert np.isinf(want).any() or nan.any()


def _without_nan_rows(S, T, k, squared):
    """The oracle on the rows no NaN touches: the NaN target taken out (indices above it shifted back), the NaN source row masked."""
    keep_t = np.arange(T.shape[0]) != C.NAN_TARGET_ROW
    od, oi = O.knn(T[keep_t], S, k, dist_type=dist_type(squared))
    oi = np.where(oi >= C.NAN_TARGET_ROW, oi + 1, oi)
    rows = np.arange(S.shape[0]) != C.NAN_SOURCE_ROW
    return od.reshape(S.shape[0], k), oi.reshape(S.shape[0], k), rows


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('F,m,n', [(3, 257, 300), (32, 257, 300), (3, 5, 4100), (7, 257, 40)])
def test_nn_search_nan_never_enters(F, m, n, squared):
    """A NaN distance is never admitted: the NaN target is passed over, the NaN source row has no comparable distance and gets an index
    outside [0, n) (which mutual_matches treats as unmatched); every other row is the oracle's on the remaining targets."""
    from roreg_amd import hip
    S, T = C.nan(F, m, n)
    od, oi, rows = _without_nan_rows(S, T, 1, squared)
    idx, d = hip.nn_search(cu(S), cu(T), want_dist=True, squared=squared)
    idx, d = idx.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(idx[rows], oi[rows, 0]) and np.array_equal(bits(d[rows]), bits(od[rows, 0]))
    assert not 0 <= idx[C.NAN_SOURCE_ROW] < n


@pytest.mark.parametrize('squared', [False, True])
@pytest.mark.parametrize('F,m,n,k', [(3, 257, 100, 5), (32, 257, 100, 8), (3, 5, 32, 5), (32, 5, 32, 1), (7, 257, 40, 9), (3, 257, 33, 2)])
def test_knn_search_nan_never_enters(F, m, n, k, squared):
    from roreg_amd import hip
    S, T = C.nan(F, m, n)
    od, oi, rows = _without_nan_rows(S, T, k, squared)
    idx, d = hip.knn_search(cu(S), cu(T), k, want_dist=True, squared=squared)
    idx, d = idx.cpu().numpy(), d.cpu().numpy()
    assert np.array_equal(idx[rows], oi[rows]) and np.array_equal(bits(d[rows]), bits(od[rows]))
    assert (idx[C.NAN_SOURCE_ROW] == -1).all()
