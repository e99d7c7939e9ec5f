"""The families of tests/_fpfh_match_cases.py have the properties they are named for (CPU only; oracle.ref_numpy.knn(.., 1) is the definition)."""
import numpy as np
import pytest

import _fpfh_match_cases as M
from oracle import ref_numpy as O


@pytest.mark.parametrize('name', sorted(M.FAMILIES))
def test_families_are_fpfh_like(name):
    for a in M.family(name):
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 33 and a.flags.c_contiguous
        assert np.isfinite(a).all() and (a >= 0).all()
        sums = a.astype(np.float64).reshape(a.shape[0], 3, 11).sum(2)
        assert (((sums > 199.5) & (sums < 203.5)) | (sums == 0.0)).all()      # (a perturbed row exceeds 200 by its perturbation, 3 at most; zero rows)


def test_sqrt_collapse_family_has_winners_decided_by_equal_roots():
    s, t = M.family('collapse')
    d, nn, _ = M.oracle('collapse')
    x = M.radicand(s, t)
    D = O.pdist(s, t)
    rows = 0
    for i in range(s.shape[0]):
        second = np.argsort(D[i], kind='stable')[1]
        # the two best: different radicands, the winner's the greater, one root -- the first index wins only through the tie
        if D[i, second] == d[i] and x[i, nn[i]] > x[i, second] and nn[i] < second:
            rows += 1
    assert nn.tolist() != x.argmin(1).tolist()
    assert rows >= 10, rows
    assert (np.abs(d - 100.0) < 3.0).all()


def test_duplicate_families_really_tie():
    T = M.TILE
    s, t = M.family('all_one_row')
    d, nn, nn10 = M.oracle('all_one_row')
    assert (t == t[0]).all() and not nn.any() and t.shape[0] > 2 * T
    for side, name in ((1, 'boundary_dup_side1'), (0, 'boundary_dup_side0')):
        s, t = M.family(name)
        d, nn, nn10 = M.oracle(name)
        if side == 1:
            assert np.array_equal(t[T - 1], t[T]) and nn[5] == T - 1 and O.pdist(s[5:6], t)[0, T] == d[5]
        else:
            assert np.array_equal(s[T - 1], s[T]) and nn10[7] == T - 1
    s, t = M.family('boundary_dup_side2')
    d, nn, nn10 = M.oracle('boundary_dup_side2')
    assert nn[5] == T - 1 and nn10[7] == T - 1
    s, t = M.family('identical')
    d, nn, nn10 = M.oracle('identical')
    assert np.array_equal(s, t) and nn[T + 3] == 11 and nn10[T + 3] == 11 and (nn[:T] == np.arange(T)).all()


@pytest.mark.parametrize('channel', M.NEAR_CHANNELS)
def test_near_duplicates_are_won_by_the_smallest_move(channel):
    s, t = M.family(f'near_ch{channel}')
    d, nn, _ = M.oracle(f'near_ch{channel}')
    D = O.pdist(s, t)
    for i in range(s.shape[0]):
        four = D[i, 4 * i:4 * i + 4]
        assert nn[i] // 4 == i and (np.diff(four) <= 0).all() and four[0] > four[3]
        assert nn[i] == 4 * i + int(np.argmin(four))             # (the one-ulp and 1e-5 copies may share the root 1e-7 ** 0.5: the first of them)


def test_channel_32_alone_decides_its_family():
    s, t = M.family('channel32')
    _, nn, _ = M.oracle('channel32')
    _, nn_without = O.knn(t[:, :32], s[:, :32], 1)
    assert (nn == 3 * np.arange(60) + 1).all() and (nn_without == 3 * np.arange(60)).all()
    s, t = M.family('near_ch32')
    _, nn, _ = M.oracle('near_ch32')
    _, nn_without = O.knn(t[:, :32], s[:, :32], 1)
    assert (nn != nn_without).all()


def test_large_norm_family_has_several_targets_within_the_margin():
    s, t = M.family('large_norm')
    n2 = (s.astype(np.float64) ** 2).sum(1)
    assert (np.abs(n2 - 1.2e5) < 100).all()
    sep = np.sqrt(((s[:, None, :].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(-1))
    assert 0.005 < sep.min() < 0.03 and sep.max() < 0.06
    counts = M.rows_with_several_targets_within_the_margin(s, t)
    assert (counts > 1).sum() >= 100, counts
    # random rows, by contrast, mostly keep a single candidate
    s, t = M.random_case(257, 255)
    assert np.median(M.rows_with_several_targets_within_the_margin(s, t)) <= 2


def test_zero_families_hold_zero_rows():
    assert not M.family('zero_1')[1].any()
    s, t = M.family('zero_2')
    assert (~s.any(1)).sum() > 10 and (~t.any(1)).sum() > 10 and s.any(1).sum() > 100
