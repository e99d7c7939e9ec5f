"""CPU only: the families of tests/_knn_cases.py meet the conditions they are named for, shown with the oracle alone (oracle/ref_numpy.py), so
that a pass of tests/test_hip_knn.py on the device means something.  The bars are caps fixed beforehand, each test prints what it measured."""
import numpy as np
import pytest
import torch

import _knn_cases as C
from oracle import ref_numpy as O

f32, f64 = np.float32, np.float64
DT = ('L2', 'SquareL2')


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the restated slice geometry ----------------------------------------------------------------------------------------------------------
def test_slice_geometry_matches_examples_worked_by_hand_from_the_host_code():
    # roreg_nn_search_ex: gx = ceil(m/256); slices = min(ceil(2048/gx), n); slice = ceil(n/slices); grid.y = ceil(n/slice)
    assert C.nn_geometry(256, 300) == (1, 300)            # gx 1: 2048 -> 300 slices of one target
    assert C.nn_geometry(256, 4100) == (3, 1367)          # 2048 slices: ceil(4100/2048) = 3 per slice, 1366 full slices + one of 2
    assert C.nn_geometry(2305, 500) == (3, 167)           # gx 10: ceil(2048/10) = 205 slices: ceil(500/205) = 3, 166 full slices + one of 2
    assert 4100 - 1366 * 3 == 2 and 500 - 166 * 3 == 2
    # knn_slices: min(ceil(512/gx), ceil(n/32)), at least 1; roreg_knn_search_ex: slice = ceil(n/slices), grid.y = ceil(n/slice)
    assert C.knn_geometry(255, 32) == (32, 1) and C.knn_slices(255, 32) == 1         # the single-pass kernel
    assert C.knn_geometry(257, 33) == (17, 2)             # gx 2: min(256, 2) = 2 slices: 17 + 16
    assert C.knn_geometry(257, 1000) == (32, 32)          # min(256, 32) = 32 slices of ceil(1000/32) = 32: 31 full + one of 8
    assert C.knn_geometry(5000, 5000) == (193, 26)        # gx 20: min(26, 157) = 26 slices of ceil(5000/26) = 193: 25 full + one of 175
    # roreg_knn_search_seg: grid.y = min(ceil(2048/(gx n_seg)), ceil(max/32)) from the largest cloud; each cloud: slice = ceil(n/grid.y)
    sizes = C.seg_sizes(5)
    assert len(sizes) == 11 and max(sizes) == 1000        # gx 4: min(ceil(2048/44) = 47, 32) = 32
    assert C.seg_geometry(sizes, 1000) == (32, 32) and C.seg_geometry(sizes, 257) == (9, 29) and C.seg_geometry(sizes, 33) == (2, 17)
    assert C.seg_geometry(sizes, 5) == (1, 5)
    assert sizes[0] == sizes[-1] == min(sizes) and sizes[1] == sizes[-2] == max(sizes)
    # the sizes the tables name reach what they are named for
    assert {C.knn_geometry(m, n)[1] for _, _, m, n, k in C.KNN_CASES if n <= 32} == {1}
    assert {C.knn_geometry(m, 33) for m in C.KNN_MS} == {(17, 2)} and C.knn_geometry(255, 100) == (25, 4)
    assert all(C.nn_geometry(m, n)[0] == 1 for m, n in C.NN_SIZES if n <= 300)


# ---- root ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [3, 32])
def test_root_ties_make_the_two_distance_types_disagree(F):
    S, T = C.make('root_ties', F, 257, 300)
    (d1, i1), (d2, i2) = (O.knn(T, S, 1, dist_type=dt) for dt in DT)
    (_, j1), (_, j2) = (O.knn(T, S, 5, dist_type=dt) for dt in DT)
    rows = np.where(i1 != i2)[0]
    lists = int((j1 != j2).any(1).sum())
    print(f'root_ties F={F} m=257 n=300: {len(rows)} nearest neighbours and {lists} k=5 lists differ between L2 and SquareL2')
    assert len(rows) >= 8 and lists >= 129
    D, X = O.pdist(S, T, 'L2'), O.pdist(S, T, 'SquareL2')
    assert np.array_equal(bits(D[rows, i1[rows]]), bits(D[rows, i2[rows]]))          # the roots are the same float ...
    assert (bits(X[rows, i1[rows]]) != bits(X[rows, i2[rows]])).all()                # ... of different radicands
    assert (i1[rows] < i2[rows]).all() and (X[rows, i1[rows]] > X[rows, i2[rows]]).all()   # L2: the earlier index although its radicand is larger
    # the lists: the same multiset of roots either way
    assert np.array_equal(bits(np.take_along_axis(D, j1, 1)), bits(np.sort(np.take_along_axis(D, j2, 1), 1)))


def test_every_root_tie_case_of_the_tables_has_disagreeing_rows():
    for family, F, m, n in C.NN_CASES:
        if family == 'root_ties':
            S, T = C.make(family, F, m, n)
            differ = int((O.knn(T, S, 1)[1] != O.knn(T, S, 1, dist_type='SquareL2')[1]).sum())
            print(f'root_ties nn F={F} m={m} n={n}: {differ} rows differ')
            assert differ >= 8, (F, m, n, differ)
    for family, F, m, n, k in C.KNN_CASES + C.KNN_GENERIC_CASES:
        if family == 'root_ties':
            S, T = C.make(family, F, m, n, k, 'knn')
            differ = int((O.knn(T, S, k)[1] != O.knn(T, S, k, dist_type='SquareL2')[1]).any(1).sum())
            print(f'root_ties knn F={F} m={m} n={n} k={k}: {differ} lists differ')
            assert differ >= 8, (F, m, n, k, differ)


def test_shrinking_shells_put_an_equal_root_before_the_smallest_radicand_inside_its_slice():
    """What a 'SquareL2' scan that compared roots would get wrong: with one target per slice, or the rivals in other slices, the merge by
    radicand bits repairs it."""
    for family, F, m, n in C.NN_CASES:
        if family != 'root_shrink':
            continue
        S, T = C.make(family, F, m, n)
        per, slices = C.nn_geometry(m, n)
        assert per == 3
        D, X = O.pdist(S, T, 'L2'), O.pdist(S, T, 'SquareL2')
        win = O.knn(T, S, 1, dist_type='SquareL2')[1]
        start = win // per * per
        rows = [i for i in range(m) if (bits(D[i, start[i]:win[i]]) == bits(D[i, win[i]])).any()]
        differ = int((O.knn(T, S, 1)[1] != win).sum())
        print(f'root_shrink F={F} m={m} n={n}: {len(rows)} rows with an equal root earlier in the winner\'s slice, {differ} rows where L2 and SquareL2 differ')
        assert len(rows) >= 4 and differ >= 8 and all(X[i, start[i]:win[i]].min() > X[i, win[i]] for i in rows)


# ---- lattice ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [3, 7, 32])
def test_lattice_ties_are_exact_and_outnumber_the_list(F):
    S, T = C.lattice(F)
    assert S.shape == (559, F) and T.shape == (343, F) and len(np.unique(T, axis=0)) == 343          # distinct targets
    for dt in DT:
        D = O.pdist(S, T, dt)
        Ds = np.sort(D, 1)
        equal_2_to_7 = int((bits(Ds[:, 1:7]) == bits(Ds[:, 1:2])).all(1).sum())
        at_kth = (D == Ds[:, 4:5]).sum(1)                                                            # targets tied with the 5th place
        print(f'lattice F={F} {dt}: {equal_2_to_7} rows with the 2nd..7th distance bit-equal, {int((at_kth > 5).sum())} rows with more than 5 targets tied at the 5th place')
        assert equal_2_to_7 >= 100 and (at_kth > 5).sum() >= 20
    # every sum is exact: small multiples of 1/4
    assert np.array_equal(O.pdist(S, T, 'SquareL2'), ((S.astype(f64)[:, None] - T.astype(f64)[None]) ** 2).sum(-1))
    Ss, Ts = C.lattice(F, None, 3)                                                                   # 27 targets: the single-pass kernel
    Dk = np.sort(O.pdist(Ss, Ts), 1)
    assert Ts.shape[0] == 27 and ((O.pdist(Ss, Ts) == Dk[:, 4:5]).sum(1) > 5).sum() >= 5


# ---- duplicates ---------------------------------------------------------------------------------------------------------------------------
def _duplicate_cases():
    out = [(F, m, n, 1, 'nn') for fam, F, m, n in C.NN_CASES if fam == 'duplicates']
    out += [(F, m, n, k, 'knn') for fam, F, m, n, k in C.KNN_CASES + C.KNN_GENERIC_CASES if fam == 'duplicates']
    return out


@pytest.mark.parametrize('F,m,n,k,form', _duplicate_cases())
def test_duplicates_sit_in_the_slices_claimed(F, m, n, k, form):
    per, slices = (C.nn_geometry if form == 'nn' else C.knn_geometry)(m, n)
    S, T, plan, aimed = C.duplicates(F, m, n, k, per, slices)
    assert np.array_equal(C.make('duplicates', F, m, n, k, form)[1], T)
    assert 'group' in plan and (slices < 2 or {'boundary', 'ends'} <= set(plan)) and (per < 3 or 'inside' in plan), plan
    d, i = O.knn(T, S, max(k, 2))
    for name, entry in plan.items():
        rows = aimed[name]
        assert len(rows) >= 1
        if name == 'group':
            first, g, closer = entry
            assert g == k + 3 and closer >= first + g and (bits(T[first:first + g]) == bits(T[first])).all()
            D = O.pdist(S[rows], T)
            assert (D[:, closer] < D[:, first]).all()                                               # the later row really is closer
            want = ([closer] + list(range(first, first + g)))[:max(k, 2)]
            assert (i[rows] == want).all(), (name, i[rows][0], want)
            continue
        a, b = entry
        assert a < b and np.array_equal(bits(T[a]), bits(T[b]))
        sa, sb = C.slice_of(a, per), C.slice_of(b, per)
        if name == 'inside':
            assert sa == sb
        elif name == 'boundary':
            assert sb == sa + 1 and (a + 1) % per == 0 and b % per == 0                             # last element of s, first of s + 1
        else:
            assert (a, b) == (0, n - 1) and sa == 0 and sb == slices - 1
        assert (i[rows, 0] == a).all() and (i[rows, 1] == b).all() and np.array_equal(bits(d[rows, 0]), bits(d[rows, 1]))


def test_segmented_clouds_hold_a_lattice_and_duplicates_across_a_slice_boundary():
    for F in (3, 32):
        for k in (1, 5, 8):
            sizes, clouds = C.seg_clouds(F, k)
            assert [c.shape for c in clouds] == [(n, F) for n in sizes]
            per, slices = C.seg_geometry(sizes, 257)
            plan = C.duplicate_plan(per, slices, 257, k)
            a, b = plan['boundary']
            c = clouds[sizes.index(257)]
            assert np.array_equal(c[a], c[b]) and C.slice_of(b, per) == C.slice_of(a, per) + 1 and 'group' in plan
            assert np.array_equal(clouds[sizes.index(343)], C.lattice(F)[1])


# ---- non-finite distances -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('finite', ['third', 'two'])
@pytest.mark.parametrize('F', [3, 7, 32])
def test_overflow_rows_are_all_inf_and_the_oracle_and_torch_answer_index_0(F, finite):
    m, n, k = 9, 40, 5
    S, T = C.overflow(F, m, n, finite)
    for dt in DT:
        with np.errstate(over='ignore'):
            D = O.pdist(S, T, dt)
            d1, i1 = O.knn(T, S, 1, dist_type=dt)
            dk, ik = O.knn(T, S, k, dist_type=dt)
        assert not np.isnan(D).any()
        all_inf = np.isinf(D).all(1)
        assert np.array_equal(np.where(all_inf)[0], np.arange(0, m, 4))
        assert (i1[all_inf] == 0).all() and (ik[all_inf] == np.arange(k)).all() and np.isinf(d1[all_inf]).all() and np.isinf(dk[all_inf]).all()
        # torch on the same matrix, ties resolved by index: the first position of the minimum; a stable sort's first k
        Dt = torch.from_numpy(D)
        v = Dt.min(1).values
        first = (Dt == v[:, None]).to(torch.int8).argmax(1)
        assert np.array_equal(first.numpy(), i1) and np.array_equal(bits(v.numpy()), bits(d1))
        sv, si = torch.sort(Dt, dim=1, stable=True)
        assert np.array_equal(si[:, :k].numpy(), ik) and np.array_equal(bits(torch.topk(Dt, k, dim=1, largest=False).values.numpy()), bits(dk))
        # the mixed rows: the winner is one of the finite targets
        finite_t = np.where(np.isfinite(T).all(1) & (np.abs(T) < 1e10).all(1))[0]
        assert len(finite_t) == (n // 3 if finite == 'third' else 2) and 0 not in finite_t
        assert np.isfinite(d1[~all_inf]).all() and np.isin(i1[~all_inf], finite_t).all()
        if finite == 'two':                                                                          # two finite entries, then +inf in index order
            assert np.isfinite(dk[~all_inf, :2]).all() and np.isinf(dk[~all_inf, 2:]).all() and (ik[~all_inf, 2:] == [0, 1, 2]).all()


def test_overflow_shapes_of_the_device_tests_have_exactly_every_fourth_row_all_inf():
    for F, m, n in list(C.OVERFLOW_NN) + [c[:3] for c in C.OVERFLOW_KNN]:
        for finite in ('third', 'two'):
            S, T = C.overflow(F, m, n, finite)
            with np.errstate(over='ignore'):
                D = O.pdist(S, T, 'SquareL2')
            want = np.zeros(m, bool); want[0::4] = True
            assert not np.isnan(D).any() and np.array_equal(np.isinf(D).all(1), want) and np.isfinite(D[~want]).any(1).all(), (F, m, n, finite)


def test_nan_family_has_nan_in_one_row_and_one_column_only():
    for F in (3, 7, 32):
        S, T = C.nan(F, 6, 9)
        D = O.pdist(S, T)
        want = np.zeros(D.shape, bool)
        want[C.NAN_SOURCE_ROW] = True; want[:, C.NAN_TARGET_ROW] = True
        assert np.array_equal(np.isnan(D), want)


# ---- ordinary data: the oracle against float64 ----------------------------------------------------------------------------------------------
def test_oracle_equals_a_float64_brute_force_where_float64_separates_the_neighbours():
    cases = [(F, m, n, 1) for fam, F, m, n in C.NN_CASES if fam == 'randn']
    cases += [(F, m, n, k) for fam, F, m, n, k in C.KNN_CASES + C.KNN_GENERIC_CASES if fam == 'randn']
    excused = compared = 0
    for F, m, n, k in cases:
        S, T = C.randn(F, m, n)
        for dt in DT:
            d, i = O.knn(T, S, k, dist_type=dt)
            i = i.reshape(m, k)
            X = ((S.astype(f64)[:, None, :] - T.astype(f64)[None, :, :]) ** 2).sum(-1)
            D64 = X if dt == 'SquareL2' else np.sqrt(X + 1e-7)
            order = np.argsort(D64, 1, kind='stable')
            top = np.take_along_axis(D64, order[:, :k + 1], 1)
            close = (np.diff(top, axis=1) <= 1e-6 * top[:, 1:]).any(1)                               # two of the best k + 1 within 1e-6 relative
            assert np.array_equal(i[~close], order[~close, :k]), (F, m, n, k, dt)
            assert np.abs(d.reshape(m, k) - np.take_along_axis(D64, i, 1)).max() <= 4e-6 * max(1.0, D64.max())
            excused += int(close.sum()); compared += int((~close).sum())
    print(f'oracle vs float64: {compared} rows compared, {excused} excused as float64 near-ties')
    assert excused <= compared // 20


# ---- mutual check inputs ------------------------------------------------------------------------------------------------------------------
def test_mutual_inputs_hold_every_unset_value_and_the_restricted_check_is_the_oracles_on_valid_input():
    for m in C.MUTUAL_MS:
        n = m - 7
        nn01, nn10 = C.mutual_inputs(m, n)
        for arr, other in ((nn01, n), (nn10, m)):
            assert {-1, other, 4294967295} <= set(arr.tolist()) and ((arr >= 0) & (arr < other)).sum() >= len(arr) // 2
        want = C.mutual_in_range(nn01, nn10)
        assert len(want) >= m // 8 and (np.diff(want[:, 0]) > 0).all()
        ok = (nn01 >= 0) & (nn01 < n)
        clean01 = np.where(ok, nn01, 0)
        full = O.mutual_check(clean01, nn10)                                                         # the oracle, fed index 0 in place of the unset ones
        assert np.array_equal(want, full[ok[full[:, 0]]])
