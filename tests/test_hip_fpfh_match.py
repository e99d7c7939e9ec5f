"""The FPFH matcher (csrc/fpfh_match.hip, "v6o") on the device: every result bit for bit that of hip.nn_search (both
directions) + hip.mutual_matches, which tests/test_hip_knn.py pins to the oracle at their edges; cases of a few hundred rows also against
oracle.ref_numpy.knn directly.  The families are those of tests/_fpfh_match_cases.py (tests/test_fpfh_match_cases.py checks their properties on
the CPU)."""
import numpy as np
import pytest
import torch

import _fpfh_cases as K
import _fpfh_match_cases as M
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

T = M.TILE


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scan(d0, d1, r0=None, r1=None):
    """today's composition: (matches [count,2], count, nn01, dist01, nn10)"""
    from roreg_amd import hip
    nn01, dist = hip.nn_search(d0, d1, src_rows=r0, tgt_rows=r1, want_dist=True)
    nn10 = hip.nn_search(d1, d0, src_rows=r1, tgt_rows=r0)
    out, cnt = hip.mutual_matches(nn01, nn10, sample0=r0, sample1=r1)
    return out[:int(cnt)], int(cnt), nn01, dist, nn10


def _same(got, want, what=''):
    matches, count, nn01, dist01, nn10 = got[:5]
    assert tuple(count.shape) == (1,) and count.dtype == torch.int32 and int(count) == want[1], (what, int(count), want[1])
    assert nn01.dtype == torch.int64 and nn10.dtype == torch.int64 and dist01.dtype == torch.float32 and matches.dtype == torch.int64
    assert torch.equal(nn01, want[2]), what
    assert torch.equal(dist01.view(torch.int32), want[3].view(torch.int32)), what
    assert torch.equal(nn10, want[4]), what
    assert tuple(matches.shape) == (min(nn01.shape[0], nn10.shape[0]), 2) and torch.equal(matches[:want[1]], want[0]), what


def _check(s, t, what='', oracle=None):
    from roreg_amd import hip
    d0, d1 = _cuda(s), _cuda(t)
    got = hip.fpfh_match(d0, d1)
    _same(got, _scan(d0, d1), what)
    if oracle is not None:
        d01, nn01, nn10 = oracle
        assert np.array_equal(got[2].cpu().numpy(), nn01) and np.array_equal(got[4].cpu().numpy(), nn10), what
        assert np.array_equal(got[3].cpu().numpy().view(np.int32), d01.view(np.int32)), what
    return got


@pytest.mark.parametrize('shape', M.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_shapes_equal_the_scan_and_the_oracle(shape):
    s, t = M.random_case(*shape)
    oracle = None
    if max(shape) <= 300:
        d01, nn01 = O.knn(t, s, 1)
        oracle = (d01, nn01, O.knn(s, t, 1)[1])
    _check(s, t, str(shape), oracle)


@pytest.mark.parametrize('name', sorted(M.FAMILIES))
def test_families_equal_the_scan_and_the_oracle(name):
    s, t = M.family(name)
    got = _check(s, t, name, M.oracle(name))
    if name == 'all_one_row':
        assert not got[2].any()
    if name == 'channel32':
        assert torch.equal(got[2].cpu(), 3 * torch.arange(60) + 1)


def test_row_lists_with_every_unselected_row_nan():
    """Sorted lists with gaps; every row the lists leave out is NaN: the results are those of the compacted tables, mapped through the lists."""
    from roreg_amd import hip
    rng = np.random.default_rng(0x7015)
    for (n0, m0), (n1, m1) in (((400, 2 * T + 1), (350, T - 1)), ((300, 1), (300, 200)), ((5 * T, 3 * T), (4 * T, 2 * T))):
        s, t = M.random_case(m0, m1)
        r0, r1 = np.sort(rng.choice(n0, m0, replace=False)), np.sort(rng.choice(n1, m1, replace=False))
        big0, big1 = np.full((n0, 33), np.nan, np.float32), np.full((n1, 33), np.nan, np.float32)
        big0[r0], big1[r1] = s, t
        d0, d1, q0, q1 = _cuda(big0), _cuda(big1), _cuda(r0), _cuda(r1)
        got = hip.fpfh_match(d0, d1, q0, q1)
        _same(got, _scan(d0, d1, q0, q1), 'lists')
        compact = hip.fpfh_match(_cuda(s), _cuda(t))
        assert torch.equal(got[2], compact[2]) and torch.equal(got[3].view(torch.int32), compact[3].view(torch.int32)) and torch.equal(got[4], compact[4])
        c = int(got[1])
        assert c == int(compact[1]) and torch.equal(got[0][:c, 0], q0[compact[0][:c, 0]]) and torch.equal(got[0][:c, 1], q1[compact[0][:c, 1]])
        # a list on one side only
        _same(hip.fpfh_match(d0, _cuda(t), q0, None), _scan(d0, _cuda(t), q0, None), 'one list')


DEBUG_CASES = [('random', sh) for sh in M.SHAPES if max(sh) <= 2 * T + 1] + [('family', n) for n in sorted(M.FAMILIES)]


def _debug_case(kind, arg):
    """-> the greatest |a - x| / delta of the case, after checking the bound, the candidates and the guards"""
    from roreg_amd import hip
    s, t = M.random_case(*arg) if kind == 'random' else M.family(arg)
    got = hip.fpfh_match(_cuda(s), _cuda(t), debug=True)
    dbg = got[5]
    assert dbg['guards_ok'], arg
    _same(got, _scan(_cuda(s), _cuda(t)), str(arg))
    S, Tt = s.astype(np.float64), t.astype(np.float64)
    x = ((S[:, None, :] - Tt[None, :, :]) ** 2).sum(-1)
    N0, N1 = (S * S).sum(1), (Tt * Tt).sum(1)
    delta = hip.fpfh_match_delta(N0[:, None], N1[None, :])
    a = dbg['a'].astype(np.float64)
    assert a.shape == x.shape and np.isfinite(a).all()
    err = np.abs(a - x)
    assert (err <= delta).all(), (arg, float((err / np.maximum(delta, 1e-300)).max()))
    ratio = float((err[delta > 0] / delta[delta > 0]).max()) if (delta > 0).any() else 0.0
    # pass A's minima are entries of a matrix that obeys the same bound (the transposed product for the rows)
    assert (np.abs(dbg['amin0'] - x.min(1)) <= delta.max(1)).all() and (np.abs(dbg['amin1'] - x.min(0)) <= delta.max(0)).all(), arg
    assert (dbg['cnt0'] >= 1).all() and (dbg['cnt1'] >= 1).all(), arg
    assert (dbg['cnt0'] <= t.shape[0]).all() and (dbg['cnt1'] <= s.shape[0]).all()
    # the exact winner was a candidate, by the derivation's own inequality (the margin without its safety factor)
    nn01, nn10 = got[2].cpu().numpy(), got[4].cpu().numpy()
    m0 = hip.fpfh_match_margin(dbg['amin0'].astype(np.float64), N0, N1.max()) / hip.FPFH_MATCH_MARGIN_MULT
    m1 = hip.fpfh_match_margin(dbg['amin1'].astype(np.float64), N1, N0.max()) / hip.FPFH_MATCH_MARGIN_MULT
    assert (a[np.arange(s.shape[0]), nn01] <= dbg['amin0'] + m0).all(), arg
    assert (a[nn10, np.arange(t.shape[0])] <= dbg['amin1'] + m1).all(), arg
    return ratio, float(dbg['cnt0'].mean()), int(dbg['cnt0'].max())


def test_debug_bound_candidates_guards_and_the_worst_case_ratio():
    """|a - x| <= delta at every entry of every small case (x: the float64 radicand), every row and column has a candidate, the exact winners
    were candidates, the guards are intact.  The greatest |a - x| / delta over all cases is the safety ratio DESIGN.md 4.24 quotes."""
    worst = 0.0
    for kind, arg in DEBUG_CASES:
        ratio, mean, mx = _debug_case(kind, arg)
        print(f'{kind} {arg}: max |a - x| / delta = {ratio:.4f}; candidates per row: mean {mean:.2f}, max {mx}')
        worst = max(worst, ratio)
    print(f'worst |a - x| / delta over {len(DEBUG_CASES)} cases: {worst:.4f}')
    assert worst <= 1.0


def test_large_norm_family_keeps_many_candidates_and_random_rows_few():
    from roreg_amd import hip
    s, t = M.family('large_norm')
    dbg = hip.fpfh_match(_cuda(s), _cuda(t), debug=True)[5]
    assert (dbg['cnt0'] > 1).sum() >= 100                  # (the CPU test derives as much from the margin formula)
    s, t = M.random_case(2 * T + 1, 2 * T - 1)
    dbg = hip.fpfh_match(_cuda(s), _cuda(t), debug=True)[5]
    assert np.median(dbg['cnt0']) <= 2


def test_batch_equals_the_single_calls_in_either_order_and_under_a_small_cap():
    from roreg_amd import hip
    shapes = [(300, 1000), (T + 1, T - 1), (0, 50), (700, 2 * T), (33, 5)]
    tables = [M.random_case(max(a, 1), max(b, 1)) for a, b in shapes]
    tasks = [(_cuda(s[:a]), _cuda(t[:b]), None, None) for (s, t), (a, b) in zip(tables, shapes)]
    rows = _cuda(np.arange(0, 300, 2))
    tasks[0] = (tasks[0][0], tasks[0][1], rows, None)
    singles = [hip.fpfh_match(*task) for task in tasks]
    for k, (task, one) in enumerate(zip(tasks, singles)):
        if shapes[k][0] and shapes[k][1]:
            _same(one, _scan(*task), f'single {k}')
        else:
            assert int(one[1]) == 0 and all(int(x.shape[0]) == 0 for x in (one[0], one[2], one[3], one[4]))
    for order in (list(range(5)), list(range(5))[::-1]):
        for cap in (None, 100 << 10):                       # 100 KiB: the 1,300 padded rows of task 0 alone take 208 KB -- several groups
            got = hip.fpfh_match_batch([tasks[k] for k in order], workspace_cap=cap)
            for k, g in zip(order, got):
                one = singles[k]
                c = int(one[1])
                assert int(g[1]) == c and torch.equal(g[0][:c], one[0][:c]) and torch.equal(g[2], one[2]) and torch.equal(g[4], one[4])
                assert torch.equal(g[3].view(torch.int32), one[3].view(torch.int32))
    dbg = hip.fpfh_match_batch(tasks, debug=True, workspace_cap=100 << 10)
    assert all(d[5]['guards_ok'] for d in dbg) and 'a' in dbg[1][5] and 'a' not in dbg[0][5]
    assert hip.fpfh_match_batch([]) == []


def test_error_paths():
    from roreg_amd import hip
    ok = _cuda(np.zeros((4, 33), np.float32))
    for w in (32, 34):
        with pytest.raises(hip.HipError):
            hip.fpfh_match(_cuda(np.zeros((4, w), np.float32)), ok)
        with pytest.raises(hip.HipError):
            hip.fpfh_match(ok, _cuda(np.zeros((4, w), np.float32)))
    too_many = torch.zeros(hip.FPFH_MATCH_MAX_ROWS + 1, dtype=torch.int64, device='cuda')
    with pytest.raises(hip.HipError):
        hip.fpfh_match(ok, ok, too_many, None)
    with pytest.raises(hip.HipError):
        hip.fpfh_match(ok, ok, None, too_many)
    with pytest.raises(hip.HipError):
        hip.fpfh_match(ok.double(), ok)
    # the library refuses the same on its own
    rc = hip.lib().roreg_fpfh_match_batch(None, 1, hip.FPFH_MATCH_MAX_ROWS + 1, 4, 0, None, None, None, None, None, None, None, 0, None)
    assert rc != 0 and b'rows per side' in hip.lib().roreg_last_error()


@pytest.fixture(scope='module')
def terrain_descs():
    from roreg_amd import fpfh
    p0, p1, _ = K.terrain_pair(0)
    return fpfh.describe(p0, K.TERRAIN_R, voxel=K.TERRAIN_VOXEL), fpfh.describe(p1, K.TERRAIN_R, voxel=K.TERRAIN_VOXEL)


@pytest.mark.parametrize('max_matches', (None, 500))
def test_real_descriptors_match_equals_the_scan(terrain_descs, max_matches):
    from roreg_amd import fpfh
    d0, d1 = terrain_descs
    assert 4000 < int(d0.valid.sum()) < 8000 and 4000 < int(d1.valid.sum()) < 8000
    a, b = fpfh.match(d0, d1, max_matches, method='mfma'), fpfh.match(d0, d1, max_matches, method='scan')
    assert torch.equal(a, b) and (a.shape[0] == 500 if max_matches else a.shape[0] > 500)
    assert torch.equal(fpfh.match(d0, d1, max_matches), b)                       # 'auto'
    with pytest.raises(ValueError):
        fpfh.match(d0, d1, method='tree')


def test_register_and_register_scene_do_not_depend_on_the_matcher():
    from roreg_amd import fpfh
    p0, p1, _ = K.terrain_pair(0)
    one, scan = fpfh.register(p0, p1, voxel=K.TERRAIN_VOXEL, match_method='mfma'), fpfh.register(p0, p1, voxel=K.TERRAIN_VOXEL, match_method='scan')
    assert np.array_equal(one.matches, scan.matches) and one.trans.tobytes() == scan.trans.tobytes() and one.matches.shape[0] > 500
    clouds, pairs = [p0, p1, p0[::2].copy()], [(0, 1), (2, 1), (0, 2)]
    got, want = fpfh.register_scene(clouds, pairs, voxel=K.TERRAIN_VOXEL), fpfh.register_scene(clouds, pairs, voxel=K.TERRAIN_VOXEL, match_method='scan')
    for g, w in zip(got, want):
        assert np.array_equal(g.matches, w.matches) and g.trans.tobytes() == w.trans.tobytes()
    assert got[0].trans.tobytes() == one.trans.tobytes()
    assert fpfh.register_scene(clouds, [], voxel=K.TERRAIN_VOXEL) == []


def test_mid_size_pair_of_real_descriptors_equals_the_scan():
    """Two 40,000-point terrain views, at voxels 0.02 and 0.03 (about 23,000 x 14,000 rows): more than one tile column per wave quad in both
    directions, sides of different length, and the near-duplicate rows of real smooth surfaces."""
    from roreg_amd import fpfh, hip
    p0, p1, _ = K.terrain_pair(0)
    d0, d1 = fpfh.describe(p0, 0.125, voxel=0.02), fpfh.describe(p1, 0.125, voxel=0.03)
    r0, r1 = d0.valid.nonzero().reshape(-1).contiguous(), d1.valid.nonzero().reshape(-1).contiguous()
    assert 18000 < r0.shape[0] < 26000 and 10000 < r1.shape[0] < 16000
    got = hip.fpfh_match(d0.features, d1.features, r0, r1)
    _same(got, _scan(d0.features, d1.features, r0, r1), 'mid-size')
    dbg = hip.fpfh_match(d0.features, d1.features, r0[:512].contiguous(), r1[:512].contiguous(), debug=True)[5]
    print(f'mid-size pair {r0.shape[0]} x {r1.shape[0]}: {int(got[1])} mutual matches; candidates per row in a 512 x 512 sub-block: '
          f'mean {dbg["cnt0"].mean():.2f}, max {int(dbg["cnt0"].max())}; per column: mean {dbg["cnt1"].mean():.2f}, max {int(dbg["cnt1"].max())}')
    assert dbg['guards_ok'] and (dbg['cnt0'] >= 1).all() and (dbg['cnt1'] >= 1).all()
