"""CPU checks of the FPFH definition (tests/_fpfh_oracle.py), of the seeded families the GPU tests rely on (tests/_fpfh_cases.py) and of
csrc/fpfh_math.h on the host.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _fpfh_cases as K                # noqa: E402
import _fpfh_oracle as FO              # noqa: E402
import _icp_plane_cases as PC          # noqa: E402
import _sc2_oracle as SO               # noqa: E402


def test_vectorised_oracle_equals_the_loops():
    """300 points, a fifth of the normals zero, two duplicated rows: counts, m, the float32 features and their float64 values, every bit."""
    rng = np.random.default_rng(0x300)
    pts = rng.uniform(0.0, 0.4, (300, 3)).astype(np.float32)
    pts[7] = pts[100]; pts[8] = pts[101]
    nrm = K.unit_normals(rng, 300)
    nrm[::5] = 0.0
    r = 0.12
    counts, m = FO.spfh(pts, nrm, r)
    counts_l, m_l = FO.spfh_loop(pts, nrm, r)
    assert np.array_equal(counts, counts_l) and np.array_equal(m, m_l)
    assert 10 < m[m > 0].mean() < 60 and (m == 0).sum() >= 60 and np.array_equal(counts.reshape(300, 3, 11).sum(2), np.repeat(m[:, None], 3, 1))
    F, valid, F64 = FO.fpfh(pts, counts, m, r)
    F_l, valid_l, F64_l = FO.fpfh_loop(pts, counts, m, r)
    assert np.array_equal(valid, valid_l) and np.array_equal(F64.view(np.int64), F64_l.view(np.int64)) and np.array_equal(F.view(np.int32), F_l.view(np.int32))
    assert np.array_equal(valid, m > 0) and not F[~valid].any()
    # each third of a valid row with a valid neighbour sums to 200: 100 of its own histogram, 100 of its neighbours'
    full = valid & (F64.reshape(300, 3, 11).sum(2) > 150).all(1)
    assert full.sum() > 200 and np.abs(F64[full].reshape(-1, 3, 11).sum(2) - 200.0).max() < 1e-9


def test_half_plane_bins_equal_the_atan2_bins():
    """The half-plane rule against clamp(floor(11 (atan2(y, x) + pi) / (2 pi))) on 2,000,000 normal draws; a draw within 1e-9 rad of a
    bin edge may differ (the arc tangent's own rounding decides it) and is left out: at most one in a million."""
    rng = np.random.default_rng(0xa7a2)
    y, x = rng.normal(size=2_000_000), rng.normal(size=2_000_000)
    ang = np.arctan2(y, x)
    edges = np.pi * (2.0 * np.arange(0, 12) - 11.0) / 11.0
    near = (np.abs(ang[:, None] - edges[None, :]) < 1e-9).any(1)
    share = near.mean()
    print(f'draws within 1e-9 rad of a bin edge: {int(near.sum())} of {y.shape[0]}')
    assert share <= 1e-6
    got, want = FO.bin_angle(y, x), FO.bin_angle_atan2(y, x)
    assert np.array_equal(got[~near], want[~near])
    assert np.array_equal(np.bincount(got, minlength=11) > 150000, np.ones(11, bool))
    # the constants are the cosines and sines of the edges
    k = np.arange(6, 11)
    assert np.abs(np.array(FO.EDGE_C) - np.cos(np.pi * (2 * k - 11) / 11)).max() < 2e-16 and np.abs(np.array(FO.EDGE_S) - np.sin(np.pi * (2 * k - 11) / 11)).max() < 2e-16
    # and the special points of the rule
    assert FO.bin_angle(0.0, 0.0) == 5 and FO.bin_angle(0.0, -1.0) == 10 and FO.bin_angle(0.0, 1.0) == 5 and FO.bin_angle(-1e-300, -1.0) == 0
    assert list(FO.bin_linear(np.array([-1.0, -1.0 - 1e-16, 1.0, 1.0 + 1e-15, 0.0]))) == [0, 0, 10, 10, 5]


def _math_table():
    """Rows (x_i, n_i, x_j, n_j, c): seeded pairs with float32 coordinates, the axis family's pairs, axis-aligned rows whose orientation dot
    is exactly 0, zero normals and a duplicated point."""
    rng = np.random.default_rng(0x3a7b)
    n = 4000
    xi = rng.uniform(-1, 1, (n, 3)).astype(np.float32).astype(np.float64)
    xj = (xi + rng.uniform(-0.2, 0.2, (n, 3))).astype(np.float32).astype(np.float64)
    rows = [np.concatenate([xi, K.unit_normals(rng, n), xj, K.unit_normals(rng, n), np.tile(rng.uniform(-1, 1, (1, 3)), (n, 1))], 1)]
    for _, ni, dp, nj in K.AXIS_PAIRS:
        for c in ((0.5, 0.25, 3.0), (0.0, 0.0, 0.0), (1.0, -2.0, -1.0)):
            rows.append(np.concatenate([np.zeros(3), ni, dp, nj, c])[None])
            rows.append(np.concatenate([dp, nj, np.zeros(3), ni, c])[None])
    pts, nrm = K.orient_case()
    c = np.tile(np.float64(K.ORIENT_VIEWPOINT)[None], (500, 1))
    rows.append(np.concatenate([pts[:500].astype(np.float64), nrm[:500, :3], pts[500:1000].astype(np.float64), nrm[500:1000, :3], c], 1))
    same = rows[0][:5].copy(); same[:, 6:9] = same[:, 0:3]          # d2 == 0
    rows.append(same)
    return np.ascontiguousarray(np.concatenate(rows), np.float64)


def _math_expected(t):
    xi, ni, xj, nj, c = (t[:, 3 * q:3 * q + 3] for q in range(5))
    fi, fj = FO.orient_flags(xi, ni, c), FO.orient_flags(xj, nj, c)
    ni, nj = np.where(fi[:, None], -ni, ni), np.where(fj[:, None], -nj, nj)
    dp = xj - xi
    d2 = FO.dot(dp, dp)
    ok, b1, b2, b3 = FO.pair_bins(dp, np.where(d2 > 0, d2, 1.0), ni, nj)
    ok = ok & (d2 > 0)
    b = np.where(ok[:, None], np.stack([b1, b2, b3], 1), -1)
    return np.concatenate([fi[:, None], fj[:, None], ~ok[:, None], b], 1).astype(np.int64)


def test_fpfh_math_header_under_the_sanitizers(tmp_path):
    """csrc/fpfh_math.h compiled into a stand-alone host program (tests/_fpfh_math_check.cpp, its own main) with AddressSanitizer and
    UndefinedBehaviorSanitizer: orientation flags, skip flags and the three bins of every row of a seeded table equal the oracle's."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'fpfh_math_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                           '-I' + os.path.join(ROOT, 'roreg_amd', 'csrc'), os.path.join(HERE, '_fpfh_math_check.cpp'), '-o', exe])
    table = _math_table()
    path = str(tmp_path / 'table.f64')
    table.tofile(path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().split('\n')
    assert int(lines[-1]) == table.shape[0]
    got = np.array([[int(v) for v in ln.split()] for ln in lines[:-1]], np.int64)
    want = _math_expected(table)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, f'{bad.size} rows differ, the first: row {bad[0]} got {got[bad[0]]} want {want[bad[0]]}'
    # the table reaches what it is for: both orientation answers, exact zero dots, skipped pairs, every bin of every feature
    xi, ni, c = table[:, 0:3], table[:, 3:6], table[:, 12:15]
    assert want[:, 0].sum() > 1000 and (want[:, 0] == 0).sum() > 1000 and ((FO.dot(ni, c - xi) == 0.0) & (ni != 0).any(1)).sum() >= 20
    assert want[:, 2].sum() >= 10 and all(set(want[want[:, 2] == 0, q]) == set(range(11)) for q in (3, 4, 5))


def test_axis_family_reaches_the_edges():
    """What tests/_fpfh_cases.py AXIS_PAIRS says of each pair, from the oracle's pair feature."""
    f = {}
    for name, ni, dp, nj in K.AXIS_PAIRS:
        d2 = FO.dot(dp, dp)
        a1, a2 = FO.dot(ni, dp) / np.sqrt(d2), FO.dot(nj, dp) / np.sqrt(d2)
        ok, y, x, f2, f3 = FO.pair_feature(dp, d2, ni, nj)
        f[name] = dict(a1=a1, a2=a2, ok=bool(ok), y=float(y), x=float(x), f2=float(f2), f3=float(f3), bins=[int(v) for v in FO.pair_bins(dp, d2, ni, nj)[1:]])
        assert d2 <= K.AXIS_R ** 2
    a = f['f2_plus_one_xy_zero_tie']
    assert a['ok'] and a['a1'] == 0.0 and a['a2'] == 0.0 and a['f2'] == 1.0 and a['x'] == 0.0 and a['y'] == 0.0 and a['bins'] == [5, 10, 5]
    assert f['f2_minus_one']['f2'] == -1.0 and f['f2_minus_one']['bins'][1] == 0
    b = f['y_zero_x_negative']
    assert b['y'] == 0.0 and b['x'] == -1.0 and b['bins'][0] == 10
    t = f['tie_nonzero']
    assert t['a1'] == t['a2'] and t['a1'] > 0.7 and t['f3'] == t['a1']                  # no swap: f3 = a1, not -a2
    assert not f['no_frame']['ok'] and not FO.pair_feature(-K.EX, 1.0, K.EY, K.EX)[0]   # ... from either end
    s = f['swap']
    assert s['a1'] == 0.0 and abs(s['a2']) > 0.7 and s['f3'] == -s['a2']
    # the pairs are isolated: in the family's cloud every point has exactly one neighbour, and the no-frame pair has none that counts
    pts, nrm = K.axis_case()
    counts, m = FO.spfh(pts, nrm, K.AXIS_R)
    want = np.ones(len(pts), np.int32); want[2 * 4:2 * 4 + 2] = 0
    assert np.array_equal(m, want)


@pytest.mark.parametrize('case', [c for c in K.CASES if c[0] != 'terrain'], ids=K.case_id)
def test_families_meet_their_conditions(case):
    pts, nrm, r = K.case(*case)
    counts, m, F, valid, _ = K.reference(*case)
    n = pts.shape[0]
    assert counts.shape == (n, 33) and np.array_equal(counts.reshape(n, 3, 11).sum(2), np.repeat(m[:, None], 3, 1)) and np.array_equal(valid, m > 0)
    name, arg = case
    if name == 'box' and arg >= 255:
        assert 20 <= m.mean() <= 45, m.mean()
    if name == 'box' and arg <= 5:
        assert (m == arg - 1).all()
    if name == 'lattice':
        kind = PC.lattice_case(arg)[1]                            # a centre counts its 30 neighbours at exactly r and none of those beyond
        assert (m[kind == PC.KIND_CENTRE] == 30).all()
    if name == 'duplicate':
        d = pts[None, 10:40].astype(np.float64) - pts[:, None].astype(np.float64)
        assert ((d == 0).all(2).sum(0) == 2).all() and (m[10:40] == m[200:230]).all()
    if name == 'third':
        assert (m[::3] == 0).all() and (m[1::3] > 0).all() and not F[::3].any()
    if name == 'none':
        assert not m.any() and not counts.any() and not F.any()
    if name == 'cluster':
        assert (m == K.CLUSTER_N - 1).all() and counts.max() > 255


def _mutual(F0, F1):
    """Mutual nearest neighbours of two float32 descriptor tables, the first index among equal distances."""
    a, b = F0.astype(np.float64), F1.astype(np.float64)
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    n01, n10 = d.argmin(1), d.argmin(0)
    i = np.arange(a.shape[0])
    keep = n10[n01] == i
    return np.stack([i[keep], n01[keep]], 1)


@pytest.mark.parametrize('seed', K.TERRAIN_SEEDS)
def test_oracle_chain_registers_the_terrain(seed):
    """Voxel oracle at 0.05, normal oracle at 0.1, centroid orientation, FPFH at 0.25, mutual nearest neighbours, the spatial-compatibility
    oracle at tau = 0.1, the hypothesis with most inliers: within 2 degrees and 5 cm of the ground truth.  The bar only shows that the
    family exercises the pipeline.  The chain stops at a raw hypothesis, a Kabsch fit of 20 matched voxel centroids; the inliers that
    pick it are counted within one voxel (K.TERRAIN_INLIER, where the reasoning is).  Seeds 0..3: 0.154 degrees / 1.47 cm, 0.724 / 0.97,
    0.161 / 0.43, 0.878 / 1.08, on 1426, 1258, 1646, 1588 mutual matches with 305, 169, 294, 502 of them within 0.1 of the truth.  The
    choice is not delicate: at every radius of 0.03, 0.04, 0.05, 0.06, 0.07, 0.08 the four winners lie within 1.41 degrees and 2.51 cm.
    Counted at 0.1 the near-tied hypotheses are not told apart -- the twelve best of seed 2 hold 298..302 inliers and lie 0.16 .. 2.67
    degrees from the truth -- and the winners are 0.835, 1.748, 2.671 and 1.072 degrees off, the third over the bar: each printed below."""
    Tg = K.terrain_pair(seed)[2]
    views = [K.terrain_view(seed, w) for w in (0, 1)]
    refs = [K.terrain_reference(seed, w) for w in (0, 1)]
    rows = [np.nonzero(r[4])[0] for r in refs]
    mm = _mutual(refs[0][3][rows[0]], refs[1][3][rows[1]])
    P = views[0][0][rows[0][mm[:, 0]]].astype(np.float64); Q = views[1][0][rows[1][mm[:, 1]]].astype(np.float64)
    hyp = SO.hypotheses(P, Q, K.TERRAIN_TAU).Trans
    res = np.sqrt((((Q @ hyp[:, :, :3].transpose(0, 2, 1)) + hyp[:, None, :, 3] - P[None]) ** 2).sum(2))
    inl = (res <= K.TERRAIN_INLIER).sum(1)
    best = int(inl.argmax())
    loose = int((res <= K.TERRAIN_TAU).sum(1).argmax())
    T = np.eye(4); T[:3] = hyp[best]
    true_inl = int((np.sqrt((((Q @ Tg[:3, :3].T) + Tg[:3, 3] - P) ** 2).sum(1)) <= K.TERRAIN_TAU).sum())
    deg, dt = K.pose_error(T, Tg)
    Tl = np.eye(4); Tl[:3] = hyp[loose]
    print(f'terrain seed {seed}: {views[0][0].shape[0]} / {views[1][0].shape[0]} points, {mm.shape[0]} mutual matches, {true_inl} true inliers, '
          f'best hypothesis {int(inl[best])} inliers within {K.TERRAIN_INLIER}, {deg:.3f} degrees, {dt * 100:.2f} cm '
          f'(the winner counted at {K.TERRAIN_TAU}: {K.pose_error(Tl, Tg)[0]:.3f} degrees)')
    assert deg <= K.TERRAIN_DEG and dt <= K.TERRAIN_T
