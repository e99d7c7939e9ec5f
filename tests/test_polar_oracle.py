"""csrc/polar.h -- polar_uvt, the close of both RANSAC refinements, and polar_proper, the close of every spatial-compatibility hypothesis --
in a stand-alone host program (tests/_polar_check.cpp, its own main) under AddressSanitizer and UndefinedBehaviorSanitizer, against mpmath
at 60 digits (tests/_polar_oracle.py) on the seeded families of tests/_polar_cases.py; and the conditions the GPU tests
(tests/test_hip_kabsch_edges.py) rely on: the reduction bars hold for a numpy evaluation of the same two-pass formula, the cases cover every
combination they name.  No GPU.

Errors are in units of eps kappa, eps = 2^-52, kappa = sigma1 / (sigma2 + sigma3) for U V^T (sigma2 - sigma3 where polar_proper fixes a
reflection).  The bar of a family is max(8, LAPACK's figure on the same matrices): 8 is the polar factor's perturbation bound
2 |dH| / (sigma2 + sigma3) at a backward error of 4 eps |H|; LAPACK's figure is numpy's U @ VT against mpmath in the same units.  Neither
comes from the header under test."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _polar_cases as C
import _polar_oracle as PO

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = PO.EPS
FLOOR = 8.0
ILL_POSED = 1e-6                                                   # polar_proper's accuracy is not asserted where sigma2 - sigma3 < 1e-6 sigma1 under a reflection


@pytest.fixture(scope='module')
def header(tmp_path_factory):
    """-> run(H [n,3,3]) = (polar_uvt [n,3,3], polar_proper [n,3,3]) from the sanitized host program"""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    tmp = tmp_path_factory.mktemp('polar')
    exe = str(tmp / 'polar_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                           '-I' + os.path.join(ROOT, 'roreg_amd', 'csrc'), os.path.join(HERE, '_polar_check.cpp'), '-o', exe])
    count = [0]

    def run(H):
        H = np.ascontiguousarray(H, np.float64).reshape(-1, 3, 3)
        count[0] += 1
        path = str(tmp / f'matrices{count[0]}.f64')
        H.tofile(path)
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().split('\n')
        assert int(lines[-1]) == H.shape[0]
        got = np.array([[int(v, 16) for v in ln.split()] for ln in lines[:-1]], np.uint64).view(np.float64).reshape(-1, 2, 3, 3)
        return got[:, 0], got[:, 1]

    return run


def _lapack(H):
    U, _, VT = np.linalg.svd(H)
    R = U @ VT
    D = np.diag([1.0, 1.0, 1.0 if np.linalg.det(R) > 0 else -1.0])
    return R, U @ D @ VT


def _units(err, kappa):
    return err / (EPS * kappa)


def family_figures(H, refs, uvt, proper):
    """per matrix, in units of eps kappa: (header U V^T, LAPACK U V^T, header proper, LAPACK proper; NaN where the proper problem is ill posed)"""
    out = np.full((H.shape[0], 4), np.nan)
    for i, (h, ref) in enumerate(zip(H, refs)):
        Rl, Rlp = _lapack(h)
        ku, kp = PO.kappa_uvt(ref['S']), PO.kappa_proper(ref['S'], ref['det'])
        out[i, 0], out[i, 1] = _units(PO.diff(uvt[i], ref['R']), ku), _units(PO.diff(Rl, ref['R']), ku)
        if ref['det'] > 0 or ref['S'][1] - ref['S'][2] >= ILL_POSED * ref['S'][0]:
            out[i, 2], out[i, 3] = _units(PO.diff(proper[i], ref['Rp']), kp), _units(PO.diff(Rlp, ref['Rp']), kp)
    return out


def _ortho(R):
    return np.abs(R @ R.T - np.eye(3)).max()


@pytest.fixture(scope='module')
def results(header):
    f = C.families(C.N_CPU)
    return {name: header(H) for name, H in f.items()}


def test_accuracy_per_family_against_mpmath(results):
    """polar_uvt and polar_proper within the family's bar; every polar_proper row of rank >= 2 orthogonal with det +1 to 64 eps, every
    polar_uvt row with the reference's det."""
    f, refs = C.families(C.N_CPU), C.reference(C.N_CPU)
    bad = []
    for name in C.ACCURACY_UVT:
        uvt, proper = results[name]
        fig = family_figures(f[name], refs[name], uvt, proper)
        bar_u, bar_p = max(FLOOR, fig[:, 1].max()), max(FLOOR, np.nanmax(fig[:, 3]))
        skipped = int(np.isnan(fig[:, 2]).sum())
        print(f'{name:12s} {f[name].shape[0]:4d} matrices: U V^T header {fig[:, 0].max():6.2f} LAPACK {fig[:, 1].max():6.2f} bar {bar_u:6.2f} | proper header '
              f'{np.nanmax(fig[:, 2]):6.2f} LAPACK {np.nanmax(fig[:, 3]):6.2f} bar {bar_p:6.2f} ({skipped} ill posed)')
        if not fig[:, 0].max() <= bar_u:
            bad.append((name, 'uvt', fig[:, 0].max(), bar_u))
        if not np.nanmax(fig[:, 2]) <= bar_p:
            bad.append((name, 'proper', np.nanmax(fig[:, 2]), bar_p))
        for i, ref in enumerate(refs[name]):
            if not (_ortho(proper[i]) <= 64 * EPS and abs(np.linalg.det(proper[i]) - 1.0) <= 64 * EPS):
                bad.append((name, i, 'proper is no rotation', _ortho(proper[i]), np.linalg.det(proper[i])))
            if not (_ortho(uvt[i]) <= 64 * EPS and abs(np.linalg.det(uvt[i]) - ref['det']) <= 64 * EPS):
                bad.append((name, i, 'uvt det', np.linalg.det(uvt[i]), ref['det']))
    assert not bad, bad[:10]


def test_exact_rank_two_gives_the_proper_rotation_of_the_two_leading_pairs(results):
    f, refs = C.families(C.N_CPU), C.reference(C.N_CPU)
    H, (uvt, proper) = f['rank2'], results['rank2']
    assert all(C.exactly_rank2(h) for h in H)
    gen = family_figures(f['generic'], refs['generic'], *results['generic'])
    bar = max(FLOOR, gen[:, 1].max())
    worst = 0.0
    for i, ref in enumerate(refs['rank2']):
        kappa = ref['S'][0] / ref['S'][1]
        worst = max(worst, _units(PO.diff(uvt[i], ref['R2']), kappa))
        assert _ortho(uvt[i]) <= 64 * EPS and abs(np.linalg.det(uvt[i]) - 1.0) <= 64 * EPS, i
        assert np.array_equal(uvt[i], proper[i]), i
    print(f'rank2: {H.shape[0]} matrices, header against u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T: {worst:.2f} eps sigma1 / sigma2, bar {bar:.2f}')
    assert worst <= bar


def test_degenerate_inputs(results, header):
    """rank <= 1 and H = 0: exactly I from both; one NaN entry: NaN in all nine"""
    for name in ('rank1', 'zero'):
        for R in results[name]:
            assert R.shape[0] >= 2 and all(np.array_equal(r, np.eye(3)) for r in R), name
    for R in results['nan']:
        assert R.shape[0] == 9 and np.isnan(R).all()
    inf = C.families(C.N_CPU)['generic'][:4].copy()
    inf[0, 0, 0], inf[1, 2, 1], inf[2, 1, 1], inf[3, 0, 2] = np.inf, -np.inf, np.inf, -np.inf
    inf[2, 0, 0] = -np.inf
    for R in header(inf):                                          # an infinite entry (LAPACK refuses it): NaN as well, no trip through the sweeps
        assert np.isnan(R).all()


def test_scale_does_not_change_the_factor(header):
    """R(2^k H) = R(H) bit for bit for k = +-200, +-500 on a well- and an ill-conditioned matrix (the decimal scales 1e-6 .. 1e6 are inside every
    family of test_accuracy_per_family_against_mpmath)"""
    members = C.pow2_members(C.N_CPU)
    base = header(np.stack([H for _, H, _ in members]))
    scaled = header(np.stack([np.ldexp(H, k) for _, H, k in members]))
    for q, (name, H, k) in enumerate(members):
        assert np.isfinite(np.ldexp(H, k)).all() and np.any(np.ldexp(H, k))
        for which in (0, 1):
            assert base[which][q].tobytes() == scaled[which][q].tobytes(), (name, k, 'uvt proper'.split()[which], np.abs(base[which][q] - scaled[which][q]).max())


def test_either_side_of_the_hosts_lapack_switch(results):
    """hip.stats_rank_deficient_many sends sigma3 <= 1e-10 sigma1 to numpy's U @ VT: on the families either side of it the header and numpy
    agree within the family's bar, so a pair's result does not depend on the route that closed it."""
    from roreg_amd import hip
    f, refs = C.families(C.N_CPU), C.reference(C.N_CPU)
    worst_abs = 0.0
    for s in C.SWITCH_S3:
        name = f'small-{s:g}'
        H, (uvt, proper) = f[name], results[name]
        fig = family_figures(H, refs[name], uvt, proper)
        bar = max(FLOOR, fig[:, 1].max())
        routed = hip.stats_rank_deficient_many(np.concatenate([H.reshape(-1, 9), np.zeros((H.shape[0], 7))], 1))
        assert routed.all() if s < 1e-10 else not routed.any(), name
        gap = np.array([_units(np.abs(uvt[i] - _lapack(H[i])[0]).max(), PO.kappa_uvt(refs[name][i]['S'])) for i in range(H.shape[0])])
        worst_abs = max(worst_abs, max(np.abs(uvt[i] - _lapack(H[i])[0]).max() for i in range(H.shape[0])))
        print(f'{name}: header against numpy U @ VT {gap.max():.2f} eps kappa (bar {bar:.2f}); {int(routed.sum())} of {H.shape[0]} go to LAPACK')
        assert gap.max() <= bar, name
    print(f'largest |R_header - R_LAPACK| either side of the switch: {worst_abs:.2e}')


def test_families_reach_their_purpose(results):
    f, refs = C.families(C.N_GPU), C.reference(C.N_GPU)
    reflections = sum(r['det'] < 0 for name in refs for r in refs[name])
    rank2 = sum(C.exactly_rank2(h) for h in f['rank2'])
    skips = sum(C.first_pair_orthogonal(h) for name in f for h in f[name])
    print(f'{reflections} rows with a reflection, {rank2} exact rank-2 rows (the ngood == 2 branch), {skips} rows whose first column pair has gamma == 0')
    assert reflections >= 8 and rank2 >= 8 and skips >= 8
    # exact rank 2 leaves one column of A at rounding level, below polar_uvt's 1e-13 of the largest: ngood == 2; sigma3 = 1e-12 stays above it
    assert all(r['S'][2] <= 1e-14 * r['S'][0] for r in refs['rank2']) and all(r['S'][2] >= 5e-13 * r['S'][0] for r in refs['small-1e-12'])
    for name, H in f.items():
        assert H.shape[0] <= 45 and (name in ('zero', 'nan') or H.shape[0] >= 10), name
        if name not in C.DEGENERATE + ('rank2',):                          # (rank2's negative decades are powers of two: exactness)
            scales = np.log10(np.array([r['S'][0] for r in refs[name]]))
            assert scales.min() < -4 and scales.max() > 4, name            # the decimal scales are in


# ---- the conditions of the GPU tests --------------------------------------------------------------------------------------------------------
def test_reduction_cases_cover_every_combination():
    cases = C.reduction_cases()
    assert len(cases) == len(C.SIZES) * len(C.PATTERNS)
    assert {(c[1], c[2]) for c in cases} == {(p, w) for p in C.PATTERNS for w in C.WEIGHTS}
    assert {(c[1], c[3]) for c in cases} == {(p, f) for p in C.PATTERNS for f in C.FORMS}
    assert {(c[0], c[3]) for c in cases} == {(m, f) for m in C.SIZES for f in C.FORMS}
    assert {(c[1], c[4]) for c in cases} == {(p, o) for p in C.PATTERNS for o in (0, 1)}
    assert {(c[2], c[3]) for c in cases if c[3] != 'none'} == {(w, f) for w in C.WEIGHTS for f in ('f64', 'f32')}


def test_numpy_two_pass_formula_stays_inside_the_reduction_bars():
    """The bars of the device test -- gamma eps (sum w'|a||b| + |c0| sum w'|b| + |c1| sum w'|a|) on H and gamma eps sum w'|k| on the centroids,
    gamma = ceil(M / 256) + 16 -- hold for numpy's float64 evaluation of the same two-pass formula on every case: they are no tighter than
    float64 summation itself."""
    worst = [0.0, 0.0]
    for key in C.reduction_cases():
        case, ref = C.reduction_case(*key), C.reduction_reference(key)
        if ref is None:
            assert case['rows'].size == 0
            continue
        H, c0, c1 = C.numpy_two_pass(case)
        bH, b0, b1 = C.reduction_bars(case, ref)
        eH = PO.vec_diff(H, ref['mp']['H'])
        e0, e1 = PO.vec_diff(c0, ref['mp']['c0']), PO.vec_diff(c1, ref['mp']['c1'])
        frac = lambda e, b: np.where(b > 0, e / np.where(b > 0, b, 1.0), 0.0).max()          # (one inlier: a = b = 0, H = 0 exactly, bar 0)
        worst = [max(worst[0], frac(eH, bH)), max(worst[1], frac(e0, b0), frac(e1, b1))]
        assert (eH <= bH).all() and (e0 <= b0).all() and (e1 <= b1).all(), key
    print(f'numpy two-pass: largest error as a fraction of the bar: H {worst[0]:.3f}, centroids {worst[1]:.3f}')


def test_few_inlier_model_is_the_stated_order():
    """the rational model of the n <= 7 path: its weights and centroids (no fused step there) equal a plain float64 loop bit for bit, its H
    is within a few eps of the exact one"""
    rng = np.random.default_rng(5)
    k0, k1, w = rng.normal(size=(7, 3)), rng.normal(size=(7, 3)), rng.uniform(0.1, 1, 7)
    for n in range(1, 8):
        rows = list(range(n))
        H, c0, c1, cnt = C.few_inlier_model(k0, k1, w, rows, False)
        tot = 0.0
        for i in rows:
            tot = tot + w[i]
        sk = [w[i] / tot for i in rows]
        want0 = np.zeros(3)
        for q, i in enumerate(rows):
            want0 = k0[i] * sk[q] if q == 0 else want0 + k0[i] * sk[q]
        assert cnt == n and np.array_equal(c0, want0)
        ref = PO.kabsch(k0, k1, w, rows)
        assert np.abs(H - ref['H']).max() <= 32 * EPS * np.abs(k0).max() * np.abs(k1).max()


def test_sc2_cases_keep_the_ill_posed_cap_and_the_near_planar_one_has_reflections():
    """With the numpy oracle: every case of test_hip_kabsch_edges.py::test_sc2_fits_against_mpmath leaves at most 10 % of its fitted rows
    ill posed (sigma2 < 1e-6 sigma1, or sigma2 - sigma3 < 1e-6 sigma1 under a reflection), the near-planar case has >= 8 rows with a
    reflection to fix and keeps the threshold margin."""
    import _sc2_cases as SC
    for case in C.sc2_cases():
        fitted = (case.ref.cons >= 0).sum(1) >= 3
        det = np.sign(np.linalg.det(SC.unfixed_rotations(case, fitted))) if fitted.any() else np.zeros(0)
        sig = case.ref.sigma[fitted]
        ill = np.array([C.sc2_posedness(s, d)[0] for s, d in zip(sig, det)], bool)
        print(f'{case.name}: {int(fitted.sum())} fitted rows, {int(ill.sum())} ill posed, {int((det < 0).sum())} with a reflection to fix, margin {case.margin:.1e}')
        assert case.margin >= SC.MARGIN and fitted.sum() >= 50 and ill.sum() <= C.SC2_SKIP_CAP * fitted.sum(), case.name
        if case.name.startswith('near-planar'):
            assert ((det < 0) & ~ill).sum() >= 8 and (det > 0).sum() >= 8
