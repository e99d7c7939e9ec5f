"""The Kabsch closes on the device against mpmath at 60 digits (tests/_polar_oracle.py): the float64 reduction of refine_body
(csrc/ransac.hip) in all its forms -- per-pair launch, batched launch, the 1..7-inlier sequential path, float64 weights, float32 scores and
the batch's w = None --, the 3x3 closing step (csrc/polar.h's polar_uvt and polar_proper) on the families of tests/_polar_cases.py, the two
together on planted motions, and the fits of the spatial-compatibility hypotheses (csrc/sc2.hip).  hip.refine(..., want_stats=True) returns the
H, c0, c1 the device reduced and the T it closed from them, which separates the two halves.  tests/test_polar_oracle.py asserts on the CPU what
these tests rely on: the bars hold for numpy's evaluation of the same formulas, the families reach their branches.  GPU only.

Bars.  Reduction, per element, gamma = ceil(M / 256) + 16 (a thread's sequential sum of ceil(M / 256) terms, the butterfly and the four-wave
sum, the products and the centring), w' the normalised weights, a, b the centred coordinates:
    |H_ij - H_mp| <= gamma eps (sum w'|a_i||b_j| + |c0_i| sum w'|b_j| + |c1_j| sum w'|a_i|),   |c - c_mp| <= gamma eps sum w'|k|.
Closing step, per family: max(8, LAPACK's own error on the same matrices) in units of eps sigma1 / (sigma2 + sigma3) -- sigma2 - sigma3 where
polar_proper fixes a reflection.  None of them is taken from the kernels' output."""
import functools

import numpy as np
import pytest
import torch

import _polar_cases as C
import _polar_oracle as PO

pytestmark = pytest.mark.gpu
EPS = PO.EPS
FLOOR = 8.0
HUGE = 2.0 ** 110                                                  # an inlier distance that admits every row, the 2^100-scaled clouds included


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _task(k0, k1, T, w=None):
    M = k0.shape[0]
    m = np.stack([np.arange(M), np.arange(M)], 1).astype(np.int64)
    return (cu(k0), cu(k1), cu(m), None if w is None else cu(w), cu(np.ascontiguousarray(T[None, :3, :])), None)


def _refine(case, dist=C.DIST):
    """the case through the launch its weight form names -> (T [4,4], stats [16]) host arrays"""
    from roreg_amd import hip
    k0, k1, T = case['k0'], case['k1'], case['T']
    if case['form'] == 'none':                                     # w = None exists in the batch only: refine_batch from the given transform
        *_, ctx = hip.ransac_batch([_task(k0, k1, T)], dist, keep=True)
        Tq, st = hip.refine_batch(ctx, [0], T[None], dist)
        return Tq[0].cpu().numpy(), st[0].cpu().numpy()
    Tq, st = hip.refine(cu(k0), cu(k1), cu(case['w']), dist, T_in=cu(T), want_stats=True, w_f32=case['form'] == 'f32')
    return Tq.cpu().numpy(), st.cpu().numpy()


def _lapack(H):
    U, _, VT = np.linalg.svd(H)
    R = U @ VT
    return R, U @ np.diag([1.0, 1.0, 1.0 if np.linalg.det(R) > 0 else -1.0]) @ VT


@functools.lru_cache(maxsize=None)
def _polar_of(bits):
    return PO.polar(np.frombuffer(bits, np.float64).reshape(3, 3))


def _polar(H):
    return _polar_of(np.ascontiguousarray(H, np.float64).tobytes())


def _ortho(R):
    return np.abs(R @ R.T - np.eye(3)).max()


# ---- the reduction ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', C.SIZES)
def test_reduction_against_mpmath(M):
    """H, c0, c1 of every inlier pattern at this M within the reduction bars of the exact weighted sums; no inlier: NaN in R and t; one
    inlier: H = 0 exactly and R = I."""
    for key in [k for k in C.reduction_cases() if k[0] == M]:
        case, ref = C.reduction_case(*key), C.reduction_reference(key)
        T, st = _refine(case)
        assert np.array_equal(T[3], [0, 0, 0, 1]), key
        if ref is None:
            assert np.isnan(T[:3]).all(), key
            continue
        n = case['rows'].size
        wn, _, S32 = C.effective_weights(case)
        if case['form'] == 'f32':
            assert st[15] == S32, key
        else:
            assert abs(st[15] - np.sum(wn)) <= 1e-12 * np.sum(wn), key                              # the same rows were summed
        bH, b0, b1 = C.reduction_bars(case, ref)
        eH = PO.vec_diff(st[:9].reshape(3, 3), ref['mp']['H'])
        e0, e1 = PO.vec_diff(st[9:12], ref['mp']['c0']), PO.vec_diff(st[12:15], ref['mp']['c1'])
        frac = lambda e, b: float(np.where(b > 0, e / np.where(b > 0, b, 1.0), np.where(e > 0, np.inf, 0.0)).max())
        print(f'{key}: {n} inliers, error / bar: H {frac(eH, bH):.3f}, c0 {frac(e0, b0):.3f}, c1 {frac(e1, b1):.3f}')
        assert (eH <= bH).all() and (e0 <= b0).all() and (e1 <= b1).all(), (key, eH / bH, e0 / b0, e1 / b1)
        if n == 1:
            assert not st[:9].any() and np.array_equal(T[:3, :3], np.eye(3)), key
        assert np.isfinite(T).all(), key


@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_few_inlier_path_is_the_stated_order_bit_for_bit(f32):
    """n = 1..7 inliers among 300 rows: stats equal, bit for bit, the model in exact rationals of sequential sums and the k-ordered chain
    fma((k0 - c0) s, k1 - c1, acc), each step rounded once (tests/_polar_cases.py few_inlier_model)."""
    from roreg_amd import hip
    rng = np.random.default_rng(0x1717)
    T = C.motion()
    for n in range(1, 8):
        M = 300
        k1 = rng.uniform(-1.5, 1.5, (M, 3))
        k0 = k1 @ T[:3, :3].T + T[:3, 3] + 5.0
        rows = np.sort(rng.choice(M, n, replace=False))
        k0[rows] -= 5.0
        k0[rows] += rng.normal(0, 1e-3, (n, 3))
        w = 10.0 ** rng.uniform(-6, 0, M)
        if f32:
            w = w.astype(np.float32).astype(np.float64)
        Tq, st = hip.refine(cu(k0), cu(k1), cu(w), C.DIST, T_in=cu(T), want_stats=True, w_f32=f32)
        st = st.cpu().numpy()
        H, c0, c1, _ = C.few_inlier_model(k0, k1, w, list(rows), f32)
        wn = w[rows] / np.sum(w[rows]) if not f32 else (w[rows].astype(np.float32) / np.sum(w[rows].astype(np.float32))).astype(np.float64)
        Hnp = ((k0[rows] - c0) * wn[:, None]).T @ (k1[rows] - c1)
        print(f'n = {n}: numpy matmul {"agrees" if np.array_equal(Hnp, H) else "differs"} with the model (not asserted); '
              f'max |H_dev - H_model| {np.abs(st[:9].reshape(3, 3) - H).max():.1e}')
        assert st[:9].tobytes() == np.ascontiguousarray(H).tobytes(), n
        assert st[9:12].tobytes() == c0.tobytes() and st[12:15].tobytes() == c1.tobytes(), n
        assert np.isfinite(Tq.cpu().numpy()).all()


# ---- the closing step --------------------------------------------------------------------------------------------------------------------------
def _closing_tasks():
    """[(family, index, k0, k1, T)] for every finite family, and one generic member with both clouds times 2^100 (H times 2^200)"""
    f = C.families(C.N_GPU)
    out = []
    for name, Hs in f.items():
        if name in ('nan', 'zero'):                                # (a NaN coordinate is no inlier; H = 0 is the single inlier of the reduction test)
            continue
        for i, A in enumerate(Hs):
            out.append((name, i) + C.closing_points(A, seed=len(out)))
    out.append(('generic*2^200', 0) + C.closing_points(f['generic'][6], seed=len(out), coord_scale=2.0 ** 100))
    return out


def _check_closing(tasks, T, st, what):
    """T [n,4,4], st [n,16] of the tasks: R against the mpmath factor of the H the device reduced, t against c0 - R c1"""
    by_family = {}
    for q, (name, i, k0, k1, Tin) in enumerate(tasks):
        H, c0, c1, R, t = st[q, :9].reshape(3, 3), st[q, 9:12], st[q, 12:15], T[q, :3, :3], T[q, :3, 3]
        assert np.array_equal(T[q, 3], [0, 0, 0, 1]) and st[q, 15] == k0.shape[0], (what, name, i)
        if name == 'rank1':
            assert np.array_equal(R, np.eye(3)), (what, name, i)
        else:
            ref = _polar(H)
            Rl = _lapack(H)[0]
            if name == 'rank2':                                    # the reduced H is rank 2 to rounding: the proper rotation of the two leading pairs
                kappa = ref['S'][0] / ref['S'][1]
                assert ref['S'][2] <= 5e-14 * ref['S'][0], (what, name, i, ref['S'])        # below polar_uvt's 1e-13: ngood == 2
                fig = (PO.diff(R, ref['R2']) / (EPS * kappa), 0.0)
                assert abs(np.linalg.det(R) - 1.0) <= 64 * EPS, (what, name, i)
            else:
                kappa = PO.kappa_uvt(ref['S'])
                fig = (PO.diff(R, ref['R']) / (EPS * kappa), PO.diff(Rl, ref['R']) / (EPS * kappa))
                assert abs(np.linalg.det(R) - ref['det']) <= 64 * EPS, (what, name, i)
            assert _ortho(R) <= 64 * EPS, (what, name, i)
            by_family.setdefault(name, []).append(fig)
        with PO.mp.workdps(PO.DIGITS):
            want = [PO.mpf(float(c0[r])) - sum(PO.mpf(float(R[r, c])) * PO.mpf(float(c1[c])) for c in range(3)) for r in range(3)]
        et = PO.vec_diff(t, want)
        assert (et <= 4 * EPS * (np.linalg.norm(c0) + 3 * np.linalg.norm(c1))).all(), (what, name, i, et)
    generic_bar = max(FLOOR, max(f[1] for f in by_family['generic']))
    for name, figs in by_family.items():
        figs = np.array(figs)
        bar = generic_bar if name in ('rank2', 'generic*2^200') else max(FLOOR, figs[:, 1].max())
        print(f'{what} {name:14s} {len(figs):3d} tasks: device {figs[:, 0].max():6.2f}, LAPACK {figs[:, 1].max():6.2f}, bar {bar:6.2f} (eps kappa)')
        assert figs[:, 0].max() <= bar, (what, name)


def test_closing_step_per_pair_launch():
    from roreg_amd import hip
    tasks = _closing_tasks()
    out = [hip.refine(cu(k0), cu(k1), cu(np.ones(k0.shape[0])), HUGE, T_in=cu(Tin), want_stats=True) for _, _, k0, k1, Tin in tasks]
    T = torch.stack([o[0] for o in out]).cpu().numpy()
    st = torch.stack([o[1] for o in out]).cpu().numpy()
    _check_closing(tasks, T, st, 'refine')


def test_closing_step_batched_launches():
    """hip.ransac_batch's two refinements (w = None, from the scored hypothesis and from the first refinement) and hip.refine_batch"""
    from roreg_amd import hip
    tasks = _closing_tasks()
    best, T1, st1, T2, st2, ctx = hip.ransac_batch([_task(k0, k1, Tin) for _, _, k0, k1, Tin in tasks], HUGE, keep=True)
    assert (best.cpu().numpy() == 0).all()
    _check_closing(tasks, T1.cpu().numpy(), st1.cpu().numpy(), 'ransac_batch first')
    _check_closing(tasks, T2.cpu().numpy(), st2.cpu().numpy(), 'ransac_batch second')
    sel = list(range(0, len(tasks), 3)) + [len(tasks) - 1]
    T3, st3 = hip.refine_batch(ctx, sel, np.stack([tasks[q][4] for q in sel]), HUGE)
    _check_closing([tasks[q] for q in sel], T3.cpu().numpy(), st3.cpu().numpy(), 'refine_batch')


# ---- both halves together ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [257, 5000])
def test_planted_motion_end_to_end(M):
    """An exact rigid motion on M matches, 40 % of them outliers metres away: the refined T against the full mpmath Kabsch of the inlier set.
    |R - R_mp| <= 2 |bar_H|_F / (sigma2 + sigma3) + bar eps kappa (the reduction bar through the polar factor's perturbation bound, plus the
    closing bar), |t - t_mp| <= bar_c0 + bar_c1 + sqrt(3) |c1| bound_R + 4 eps (|c0| + 3 |c1|)."""
    from roreg_amd import hip
    rng = np.random.default_rng([0xe2e, M])
    T = C.motion(7)
    k1 = rng.uniform(-1.5, 1.5, (M, 3))
    k0 = k1 @ T[:3, :3].T + T[:3, 3]
    out = rng.random(M) < 0.4
    k0[out] += rng.choice([-1.0, 1.0], (int(out.sum()), 3)) * rng.uniform(3.0, 9.0, (int(out.sum()), 3))
    rows = np.flatnonzero(~out)
    w = 10.0 ** rng.uniform(-6, 0, M)
    ref = PO.kabsch(k0, k1, w, rows)
    case = dict(k0=k0, k1=k1, w=w, rows=rows, M=M, form='f64')
    bH, b0, b1 = C.reduction_bars(case, ref)
    for what, (Tq, st) in (('refine', _refine(dict(case, T=T))), ('refine_batch w=None', _refine(dict(case, T=T, form='none', w=None)))):
        if what != 'refine':
            ref = PO.kabsch(k0, k1, None, rows)
            bH, b0, b1 = C.reduction_bars(dict(case, w=None, form='none'), ref)
        S = ref['S']
        lap = PO.diff(_lapack(st[:9].reshape(3, 3))[0], _polar(st[:9].reshape(3, 3))['R']) / (EPS * PO.kappa_uvt(S))
        bound_R = 2 * np.linalg.norm(bH) / (S[1] + S[2]) + max(FLOOR, lap) * EPS * PO.kappa_uvt(S)
        bound_t = b0 + b1 + np.sqrt(3) * np.linalg.norm(ref['c1']) * bound_R + 4 * EPS * (np.linalg.norm(ref['c0']) + 3 * np.linalg.norm(ref['c1']))
        eR, et = PO.diff(Tq[:3, :3], ref['mp']['R']), PO.vec_diff(Tq[:3, 3], ref['mp']['t'])
        print(f'M = {M} {what}: {rows.size} inliers, |R - R_mp| {eR:.2e} (bound {bound_R:.2e}), |t - t_mp| {et.max():.2e} (bound {bound_t.min():.2e}), '
              f'distance from the planted motion {np.abs(Tq - T).max():.2e}')
        assert eR <= bound_R and (et <= bound_t).all()
        assert np.abs(Tq - T).max() <= 1e-12                       # (and the planted motion is recovered)


# ---- the spatial-compatibility fits -----------------------------------------------------------------------------------------------------------
SC2_CASES = C.sc2_cases()


@pytest.mark.parametrize('idx', range(len(SC2_CASES)), ids=[c.name for c in SC2_CASES])
def test_sc2_fits_against_mpmath(idx):
    """Every fitted row of the case (the rows the conditioning filter of tests/test_hip_sc2.py leaves out included): the rotation against the
    mpmath proper rotation of the consensus set the device lists, within 2 |bar_H|_F / gap + max(8, LAPACK) eps sigma1 / gap, gap = sigma2 +-
    sigma3 of that set; orthogonal, det +1 and finite on every row; at most 10 % of the rows skipped as ill posed."""
    from roreg_amd import hip
    case = SC2_CASES[idx]
    M = case.P.shape[0]
    m = np.stack([np.arange(M), np.arange(M)], 1).astype(np.int64)
    Trans, offsets, dbg = hip.sc2_hypotheses_batch([(cu(case.P), cu(case.Q), cu(m))], case.tau, case.max_seeds, case.K, debug=True)
    T, cons = Trans.cpu().numpy(), dbg[0]['cons']
    assert dbg[0]['guards_ok'] and np.isfinite(T).all() and T.shape[0] == cons.shape[0]
    fitted = skipped = reflections = 0
    rows, worst = [], 0.0
    for h in range(T.shape[0]):
        R = T[h, :, :3]
        assert _ortho(R) <= 64 * EPS and abs(np.linalg.det(R) - 1.0) <= 64 * EPS, h
        members = cons[h][cons[h] >= 0]
        if members.size < 3:
            continue
        fitted += 1
        ref = _sc2_reference(idx, members.tobytes())
        ill, gap = C.sc2_posedness(ref['S'], ref['det'])
        if ill:
            skipped += 1
            continue
        reflections += ref['det'] < 0
        rows.append((h, ref, gap))
    # LAPACK's figure on the same sets, in the same units
    lap = max([PO.diff(_lapack(ref['H'])[1], ref['mp']['Rp']) / (EPS * ref['S'][0] / gap) for _, ref, gap in rows], default=0.0)
    bar = max(FLOOR, lap)
    for h, ref, gap in rows:
        members = cons[h][cons[h] >= 0]
        bH = C.reduction_bars(dict(k0=case.P, k1=case.Q, w=None, rows=members, M=members.size, form='none'), ref)[0]
        bound = 2 * np.linalg.norm(bH) / gap + bar * EPS * ref['S'][0] / gap
        err = PO.diff(T[h, :, :3], ref['mp']['Rp'])
        worst = max(worst, err / bound)
        assert err <= bound, (h, err, bound, ref['S'], ref['det'])
    print(f'{case.name}: {fitted} fitted rows, {skipped} ill posed, {reflections} with a reflection fixed, largest error / bound {worst:.3f}, '
          f'closing bar {bar:.2f} (LAPACK {lap:.2f})')
    assert skipped <= C.SC2_SKIP_CAP * max(fitted, 1)
    if case.name.startswith('near-planar'):
        assert reflections >= 8


@functools.lru_cache(maxsize=None)
def _sc2_reference(idx, member_bytes):
    case = SC2_CASES[idx]
    return PO.kabsch(case.P, case.Q, None, np.frombuffer(member_bytes, np.int32))
