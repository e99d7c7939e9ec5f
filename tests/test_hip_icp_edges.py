"""Dense ICP on the device (csrc/icp.hip) at its edges, against the numpy restatement (tests/_icp_oracle.py): the 3x3 solve across
conditioning and both determinant signs, the grid build at the boundaries of its three-launch scan, source and target counts at the
wave / workgroup / slot boundaries, queries at exactly max_dist and one float32 step beyond across cell faces and corners, the determinant
fix inside full runs, and the parameters' ends.  The input families are tests/_icp_cases.py; tests/test_icp_oracle.py asserts on the CPU
that each family meets the conditions that make it exercise its branch.  GPU only."""
import numpy as np
import pytest
import torch

import _icp_cases as C
import _icp_oracle as O

pytestmark = pytest.mark.gpu


def _dev(T):
    return torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()


def _grid(p, d, box=None):
    from roreg_amd import hip
    return hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d, box=box)


def _box(p):
    return np.stack([p.min(0), p.max(0)]).astype(np.float64)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _status(s):
    from roreg_amd import hip
    return [hip.ICP_STATUS[int(v)] for v in s.cpu().numpy()]


def _proper(R, tol=1e-12):
    return np.abs(R @ R.T - np.eye(3)).max() <= tol and abs(np.linalg.det(R) - 1.0) <= tol


def _check_against(want, T, iters, inliers, rmse, status, assign=None, name=''):
    """The bar of test_hip_icp.py::test_full_runs_end_at_the_oracles_transform: a float64 sum of <= 1e5 terms reordered is worth ~1e-11
    relative, times <= 100 for the conditioning of the 3x3 problem; an assignment flips only if a point sits within ~1e-13 of the threshold
    or of a tie -- a larger difference is a wrong assignment, not a loose tolerance."""
    print(f'{name}: device {iters} iterations, {inliers} inliers, rmse {rmse}, {status}; oracle {want.iters}, {want.inliers}, {want.rmse}, {want.status}; '
          f'max |T - T_oracle| = {np.abs(T - want.T).max():.3e}')
    assert (iters, status, inliers) == (want.iters, want.status, want.inliers), name
    assert np.abs(T - want.T).max() <= 1e-9, name
    assert abs(rmse - want.rmse) <= 1e-9 or (np.isnan(rmse) and np.isnan(want.rmse)), name
    if assign is not None and want.assign is not None:
        assert np.array_equal(assign, want.assign), name


# ---- A: the 3x3 solve ----------------------------------------------------------------------------------------------------------------------
def test_solve_across_conditioning_and_both_determinant_signs():
    """256 pairs of 3..8 points in one batch, one iteration each: status, iters and inliers are the oracle's; where the oracle solves,
    max |R - R_ref| <= 1e-12 sigma1 / gap with gap = sigma2 + sign(det U V^T) sigma3 of the oracle's H, |t - t_ref| within the same bound
    times (1 + |c_p|), and R is a proper rotation to 1e-12.  The bound is derived (C.solve_bound), not fitted: the rotation factor moves by
    <= 2 |dH| / gap and both solvers are backward stable to a few tens of eps |H|."""
    from roreg_amd import hip
    pairs, refs, _ = C.solve_family()
    batch = [(_grid(c['Q'], C.SOLVE_DIST, _box(c['Q'])), _grid(c['P'], C.SOLVE_DIST, _box(c['P'])), _dev(c['T0'])) for c in pairs]
    T, iters, inl, rmse, status, stats = hip.icp_batch(batch, C.SOLVE_DIST, max_iter=1, want_stats=True)
    T, iters, inl, stats, status = T.cpu().numpy(), iters.cpu().numpy(), inl.cpu().numpy(), stats.cpu().numpy(), _status(status)
    worst = (0.0, 0.0)
    bad = []
    for i, (c, r) in enumerate(zip(pairs, refs)):
        tag = (i, c['family'], c['mirrored'], c['decade'])
        assert status[i] == r['status'] and iters[i] == 1 and inl[i] == r['it']['n'] == int(stats[i, 0]), tag
        H = stats[i, 7:16].reshape(3, 3)
        assert np.abs(H - r['it']['H']).max() <= 1e-12 * np.abs(r['it']['H']).max(), tag        # the sums' bar of test_one_iteration_from_a_given_transform
        if r['R'] is None:
            assert _same_bits(T[i], c['T0']), tag
            continue
        bound = C.solve_bound(r)
        eR = np.abs(T[i, :3, :3] - r['R']).max()
        et = np.abs(T[i, :3, 3] - r['t']).max()
        cp = np.sqrt((r['it']['cp'] ** 2).sum())
        worst = max(worst, (eR / bound, et / (bound * (1 + cp))))
        if not (eR <= bound and et <= bound * (1 + cp) and _proper(T[i, :3, :3]) and np.array_equal(T[i, 3], [0, 0, 0, 1])):
            bad.append((tag, eR, et, bound, r['S'], r['sign']))
    print(f'largest |R - R_ref| and |t - t_ref| as fractions of their bounds: {worst[0]:.3f}, {worst[1]:.3f}')
    assert not bad, bad


@pytest.mark.parametrize('k', [40, -40])
def test_solve_does_not_depend_on_the_scale_of_the_clouds(k):
    """The solve family with both clouds, the start's translation and max_dist times 2^k (exact in float32 and float64, so every sum is the
    unscaled run's times a power of two, H's by 2^2k): status, iterations and inliers are the unscaled run's, R the same bits, t the same
    bits times 2^k.  kabsch_rotation scales the largest entry's power of two out of H before its sweeps (as csrc/polar.h polar_uvt does)."""
    from roreg_amd import hip
    pairs, _, _ = C.solve_family()
    s = np.float32(2.0) ** k

    def run(scale):
        batch = []
        for c in pairs:
            T0 = c['T0'].copy(); T0[:3, 3] *= float(scale)
            Q, P = c['Q'] * scale, c['P'] * scale
            assert np.isfinite(Q).all() and np.isfinite(P).all()
            batch.append((_grid(Q, C.SOLVE_DIST * float(scale), _box(Q)), _grid(P, C.SOLVE_DIST * float(scale), _box(P)), _dev(T0)))
        T, iters, inl, rmse, status = hip.icp_batch(batch, C.SOLVE_DIST * float(scale), max_iter=1, tol_t=1e-6 * float(scale))      # (a length too)
        return T.cpu().numpy(), iters.cpu().numpy(), inl.cpu().numpy(), _status(status)

    base, scaled = run(np.float32(1.0)), run(s)
    assert np.array_equal(base[1], scaled[1]) and np.array_equal(base[2], scaled[2]) and base[3] == scaled[3]
    assert sum(v != 'no_support' for v in base[3]) >= 100
    assert _same_bits(base[0][:, :3, :3], scaled[0][:, :3, :3])
    assert _same_bits(np.ldexp(base[0][:, :3, 3], k), scaled[0][:, :3, 3])


# ---- B: the grid build at the scan's boundaries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', C.GRID_DIMS)
def test_grid_is_a_counting_sort_at_the_scan_boundaries(dims):
    """The records are the points in (cell, original row) order, the starts are concatenate([0], cumsum(bincount)), a second build gives
    the same bytes: with cells + 1 on either side of one scan block (4096), block counts on either side of 256, and the 2^24-cell maximum."""
    p, box = C.grid_case(dims)
    g = _grid(p, 1.0, box)
    assert g.dims == dims and g.edge == 1.0
    order, starts, _ = C.grid_expected(p, g.desc['origin'][0], 1.0, dims)
    xyz, rows = (t.cpu().numpy() for t in g.records())
    got = g.cell_starts().cpu().numpy()
    assert got.shape == starts.shape and got[0] == 0 and got[-1] == p.shape[0]
    wrong = np.flatnonzero(got != starts)
    assert wrong.size == 0, (wrong[:8], got[wrong[:8]], starts[wrong[:8]])
    assert np.array_equal(rows, order) and _same_bits(xyz, p[order])
    assert torch.equal(g.buf, _grid(p, 1.0, box).buf)
    hdr = g.buf[:64].cpu().numpy()
    assert hdr.tobytes() == g.desc.tobytes()


# ---- C: counts at the chunk and wave boundaries ----------------------------------------------------------------------------------------------
def test_counts_at_the_wave_workgroup_and_slot_boundaries():
    """Sources of 1 .. 3073 points against a 4000-point target and targets of 1 .. 1025 points against a 4000-point source, one batch: the
    oracle's iterations, status, inliers, transform, rmse and last assignments; three of the pairs alone are bit-identical to the batch."""
    from roreg_amd import hip
    cases, refs = C.chunk_pairs(), C.chunk_reference()
    grids = {}

    def grid(p):
        key = (p.ctypes.data, p.shape[0])
        if key not in grids:
            grids[key] = _grid(p, C.CHUNK_DIST)
        return grids[key]

    batch = [(grid(q), grid(p), _dev(T0)) for _, q, p, T0 in cases]
    out = hip.icp_batch(batch, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True)
    T, iters, inl, rmse = (v.cpu().numpy() for v in out[:4])
    status = _status(out[4])
    for i, ((name, q, p, _), want) in enumerate(zip(cases, refs)):
        a = out[5][i].cpu().numpy()
        assert a.shape == (p.shape[0],)
        _check_against(want, T[i], int(iters[i]), int(inl[i]), float(rmse[i]), status[i], a, name)
    names = [c[0] for c in cases]
    for name in ('src65', 'src1025', 'tgt64'):
        i = names.index(name)
        alone = hip.icp_batch([batch[i]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True)
        for x, y in zip(out[:5], alone[:5]):
            assert _same_bits(x[i:i + 1].cpu().numpy(), y.cpu().numpy()), name
        assert torch.equal(out[5][i], alone[5][0]), name


# ---- D: the inclusive threshold and the search box -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid_dist', C.THR_GRID_DISTS)
@pytest.mark.parametrize('base', C.THR_BASES)
def test_exact_threshold_across_cell_faces_and_corners(base, grid_dist):
    """Queries at d2 == d^2 exactly are inliers of the target across the cell face, one float32 step further they are not; corner queries
    fall on the side the float64 brute-force search puts them; an exact tie at the threshold goes to the lowest row.  Every assignment and
    the inlier count equal O.nearest_full's, with grids built for d, 2 d and d / 2."""
    from roreg_amd import hip
    Q, P, kind = C.threshold_case(base)
    want, _ = C.threshold_reference(base)
    T, iters, inl, rmse, status, assign = hip.icp_batch([(_grid(Q, grid_dist), _grid(P, grid_dist), _dev(np.eye(4)))], C.THR_DIST, max_iter=1, want_assign=True)
    got = assign[0].cpu().numpy()
    diff = np.flatnonzero(got != want)
    print(f'base {base}, grids for {grid_dist}: {int(inl[0])} inliers (oracle {int((want >= 0).sum())}), {diff.size} assignments differ, kinds {np.bincount(kind[diff], minlength=4)}')
    assert diff.size == 0, (diff[:8], got[diff[:8]], want[diff[:8]], kind[diff[:8]])
    assert int(inl[0]) == int((want >= 0).sum()) and int(iters[0]) == 1
    ref = O.icp(Q, P, np.eye(4), C.THR_DIST, max_iter=1, nn=O.nearest_full)
    _check_against(ref, T[0].cpu().numpy(), int(iters[0]), int(inl[0]), float(rmse[0]), _status(status)[0], got, f'base {base}')


# ---- E: the determinant fix inside a full run ------------------------------------------------------------------------------------------------
def test_noisy_wall_runs_pass_through_the_determinant_fix():
    """A noisy planar scan: H's third singular value is at the noise level and det(U V^T) = -1 in some iterations of the oracle's run
    (asserted on the CPU for these seeds).  The full run ends at the oracle's transform, a proper rotation."""
    from roreg_amd import hip
    batch, refs = [], []
    for seed in C.WALL_SEEDS:
        q, p, _, T0 = C.wall_pair(seed)
        batch.append((_grid(q, C.WALL_DIST), _grid(p, C.WALL_DIST), _dev(T0)))
        refs.append(C.wall_reference(seed))
    out = hip.icp_batch(batch, C.WALL_DIST, max_iter=C.WALL_ITER, want_assign=True)
    T, iters, inl, rmse = (v.cpu().numpy() for v in out[:4])
    status = _status(out[4])
    for i, (seed, want) in enumerate(zip(C.WALL_SEEDS, refs)):
        _check_against(want, T[i], int(iters[i]), int(inl[i]), float(rmse[i]), status[i], out[5][i].cpu().numpy(), f'wall seed {seed}')
        assert _proper(T[i, :3, :3])


# ---- F: parameters and degenerate clouds -----------------------------------------------------------------------------------------------------
def test_parameter_ends_and_identical_points():
    from roreg_amd import hip, synth
    p0, p1, Tg = synth.make_dense_pair(61, 1500)
    d = 0.1
    T0 = O.perturb(Tg, 1.0, 0.02, 61)
    g0, g1 = _grid(p0, d), _grid(p1, d)

    def run(**kw):
        out = hip.icp_batch([(g0, g1, _dev(T0))], d, want_assign=True, **kw)
        return out[0][0].cpu().numpy(), int(out[1][0]), int(out[2][0]), float(out[3][0]), _status(out[4])[0], out[5][0].cpu().numpy()

    # max_iter = 0: nothing runs
    T, iters, inl, rmse, status, assign = run(max_iter=0)
    assert _same_bits(T, T0) and (iters, inl, status) == (0, 0, 'max_iter') and np.isnan(rmse)
    assert assign.shape == (1500,) and (assign == -1).all()
    want = O.icp(p0, p1, T0, d, max_iter=0)
    assert (want.iters, want.inliers, want.status) == (0, 0, 'max_iter') and np.isnan(want.rmse) and np.array_equal(want.T, T0)
    # huge tolerances: converged at the first iteration
    want = O.icp(p0, p1, T0, d, max_iter=10, tol_deg=1e9, tol_t=1e9)
    assert want.status == 'converged' and want.iters == 1
    _check_against(want, *run(max_iter=10, tol_deg=1e9, tol_t=1e9), name='huge tolerances')
    # zero tolerances: nothing is below them, max_iter is reached
    want = O.icp(p0, p1, T0, d, max_iter=6, tol_deg=0.0, tol_t=0.0)
    assert want.status == 'max_iter' and want.iters == 6
    _check_against(want, *run(max_iter=6, tol_deg=0.0, tol_t=0.0), name='zero tolerances')
    # non-default tolerances in between stop at the oracle's iteration, earlier than the defaults
    want = O.icp(p0, p1, T0, d, max_iter=30, tol_deg=0.05, tol_t=1e-3)
    full = O.icp(p0, p1, T0, d, max_iter=30)
    assert want.status == 'converged' and 1 < want.iters < full.iters
    _check_against(want, *run(max_iter=30, tol_deg=0.05, tol_t=1e-3), name='loose tolerances')
    # fifty copies of one point against themselves: H = 0
    one = np.repeat(np.float32([[0.3, -1.2, 2.5]]), 50, 0)
    Ts = O.perturb(np.eye(4), 0.5, 0.01, 62)
    want = O.icp(one, one, Ts, d, max_iter=5)
    assert (want.status, want.inliers, want.iters) == ('no_support', 50, 1) and np.array_equal(want.T, Ts)
    go = _grid(one, d)
    out = hip.icp_batch([(go, go, _dev(Ts))], d, max_iter=5, want_assign=True)
    got = (out[0][0].cpu().numpy(), int(out[1][0]), int(out[2][0]), float(out[3][0]), _status(out[4])[0], out[5][0].cpu().numpy())
    _check_against(want, *got, name='identical points')
    assert _same_bits(got[0], Ts) and (got[5] == 0).all()


# ---- G: a restructuring of csrc/icp.hip changes no bit ---------------------------------------------------------------------------------------
def test_refactor_keeps_the_parents_bits():
    """tests/golden/icp_parent_bits.npz holds every tensor that the case set of tools/record_icp_bits.py returned from the kernels of the
    commit named inside it (the last one before the point and plane drivers were merged into one skeleton): chunk-boundary batches of both
    methods forward and reversed, the solve family, the walls, the plane rank family, a non-finite T0, an empty source, and the pair
    evaluation with its assignments.  The current library must return the same bits: np.array_equal on every array, floats compared as
    their integer patterns, no tolerance, no case left out (the fixture is small enough to hold every assignment array).  The hash names
    the fixture's origin for a reader; nothing here can verify it."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import record_icp_bits as rec
    want = np.load(rec.FIXTURE)
    got = rec.run_cases()
    assert len(str(want['commit'])) == 40
    assert sorted(got) == sorted(k for k in want.files if k != 'commit')
    differ = [k for k in sorted(got) if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    assert not differ, differ
