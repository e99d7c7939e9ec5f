"""Surface normals and point-to-plane ICP on the device (csrc/icp.hip, "v6d") against their numpy restatement
(tests/_icp_plane_oracle.py).  The input families are tests/_icp_plane_cases.py; tests/test_icp_plane_oracle.py asserts on the CPU that each
family meets the conditions that make it exercise its branch.  GPU only."""
import filecmp
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import _icp_cases as C
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
from roreg_amd import synth

pytestmark = pytest.mark.gpu


def _dev(T):
    return torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()


def _grid(p, d):
    from roreg_amd import hip
    return hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _status(s):
    from roreg_amd import hip
    return [hip.ICP_STATUS[int(v)] for v in s.cpu().numpy()]


def _table(p, r, grid_dist=None, k=PC.MIN_NB):
    from roreg_amd import hip
    return hip.icp_normals(_grid(p, r if grid_dist is None else grid_dist), r, k).cpu().numpy()


def _normal_bound(lam):
    """The angle a backward-stable eigen-solver may be off by: the eigenvector of lambda_min moves by |dC| / (lambda_mid - lambda_min), both
    solvers (Jacobi on the device, LAPACK here) and the two summation orders perturb C by a few tens of eps lambda_max at most."""
    return 1e-12 * lam[:, 2] / (lam[:, 1] - lam[:, 0])


def _check_normals(got, ref, name):
    """Counts and validity flags equal; on valid rows with a gap ratio >= 1e-3 the angle to the oracle's normal, up to sign, within
    _normal_bound; invalid rows zero -> (worst fraction of the bound, share of the valid rows left out by the gap rule)."""
    assert got.shape == ref.table.shape and got.dtype == np.float64
    assert np.array_equal(got[:, 3], ref.counts.astype(np.float64)), name
    valid = (got[:, :3] != 0).any(1)
    assert np.array_equal(valid, ref.valid), (name, np.flatnonzero(valid != ref.valid)[:8])
    assert (got[~valid, :3] == 0).all()
    if not valid.any():
        return 0.0, 0.0
    assert np.abs((got[valid, :3] ** 2).sum(1) - 1.0).max() <= 1e-15
    ok = valid & (PO.gap_ratio(ref.lam) >= 1e-3)
    left_out = 1.0 - ok.sum() / valid.sum()
    if not ok.any():
        return 0.0, left_out
    frac = PO.angle_to(got[ok, :3], ref.normals[ok]) / _normal_bound(ref.lam[ok])
    print(f'{name}: {int(valid.sum())} valid of {got.shape[0]}, {left_out * 100:.4f} % left out by the gap rule, worst angle = {frac.max():.3e} of its bound')
    assert frac.max() <= 1.0, name
    return float(frac.max()), left_out


def _check_against(want, T, iters, inliers, rmse, status, assign=None, name='', tol=1e-9):
    """The bar of the point method's full runs: reordered float64 sums are worth ~1e-11 relative, the 6x6 problem's conditioning (about 7
    on these scenes) stays well below the factor 100 allowed for; an assignment flips only if a point sits within ~1e-13 of a tie."""
    print(f'{name}: device {iters} iterations, {inliers} inliers, rmse {rmse}, {status}; oracle {want.iters}, {want.inliers}, {want.rmse}, {want.status}; '
          f'max |T - T_oracle| = {np.abs(T - want.T).max():.3e}')
    assert (iters, status, inliers) == (want.iters, want.status, want.inliers), name
    assert np.abs(T - want.T).max() <= tol, name
    assert abs(rmse - want.rmse) <= tol or (np.isnan(rmse) and np.isnan(want.rmse)), name
    if assign is not None and want.assign is not None:
        assert np.array_equal(assign, want.assign), name


# ---- normals ---------------------------------------------------------------------------------------------------------------------------------
def test_dense_cloud_counts_normals_and_repeatability():
    """30,000 points with sixty duplicated rows at r = 0.1: the counts are the oracle's, the validity flags too, the normals agree with
    eigh within 1e-12 lambda_max / (lambda_mid - lambda_min); two runs and the grids built for r, 2 r and r / 2 give the same bytes."""
    p, ref = PC.dense_cloud(), PC.dense_reference()
    got = _table(p, PC.DENSE_R)
    worst, left_out = _check_normals(got, ref, 'dense')
    assert left_out <= 0.01
    assert _same_bits(got, _table(p, PC.DENSE_R))
    for gd in (2 * PC.DENSE_R, PC.DENSE_R / 2):
        other = _table(p, PC.DENSE_R, gd)
        print(f'grid built for {gd}: {int((other != got).any(1).sum())} rows differ')
        assert _same_bits(got, other)


@pytest.mark.parametrize('base', PC.LAT_BASES)
def test_lattice_membership_at_the_exact_radius_and_grid_independence(base):
    """Neighbours at exactly d2 == r^2 across a cell face and across a cell corner are counted, one float32 step beyond they are not: the
    counts equal the brute-force oracle's from grids built for r, 2 r and r / 2, and the three tables and a second run are the same bytes."""
    p, kind, owner = PC.lattice_case(base)
    ref = PC.lattice_reference(base)
    tabs = [_table(p, PC.LAT_R, gd) for gd in PC.LAT_GRID_DISTS]
    for gd, t in zip(PC.LAT_GRID_DISTS, tabs):
        bad = np.flatnonzero(t[:, 3] != ref.counts)
        print(f'base {base}, grid for {gd}: {bad.size} counts differ, kinds {np.bincount(kind[bad], minlength=5)}')
        assert bad.size == 0
        _check_normals(t, ref, f'lattice base {base}, grid for {gd}')
    assert (tabs[0][:27, 3] == 31).all()
    assert _same_bits(tabs[0], tabs[1]) and _same_bits(tabs[0], tabs[2])
    assert _same_bits(tabs[0], _table(p, PC.LAT_R, PC.LAT_GRID_DISTS[0]))


def test_normals_of_small_and_degenerate_clouds():
    from roreg_amd import hip
    for n in PC.SMALL_N:
        p = PC.small_cloud(n)
        _check_normals(_table(p, PC.SMALL_R), PO.normals_full(p, PC.SMALL_R), f'{n} points')
    p6 = PC.small_cloud(6)
    assert (_table(p6, 10.0)[:, 3] == 6).all() and (_table(p6, 10.0)[:, :3] != 0).any(1).all()        # m == k is valid
    assert not (_table(p6, 10.0, k=7)[:, :3] != 0).any()
    t = _table(PC.copies_cloud(), PC.SMALL_R)
    assert (t[:, 3] == 50).all() and (t[:, :3] == 0).all()
    t = _table(PC.collinear_cloud(), PC.SMALL_R)
    assert np.array_equal(t[:, 3], PO.normals_full(PC.collinear_cloud(), PC.SMALL_R).counts) and (t[:, 3] >= PC.MIN_NB).all() and (t[:, :3] == 0).all()
    for p, nrm in PC.coplanar_clouds():
        t = _table(p, PC.SMALL_R)
        assert np.array_equal(t[:, 3], PO.normals_full(p, PC.SMALL_R).counts)
        ang = PO.angle_to(t[:, :3], np.broadcast_to(nrm, (p.shape[0], 3)))
        print('coplanar lattice: worst angle to the exact normal', ang.max())
        assert ang.max() <= 1e-15
    assert hip.icp_normals(_grid(np.zeros((0, 3), np.float32), 0.1), 0.1).shape == (0, 4)
    bad = PC.small_cloud(65).copy(); bad[7, 1] = np.nan
    with pytest.raises(hip.HipError):
        _grid(bad, PC.SMALL_R)
    with pytest.raises(hip.HipError):
        hip.icp_normals(_grid(p6, 0.1), float('nan'))


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', PC.TIE_DISTS)
def test_one_plane_iteration_from_a_given_transform(d):
    """max_iter = 1 on the pair with planted ties, normals of radius 2 d computed on the device: n_valid and the assignments equal the
    oracle's, c, A and b agree to 1e-12 of their largest entry."""
    from roreg_amd import hip
    p0, p1, T0 = PC.tie_pair()
    want = PC.tie_reference(d)
    g0 = _grid(p0, d)
    nrm = hip.icp_normals(g0, 2 * d)
    _check_normals(nrm.cpu().numpy(), PC.tie_normals(d), f'tie pair, radius {2 * d}')
    T, iters, inl, rmse, status, assign, stats = hip.icp_plane_batch([(g0, _grid(p1, d), nrm, _dev(T0))], d, max_iter=1, want_assign=True, want_stats=True)
    assign = assign[0].cpu().numpy(); stats = stats[0].cpu().numpy()
    print(f'd = {d}: n_valid {int(inl[0])} (oracle {want["n_valid"]} of {want["n"]} distance inliers), {int((assign != want["assign"]).sum())} assignments differ')
    assert np.array_equal(assign, want['assign'])
    assert int(inl[0]) == want['n_valid'] == int(stats[0]) and int(iters[0]) == 1
    c, A, b = stats[1:4], stats[4:25], stats[25:31]
    err = (np.abs(c - want['c']).max() / np.abs(want['c']).max(), np.abs(A - PO.upper(want['A'])).max() / np.abs(want['A']).max(),
           np.abs(b - want['b']).max() / np.abs(want['b']).max())
    print('relative differences of c, A, b:', err)
    assert max(err) <= 1e-12
    assert abs(stats[31] - want['sum_e2']) <= 1e-12 * want['sum_e2'] and abs(float(rmse[0]) - np.sqrt(want['sum_e2'] / want['n_valid'])) <= 1e-12
    x, lam = PO.solve(want['A'], want['b'], want['n_valid'])          # the update itself: the sums' 1e-12 times cond(A) (about 7)
    Rn, tn = PO.update(T0[:3, :3], T0[:3, 3], want['c'], x)
    Td = T[0].cpu().numpy()
    assert np.abs(Td[:3, :3] - Rn).max() <= 1e-10 and np.abs(Td[:3, 3] - tn).max() <= 1e-10 and _status(status) == ['max_iter']
    assert np.abs(Td[:3, :3] @ Td[:3, :3].T - np.eye(3)).max() <= 1e-14


def test_full_plane_runs_end_at_the_oracles_transform():
    """The convergence pair from both starts, d = 0.1, normal radius 0.2: the oracle's iteration count and status, T within 1e-9; and both
    methods' distance from the ground truth."""
    from roreg_amd import icp
    p0, p1, Tg = PC.conv_pair()
    starts = PC.conv_starts()
    got = icp.refine([(p0, p1, T0) for T0 in starts], max_dist=PC.CONV_DIST, max_iter=PC.CONV_ITER, method='plane', normal_radius=PC.CONV_RADIUS)
    point = icp.refine([(p0, p1, T0) for T0 in starts], max_dist=PC.CONV_DIST, max_iter=PC.CONV_ITER)
    for s, (g, pt) in enumerate(zip(got, point)):
        want, _ = PC.conv_reference(s, PC.CONV_RADIUS, PC.CONV_ITER)
        e, ep = O.pose_error(g.T, Tg), O.pose_error(pt.T, Tg)
        print(f'start {s}: plane {g.iters} iterations, {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm from the ground truth; point {pt.iters} iterations, '
              f'{ep[0]:.4f} deg / {ep[1] * 1e3:.3f} mm')
        _check_against(want, g.T, g.iters, g.inliers, g.rmse, g.status, name=f'start {s}')
        assert g.status == 'converged' and g.iters < pt.iters


def test_cycle_case_runs_to_max_iter():
    """Normal radius 0.1 from the first start: the Gauss-Newton step alternates between two assignment sets with a rotation step below
    tol_deg and a translation step above tol_t, so the run ends in max_iter; T within 1e-9 of the oracle's at max_iter = 30."""
    from roreg_amd import icp
    p0, p1, _ = PC.conv_pair()
    want, _ = PC.conv_reference(0, PC.CYCLE_RADIUS, PC.CYCLE_ITER)
    g = icp.refine(p0, p1, PC.conv_starts()[0], max_dist=PC.CONV_DIST, max_iter=PC.CYCLE_ITER, method='plane', normal_radius=PC.CYCLE_RADIUS)
    _check_against(want, g.T, g.iters, g.inliers, g.rmse, g.status, name='cycle')
    assert g.status == 'max_iter' and g.iters == PC.CYCLE_ITER


def test_rank_of_the_normal_equations():
    """One and two exact planes: no_support with T0 returned (three and one zero eigenvalues of A); three orthogonal planes: converged at the
    oracle's transform; a noisy wall: what the oracle says, within the sums' 1e-12 times the condition number of its A (about 5e4)."""
    from roreg_amd import hip
    for n in PC.RANK_PLANES:
        tgt, src, Tg, T0 = PC.planes_pair(n)
        want, trace = PC.planes_reference(n)
        g = _grid(tgt, PC.RANK_DIST)
        nrm = hip.icp_normals(g, PC.RANK_RADIUS)
        _check_normals(nrm.cpu().numpy(), PC.planes_normals(n), f'{n} planes')
        if n < 3:                                                   # exact axes: the zero eigenvalues of A are exact zeros on the device too
            assert (np.abs(nrm.cpu().numpy()[:, :3]).max(1) == 1.0).all()
        T, iters, inl, rmse, status = hip.icp_plane_batch([(g, _grid(src, PC.RANK_DIST), nrm, _dev(T0))], PC.RANK_DIST, max_iter=PC.RANK_ITER)
        _check_against(want, T[0].cpu().numpy(), int(iters[0]), int(inl[0]), float(rmse[0]), _status(status)[0], name=f'{n} planes')
        if n < 3:
            assert _status(status) == ['no_support'] and _same_bits(T[0].cpu().numpy(), T0)
        else:
            assert _status(status) == ['converged']
    for seed in PC.WALL_SEEDS:
        q, p, _, T0 = C.wall_pair(seed)
        want, trace = PC.wall_reference(seed)
        cond = max(x['lam'][-1] / x['lam'][0] for x in trace)
        g = _grid(q, C.WALL_DIST)
        nrm = hip.icp_normals(g, PC.RANK_RADIUS)
        _check_normals(nrm.cpu().numpy(), PC.wall_normals(seed), f'wall seed {seed}')
        T, iters, inl, rmse, status = hip.icp_plane_batch([(g, _grid(p, C.WALL_DIST), nrm, _dev(T0))], C.WALL_DIST, max_iter=C.WALL_ITER)
        _check_against(want, T[0].cpu().numpy(), int(iters[0]), int(inl[0]), float(rmse[0]), _status(status)[0], name=f'wall seed {seed}, cond {cond:.2e}',
                       tol=1e-12 * cond)


def test_batch_invariance_and_slot_boundaries():
    """Sources of 1, 1023, 1024, 1025 and 3073 points against a whole target: one iteration's sums within 1e-12 of the oracle's, the full
    runs at the oracle's transform; a pair alone, in a batch of seven and in reversed order gives the same bits."""
    from roreg_amd import hip
    cases = PC.chunk_pairs()
    refs = PC.chunk_reference()
    tgt = cases[0][1]
    g0 = _grid(tgt, C.CHUNK_DIST)
    nrm = hip.icp_normals(g0, PC.CHUNK_RADIUS)
    _check_normals(nrm.cpu().numpy(), PC.chunk_normals(), 'chunk target')
    batch = [(g0, _grid(p, C.CHUNK_DIST), nrm, _dev(T0)) for _, _, p, T0 in cases]
    one = hip.icp_plane_batch(batch, C.CHUNK_DIST, max_iter=1, want_assign=True, want_stats=True)
    full = hip.icp_plane_batch(batch, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True)
    for i, ((name, q, p, T0), (it, want)) in enumerate(zip(cases, refs)):
        st = one[6][i].cpu().numpy()
        assert np.array_equal(one[5][i].cpu().numpy(), it['assign']) and int(st[0]) == it['n_valid'], name
        if it['n_valid']:
            err = (np.abs(st[1:4] - it['c']).max() / np.abs(it['c']).max(), np.abs(st[4:25] - PO.upper(it['A'])).max() / np.abs(it['A']).max(),
                   np.abs(st[25:31] - it['b']).max() / np.abs(it['b']).max())
            print(name, 'relative differences of c, A, b:', err)
            assert max(err) <= 1e-12, name
        T, iters, inl, rmse = (v.cpu().numpy() for v in full[:4])
        _check_against(want, T[i], int(iters[i]), int(inl[i]), float(rmse[i]), _status(full[4])[i], full[5][i].cpu().numpy(), name)
    seven = batch + [batch[3], batch[1]]
    a = [v.cpu().numpy() for v in hip.icp_plane_batch(seven, C.CHUNK_DIST, max_iter=C.CHUNK_ITER)]
    b = [v.cpu().numpy() for v in hip.icp_plane_batch(seven[::-1], C.CHUNK_DIST, max_iter=C.CHUNK_ITER)]
    assert (a[1][1:5] > 1).all()
    for x, y in zip(a, b):
        assert _same_bits(x[::-1], y)
    for x, y in zip(a, [v.cpu().numpy() for v in full[:5]]):
        assert _same_bits(x[:5], y) and _same_bits(x[5], y[3]) and _same_bits(x[6], y[1])
    for i in (0, 3, 4):
        alone = hip.icp_plane_batch([batch[i]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER)
        for x, y in zip(a, alone):
            assert _same_bits(x[i:i + 1], y.cpu().numpy()), cases[i][0]


def test_point_method_is_untouched():
    """method='point' is the default, bit for bit; a plane call between two point calls on the same grids changes nothing in them."""
    from roreg_amd import hip, icp
    p0, p1, Tg = synth.make_dense_pair(41, 5000)
    T0 = O.perturb(Tg, 2.0, 0.03, 41)
    a = icp.refine(p0, p1, T0, max_dist=0.1, max_iter=12)
    b = icp.refine(p0, p1, T0, max_dist=0.1, max_iter=12, method='point')
    assert _same_bits(a.T, b.T) and a[1:3] == b[1:3] and a.status == b.status and _same_bits(np.float64(a.rmse), np.float64(b.rmse))
    want = O.icp(p0, p1, T0, 0.1, max_iter=12)
    assert a.iters == want.iters and a.inliers == want.inliers and np.abs(a.T - want.T).max() <= 1e-9
    g0, g1 = _grid(p0, 0.1), _grid(p1, 0.1)
    pairs = [(g0, g1, _dev(T0)), (g1, g0, _dev(np.linalg.inv(T0)))]
    before = [v.cpu().numpy() for v in hip.icp_batch(pairs, 0.1, max_iter=12)]
    plane = hip.icp_plane_batch([(g0, g1, hip.icp_normals(g0, 0.2), pairs[0][2])], 0.1, max_iter=12)
    after = [v.cpu().numpy() for v in hip.icp_batch(pairs, 0.1, max_iter=12)]
    assert int(plane[1][0]) > 1 and _status(plane[4])[0] in ('converged', 'max_iter')
    for x, y in zip(before, after):
        assert _same_bits(x, y)
    with pytest.raises(ValueError):
        icp.refine(p0, p1, T0, max_dist=0.1, method='plain')


# ---- the public surface ----------------------------------------------------------------------------------------------------------------------
def test_estimate_normals_and_the_engines_cache():
    from roreg_amd import hip, icp
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    p0, p1, Tg = synth.make_dense_pair(43, 6000)
    nrm, valid, counts = icp.estimate_normals(p0, 0.2)
    assert nrm.shape == (6000, 3) and nrm.dtype == np.float64 and valid.shape == (6000,) and valid.dtype == np.bool_
    assert counts.shape == (6000,) and np.issubdtype(counts.dtype, np.integer)
    ref = PO.normals(p0, 0.2)
    assert np.array_equal(counts, ref.counts) and np.array_equal(valid, ref.valid)
    assert (nrm[~valid] == 0).all() and np.abs((nrm[valid] ** 2).sum(1) - 1).max() <= 1e-15
    assert np.array_equal(icp.estimate_normals(p0, 0.2, min_neighbors=40)[1], ref.counts >= 40)
    # the engine: the same bits as icp.refine, normals computed once per (cloud, radius, min_neighbors)
    T0 = O.perturb(Tg, 2.0, 0.03, 43)
    eng = RegistrationEngine(default_config(), None, None)
    c0, c1 = (eng.attach_points(CloudState(before=None), p) for p in (p0, p1))
    items = [(c0, c1, _dev(T0)), (c1, c0, _dev(np.linalg.inv(T0)))]
    out = eng.icp_many(items, 0.1, 20, method='plane')
    assert set(c0.normals) == {(0.2, 6)} and set(c1.normals) == {(0.2, 6)} and len(c0.grids) == 1
    ptr = c0.normals[(0.2, 6)].data_ptr()
    out2 = eng.icp_many(items, 0.1, 20, method='plane')
    assert c0.normals[(0.2, 6)].data_ptr() == ptr and len(c0.normals) == 1
    eng.icp_many(items[:1], 0.1, 20, method='plane', normal_radius=0.15)
    assert set(c0.normals) == {(0.2, 6), (0.15, 6)} and set(c1.normals) == {(0.2, 6)}
    want = icp.refine([(p0, p1, T0), (p1, p0, np.linalg.inv(T0))], max_dist=0.1, max_iter=20, method='plane')
    for x, y in zip(out, out2):
        assert torch.equal(x, y)
    got = icp.results_to_host(*out)
    for g, w in zip(got, want):
        assert _same_bits(g.T, w.T) and g[1:3] == w[1:3] and g.status == w.status and _same_bits(np.float64(g.rmse), np.float64(w.rmse))
    assert got[0].iters > 1 and got[0].status in ('converged', 'max_iter')
    with pytest.raises(ValueError):
        eng.icp_many(items, 0.1, method='planar')


def test_run_scene_carries_the_plane_refinement(tmp_path):
    from test_hip_icp import _cfg_and_nets, _dense_scene
    from roreg_amd import icp
    from roreg_amd.engine import RegistrationEngine
    z = load_golden('pipeline_mutual_yohoo')
    cfg, gf, et = _cfg_and_nets(tmp_path, z, ET='yohoo')
    keynum = int(z['keynum'])
    ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
    dense = _dense_scene(ds, 8000, 31)
    keys = [ds.get_kps(i) for i in ds.pc_ids]
    opts = dict(max_dist=0.1, max_iter=20, method='plane', normal_radius=0.2)
    eng = RegistrationEngine(cfg, gf, et)
    np.random.seed(99)
    ready = {}
    res = eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=keynum, max_iter=1000, points=dense, icp=opts, ready=ready)
    want = icp.refine([(dense[int(r.id0)], dense[int(r.id1)], r.trans) for r in res], **opts)
    for r, w in zip(res, want):
        print(r.id0, r.id1, r.icp_iters, r.icp_inliers, r.icp_rmse, r.icp_status)
        assert _same_bits(r.trans_icp, w.T) and (r.icp_iters, r.icp_inliers, r.icp_status) == (w.iters, w.inliers, w.status)
        assert _same_bits(np.float64(r.icp_rmse), np.float64(w.rmse))
    assert any(r.icp_iters >= 1 for r in res)
    assert all(len(c.normals) <= 1 for c in ready.values()) and any(len(c.normals) == 1 for c in ready.values())


def test_run_distributed_writes_the_plane_block_beside_unchanged_outputs(tmp_path):
    """run_distributed.evaluate at world size 1 on two synthetic scenes, once with the point and once with the plane method: the {ET}/
    files and the first results.log block are the same bytes in both; the plane run writes {ET}_icp_plane/ and an '-icp-plane' block (and
    no {ET}_icp/), its table holds icp.refine(method='plane')'s results."""
    from test_hip_icp import _cfg_and_nets, _dense_scene
    from roreg_amd import distributed as D, icp, run_distributed as RD_
    from roreg_amd.engine import RegistrationEngine
    z = load_golden('pipeline_mutual_yohoo')
    outs, cfgs, scenes = {}, {}, {}
    for kind, opts in (('point', dict(max_dist=0.1, max_iter=15)), ('plane', dict(max_dist=0.1, max_iter=15, method='plane', normal_radius=0.2))):
        root = tmp_path / kind
        root.mkdir()
        cfg, gf, et = _cfg_and_nets(root, z, ET='yohoo', testset='synth')
        datasets = {'wholesetname': 'synth'}
        for k in range(2):
            ds = synth.make_scene(int(z['scene_seed']) + k, n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name=f'synth/scene{k}')
            ds.write_inputs(cfg.output_cache_fn)
            ds.gt_dir = f'{root}/nonexistent/{ds.name}/gt.log'
            dense = _dense_scene(ds, 6000, 31 + k)
            ds.get_pc = lambda i, dense=dense: dense[int(i)]
            datasets[f'scene{k}'] = ds
            scenes[k] = (ds, dense)
        outs[kind] = RD_.evaluate(cfg, datasets, RegistrationEngine(cfg, gf, et), rank=0, world=1, seed=3, icp=opts)
        cfgs[kind] = (cfg, opts)
    point, plane = outs['point'], outs['plane']
    for k in set(point) - {'icp'}:
        assert point[k] == plane[k] or (np.isnan(point[k]) and np.isnan(plane[k])), k
    log0 = open(f'{cfgs["point"][0].base_dir}/results.log').read().splitlines(); log1 = open(f'{cfgs["plane"][0].base_dir}/results.log').read().splitlines()
    assert len(log0) == len(log1) == 11 and log0[:7] == log1[:7]
    assert log0[7] == log0[0] + '-icp' and log1[7] == log0[0] + '-icp-plane' and log1[10].startswith('registration recall(pointdsc)')
    rows = {(r['scene'], r['id0'], r['id1']): r for r in D.unpack_rows(plane['icp']['table'])}
    for k, (ds, dense) in scenes.items():
        d0, d1 = (f'{cfgs[kind][0].output_cache_fn}/{ds.name}/match_{cfgs[kind][0].keynum}' for kind in ('point', 'plane'))
        sub = f'yohoo/{cfgs["point"][0].max_iter}iters'
        files = sorted(os.listdir(f'{d0}/{sub}'))
        assert files == sorted(os.listdir(f'{d1}/{sub}')) and len(files) == len(ds.pair_ids) + 1
        for f in files:
            if f.endswith('.npz'):
                a, b = np.load(f'{d0}/{sub}/{f}'), np.load(f'{d1}/{sub}/{f}')
                assert _same_bits(a['trans'], b['trans']) and int(a['recalltime']) == int(b['recalltime'])
            else:
                assert filecmp.cmp(f'{d0}/{sub}/{f}', f'{d1}/{sub}/{f}', shallow=False)
        assert os.path.isdir(f'{d0}/yohoo_icp') and not os.path.exists(f'{d0}/yohoo_icp_plane')
        assert os.path.isdir(f'{d1}/yohoo_icp_plane') and not os.path.exists(f'{d1}/yohoo_icp')
        coarse = {f[:-4]: np.load(f'{d1}/{sub}/{f}')['trans'] for f in files if f.endswith('.npz')}
        want = icp.refine([(dense[int(a)], dense[int(b)], coarse[f'{a}-{b}']) for a, b in ds.pair_ids], **cfgs['plane'][1])
        sub_icp = f'yohoo_icp_plane/{cfgs["plane"][0].max_iter}iters'
        for (a, b), w in zip(ds.pair_ids, want):
            row = rows[(k, a, b)]
            assert _same_bits(row['trans'][:3], w.T[:3]) and row['n_match'] == w.inliers and row['recalltime'] == w.iters
            f = np.load(f'{d1}/{sub_icp}/{a}-{b}.npz')
            assert _same_bits(f['trans'][:3], w.T[:3]) and int(f['recalltime']) == w.iters and int(f['inliers']) == w.inliers
        assert os.path.exists(f'{d1}/{sub_icp}/pre.log')
    assert plane['icp']['pairs'] == sum(len(ds.pair_ids) for ds, _ in scenes.values())
