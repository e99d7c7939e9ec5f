"""Robust losses in the point-to-plane and plane-to-plane ICP on the device (csrc/icp.hip, "v6p") against their numpy definition
(tests/_icp_robust_oracle.py).  The input families are tests/_icp_robust_cases.py; tests/test_icp_robust_oracle.py asserts on the CPU that
each family meets the conditions that make it exercise what it is here for.  One-iteration sums are compared with the oracle run on the
device's own normal tables (hip.icp_normals, pinned to its oracle by tests/test_hip_icp_plane.py): exact in their inputs.  Full runs are
compared with the families' cached references (numpy normals, as tests/test_hip_icp_plane.py does).  Tolerances are those of
tests/test_hip_icp_plane.py for the same sums: c, A and b within 1e-12 of their largest entry, sum e^2 within 1e-12 of itself, T within 1e-9
(the walls: 1e-12 x cond(A)).  GPU only."""
import numpy as np
import pytest
import torch

import _icp_cases as C
import _icp_gicp_cases as GC
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
import _icp_robust_cases as RC

pytestmark = pytest.mark.gpu

_TABLES, _GRIDS = {}, {}


def _dev(T):
    return torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()


def _grid(name, p, d):
    from roreg_amd import hip
    key = (name, float(d))
    if key not in _GRIDS:
        _GRIDS[key] = hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d)
    return _GRIDS[key]


def _table(name, p, radius):
    """The device's normal table of cloud `name` -> (device tensor, its host copy), computed once per (name, radius)."""
    from roreg_amd import hip
    key = (name, float(radius))
    if key not in _TABLES:
        t = hip.icp_normals(_grid(name, p, radius), radius, PC.MIN_NB)
        _TABLES[key] = (t, t.cpu().numpy())
    return _TABLES[key]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _status(s):
    from roreg_amd import hip
    return [hip.ICP_STATUS[int(v)] for v in np.asarray(s)]


def _host(out):
    return [[x.cpu().numpy() for x in v] if isinstance(v, list) else v.cpu().numpy() for v in out]


def _batch(method, pairs, d, **kw):
    """pairs [(target grid, source grid, Nq, Np, T0)] through the method's entry -> host arrays"""
    from roreg_amd import hip
    if method == 'plane':
        return _host(hip.icp_plane_batch([(g0, g1, Nq, T0) for g0, g1, Nq, Np, T0 in pairs], d, **kw))
    return _host(hip.icp_gicp_batch(list(pairs), d, **kw))


def _check_sums(stats, assign, want, name):
    """One weighted iteration's sums against the oracle's: assignments and the count equal, c, A and b within 1e-12 of their largest entry,
    the unweighted sum e^2 within 1e-12 of itself -> the worst fraction of those bounds."""
    assert np.array_equal(assign, want['assign']), name
    assert int(stats[0]) == want['n_valid'], name
    if want['n_valid'] == 0:
        assert (stats == 0).all(), name
        return 0.0
    A, b, c = PO.upper(want['A']), want['b'], want['c']
    frac = (np.abs(stats[1:4] - c).max() / (1e-12 * np.abs(c).max()), np.abs(stats[4:25] - A).max() / (1e-12 * np.abs(A).max()),
            np.abs(stats[25:31] - b).max() / (1e-12 * np.abs(b).max()), abs(stats[31] - want['sum_e2']) / (1e-12 * want['sum_e2']))
    print(f'{name}: n_valid = {want["n_valid"]}; c, A, b, sum e^2 at {frac[0]:.2e}, {frac[1]:.2e}, {frac[2]:.2e}, {frac[3]:.2e} of their 1e-12 bounds')
    assert max(frac) <= 1.0, name
    return max(frac)


def _check_against(want, T, iters, inliers, rmse, status, name, tol=1e-9):
    print(f'{name}: device {iters} iterations, {inliers} inliers, rmse {rmse}, {status}; oracle {want.iters}, {want.inliers}, {want.rmse}, {want.status}; '
          f'max |T - T_oracle| = {np.abs(T - want.T).max():.3e} (bound {tol:.1e})')
    assert (iters, status, inliers) == (want.iters, want.status, want.inliers), name
    assert np.abs(T - want.T).max() <= tol, name
    assert abs(rmse - want.rmse) <= tol or (np.isnan(rmse) and np.isnan(want.rmse)), name


def _chunk_batch():
    """-> (cases, [(target grid, source grid, Nq, Np, T0)], [(Nq host, Np host)]): the chunk family, every source with its own table"""
    cases = PC.chunk_pairs()
    g0 = _grid('chunk target', cases[0][1], C.CHUNK_DIST)
    Nq = _table('chunk target', cases[0][1], GC.CHUNK_RADIUS)
    batch, host = [], []
    for name, _, p, T0 in cases:
        Np = _table('chunk ' + name, p, GC.CHUNK_RADIUS)
        batch.append((g0, _grid('chunk ' + name, p, C.CHUNK_DIST), Nq[0], Np[0], _dev(T0)))
        host.append((Nq[1], Np[1]))
    return cases, batch, host


# ---- 1: one iteration ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', RC.LOSSES)
@pytest.mark.parametrize('method', RC.METHODS)
def test_one_weighted_iteration_from_a_given_transform(method, loss):
    """max_iter = 1 on the pair with planted ties at d = 0.1, scale 0.01 (at least a tenth of the residuals on each side of it): assignments
    and n_valid are the oracle's, the weighted A and b, c and the unweighted sum e^2 within 1e-12; the update is the oracle's solve."""
    p0, p1, T0 = PC.tie_pair()
    d = RC.ONE_DIST
    Nq, Np = _table('tie target', p0, 2 * d), _table('tie source', p1, 2 * d)
    want = RC.one_run(method, p0, p1, Nq[1], Np[1], T0, d, loss, RC.ONE_SCALE)
    inside, outside = RC.sides(want, RC.ONE_SCALE)
    assert inside >= RC.ONE_SHARE and outside >= RC.ONE_SHARE
    T, iters, inl, rmse, status, assign, stats = _batch(method, [(_grid('tie target', p0, d), _grid('tie source', p1, d), Nq[0], Np[0], _dev(T0))], d, max_iter=1,
                                                        want_assign=True, want_stats=True, loss=loss, scale=RC.ONE_SCALE)
    _check_sums(stats[0], assign[0], want, f'{method} {loss}')
    assert int(inl[0]) == want['n_valid'] and int(iters[0]) == 1 and _status(status) == ['max_iter']
    assert abs(float(rmse[0]) - np.sqrt(want['sum_e2'] / want['n_valid'])) <= 1e-12
    x, lam = PO.solve(want['A'], want['b'], want['n_valid'])
    Rn, tn = PO.update(T0[:3, :3], T0[:3, 3], want['c'], x)
    assert np.abs(T[0][:3, :3] - Rn).max() <= 1e-10 and np.abs(T[0][:3, 3] - tn).max() <= 1e-10
    # and the loss did something: the unweighted entry's A differs in the third digit at the least
    plain = _batch(method, [(_grid('tie target', p0, d), _grid('tie source', p1, d), Nq[0], Np[0], _dev(T0))], d, max_iter=1, want_stats=True)
    assert np.abs(plain[5][0][4:25] - stats[0][4:25]).max() > 1e-3 * np.abs(plain[5][0][4:25]).max()
    assert _same_bits(plain[5][0][[0, 1, 2, 3, 31]], stats[0][[0, 1, 2, 3, 31]])          # count, c and sum e^2: not touched, bit for bit


# ---- 2: full runs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', RC.LOSSES)
@pytest.mark.parametrize('method', RC.METHODS)
def test_full_runs_on_the_convergence_pair(method, loss):
    """Both starts in one batch, scale 0.02: the oracle's iteration count, status and inliers, T within 1e-9."""
    p0, p1, Tg = PC.conv_pair()
    Nq, Np = _table('conv target', p0, RC.CONV_RADIUS), _table('conv source', p1, RC.CONV_RADIUS)
    g0, g1 = _grid('conv target', p0, RC.CONV_DIST), _grid('conv source', p1, RC.CONV_DIST)
    starts = PC.conv_starts()
    T, iters, inl, rmse, status = _batch(method, [(g0, g1, Nq[0], Np[0], _dev(T0)) for T0 in starts], RC.CONV_DIST, max_iter=RC.CONV_ITER, loss=loss,
                                         scale=RC.CONV_SCALE)
    for s in range(len(starts)):
        want, trace = RC.conv_reference(method, loss, s)
        assert RC.verdict_margin(trace) >= RC.MARGIN and want.status == 'converged'
        _check_against(want, T[s], int(iters[s]), int(inl[s]), float(rmse[s]), _status(status)[s], f'{method} {loss} start {s}')


@pytest.mark.parametrize('seed', RC.OUT_SEEDS)
def test_outlier_family_on_the_device(seed):
    """The raised patch: icp.refine under tukey at 0.03 ends where the oracle ends (iteration count, status, T within 1e-9), at no more than a
    tenth of the translation and rotation error of the run without a loss, which ends at least 5 mm off."""
    from roreg_amd import icp
    q, p, Tg = RC.outlier_pair(seed)
    opts = dict(max_dist=RC.OUT_DIST, max_iter=RC.OUT_ITER, method='plane', normal_radius=RC.OUT_RADIUS)
    robust = icp.refine(q, p, np.eye(4), loss=RC.OUT_LOSS, loss_scale=RC.OUT_SCALE, **opts)
    plain = icp.refine(q, p, np.eye(4), **opts)
    want, trace = RC.outlier_reference(seed, RC.OUT_LOSS)
    assert RC.verdict_margin(trace) >= RC.MARGIN
    _check_against(want, robust.T, robust.iters, robust.inliers, robust.rmse, robust.status, f'outlier seed {seed}')
    (deg0, t0), (deg1, t1) = O.pose_error(plain.T, Tg), O.pose_error(robust.T, Tg)
    print(f'seed {seed}: no loss {deg0:.4f} deg / {t0 * 1e3:.2f} mm in {plain.iters} searches; tukey {deg1:.4f} deg / {t1 * 1e3:.3f} mm in {robust.iters}')
    assert t0 * 1e3 >= RC.OUT_PLAIN_MM and t1 <= RC.OUT_FACTOR * t0 and deg1 <= RC.OUT_FACTOR * deg0


def test_noisy_walls_under_a_loss():
    """The ill-conditioned normal equations of the walls under tukey (plane method): what the oracle says, within the sums' 1e-12 times the
    condition number of its A."""
    for seed in C.WALL_SEEDS:
        q, p, _, T0 = C.wall_pair(seed)
        want, trace = RC.wall_reference(seed)
        cond = max(x['lam'][-1] / x['lam'][0] for x in trace)
        Nq = _table(f'wall {seed}', q, PC.RANK_RADIUS)
        T, iters, inl, rmse, status = _batch('plane', [(_grid(f'wall {seed}', q, C.WALL_DIST), _grid(f'wall {seed} source', p, C.WALL_DIST), Nq[0], None, _dev(T0))],
                                             C.WALL_DIST, max_iter=C.WALL_ITER, loss=RC.WALL_LOSS, scale=RC.WALL_SCALE)
        _check_against(want, T[0], int(iters[0]), int(inl[0]), float(rmse[0]), _status(status)[0], f'wall seed {seed}, cond {cond:.2e}', tol=1e-12 * cond)


# ---- 3: slot boundaries and batches ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', RC.METHODS)
def test_slot_boundaries_and_batch_independence(method):
    """Sources of 1, 1023, 1024, 1025 and 3073 points under huber at 0.01: one iteration's sums and the full runs against the oracle on the
    same tables; a pair alone, in a batch of seven and in the reversed batch gives the same bits; and a batch that MIXES losses (every
    task record carries its own kind and scale) gives every pair the bits of its single call."""
    cases, batch, host = _chunk_batch()
    kw = dict(loss=RC.CHUNK_LOSS, scale=RC.CHUNK_SCALE)
    one = _batch(method, batch, C.CHUNK_DIST, max_iter=1, want_assign=True, want_stats=True, **kw)
    full = _batch(method, batch, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True, **kw)
    for i, ((name, q, p, T0), (Nq, Np)) in enumerate(zip(cases, host)):
        _check_sums(one[6][i], one[5][i], RC.one_run(method, q, p, Nq, Np, T0, C.CHUNK_DIST, RC.CHUNK_LOSS, RC.CHUNK_SCALE), f'{method} {name}')
        want, trace = RC.full_run(method, q, p, Nq, Np, T0, C.CHUNK_DIST, RC.CHUNK_LOSS, RC.CHUNK_SCALE, C.CHUNK_ITER)
        assert RC.verdict_margin(trace) >= RC.MARGIN, name
        _check_against(want, full[0][i], int(full[1][i]), int(full[2][i]), float(full[3][i]), _status(full[4])[i], f'{method} {name}')
    assert _status(full[4])[0] == 'no_support' and _same_bits(full[0][0], cases[0][3])          # one point: T0 kept
    seven = batch + [batch[3], batch[1]]
    a = _batch(method, seven, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True, **kw)
    b = _batch(method, seven[::-1], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True, **kw)
    assert (a[1][1:5] > 1).all()
    for x, y in zip(a, b):
        assert _same_bits(x[::-1], y)
    for x, y in zip(a, full):
        assert _same_bits(x[:5], y) and _same_bits(x[5], x[3]) and _same_bits(x[6], x[1])
    for i in (0, 3, 4):
        alone = _batch(method, [batch[i]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True, **kw)
        for x, y in zip(a, alone):
            assert _same_bits(x[i:i + 1], y), cases[i][0]
    # mixed: pair 4 under every loss and under none, pair 3 under huber, in one call
    mix = [batch[4]] * 5 + [batch[3]]
    losses = list(RC.LOSSES) + [None, RC.CHUNK_LOSS]
    scales = [0.01, 0.02, 0.03, 0.04, None, RC.CHUNK_SCALE]
    m = _batch(method, mix, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True, loss=losses, scale=scales)
    for i, (l, k) in enumerate(zip(losses, scales)):
        single = _batch(method, [mix[i]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True, loss=l, scale=k)
        for x, y in zip(m, single):
            assert _same_bits(x[i:i + 1], y), (l, k)
    assert len({m[0][i].tobytes() for i in range(5)}) == 5 and _same_bits(m[0][5], full[0][3])
    # (a pair without a loss inside a weighted call runs the weighted kernel at weight 1: the unweighted entry's sums, hence its bits)
    assert _same_bits(m[0][4], _batch(method, [batch[4]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER)[0][0])
    from roreg_amd import hip
    for bad in (dict(loss=['huber'], scale=0.01), dict(loss='l2', scale=0.01), dict(loss='tukey'), dict(loss='tukey', scale=0.0), dict(loss='tukey', scale=float('nan')),
                dict(loss='tukey', scale=float('inf')), dict(scale=0.01)):
        with pytest.raises(hip.HipError):
            _batch(method, mix, C.CHUNK_DIST, max_iter=1, **bad)


# ---- 4: zero weights, huge scales ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', RC.METHODS)
def test_zero_weights_and_huge_scales(method):
    """tukey at scale 1e-6 on the noisy 3073-point pair: (all but a handful of) the weights are zero, A has no rank, the run ends in
    no_support after one search with T0 returned bit for bit -- the existing rule, as the oracle applies it too.  A scale of 1e6: every
    loss gives the unweighted entry's iteration count, status and T within 1e-9."""
    cases, batch, host = _chunk_batch()
    name, q, p, T0 = cases[4]
    Nq, Np = host[4]
    T, iters, inl, rmse, status = _batch(method, [batch[4]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, loss='tukey', scale=1e-6)
    want, _ = RC.full_run(method, q, p, Nq, Np, T0, C.CHUNK_DIST, 'tukey', 1e-6, C.CHUNK_ITER)
    assert want.status == 'no_support' and want.iters == 1
    assert _status(status) == ['no_support'] and int(iters[0]) == 1 and _same_bits(T[0], T0) and int(inl[0]) == want.inliers > 1000
    assert abs(float(rmse[0]) - want.rmse) <= 1e-12
    plain = _batch(method, [batch[4]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER)
    assert _status(plain[4]) == ['converged'] and int(plain[1][0]) > 1
    for loss in RC.LOSSES:
        got = _batch(method, [batch[4]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, loss=loss, scale=1e6)
        print(f'{method} {loss} at scale 1e6: max |T - T_unweighted| = {np.abs(got[0][0] - plain[0][0]).max():.3e}')
        assert np.abs(got[0][0] - plain[0][0]).max() <= 1e-9 and int(got[1][0]) == int(plain[1][0]) and _status(got[4]) == ['converged']
        assert int(got[2][0]) == int(plain[2][0])


# ---- 5: no loss ---------------------------------------------------------------------------------------------------------------------------------
def test_without_a_loss_every_route_gives_the_bits_it_gave():
    """loss=None through hip (against tests/golden/icp_parent_bits.npz: the walls' plane runs as an earlier commit's kernels returned them),
    through icp.refine and through RegistrationEngine.icp_many, for both methods: the same bits as the call without the arguments."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import record_icp_bits as rec
    from roreg_amd import hip, icp, synth
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    golden = np.load(rec.FIXTURE)
    walls = [C.wall_pair(seed) for seed in C.WALL_SEEDS]
    grids = [hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda(), C.WALL_DIST) for q, _, _, _ in walls]
    plane = [(g, hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda(), C.WALL_DIST), hip.icp_normals(g, PC.RANK_RADIUS), _dev(T0))
             for g, (_, p, _, T0) in zip(grids, walls)]
    got = hip.icp_plane_batch(plane, C.WALL_DIST, max_iter=C.WALL_ITER, want_assign=True, want_stats=True, loss=None, scale=None)
    for f, v in zip(('T', 'iters', 'inliers', 'rmse', 'status', 'assign', 'stats'), got):
        v = np.concatenate([rec._host(a) for a in v]) if isinstance(v, list) else rec._host(v)          # (floats as their bit patterns, as the fixture holds them)
        assert v.dtype == golden[f'wall/plane/{f}'].dtype and np.array_equal(v, golden[f'wall/plane/{f}']), f
    p0, p1, Tg = synth.make_dense_pair(43, 6000)
    T0 = O.perturb(Tg, 2.0, 0.03, 43)
    eng = RegistrationEngine(default_config(), None, None)
    c0, c1 = (eng.attach_points(CloudState(before=None), p) for p in (p0, p1))
    for method in RC.METHODS:
        a = icp.refine(p0, p1, T0, max_dist=0.1, max_iter=20, method=method)
        b = icp.refine(p0, p1, T0, max_dist=0.1, max_iter=20, method=method, loss=None, loss_scale=None)
        assert _same_bits(a.T, b.T) and a[1:3] == b[1:3] and a.status == b.status and a.iters > 1 and _same_bits(np.float64(a.rmse), np.float64(b.rmse))
        x = eng.icp_many([(c0, c1, _dev(T0))], 0.1, 20, method=method)
        y = eng.icp_many([(c0, c1, _dev(T0))], 0.1, 20, method=method, loss=None, loss_scale=None)
        for u, v in zip(x, y):
            assert torch.equal(u, v)
        assert _same_bits(x[0][0].cpu().numpy(), a.T)


# ---- 6: the Python layers -----------------------------------------------------------------------------------------------------------------------
def test_refine_icp_many_and_fpfh_register_carry_the_loss():
    """icp.refine(loss=) -- a TypeError without the feature -- equals the low-level entry and RegistrationEngine.icp_many(loss=) bit for bit,
    for both methods; fpfh.register hands its icp dict on to icp.refine (run_scene and Registrar hand theirs to icp_many in the same way);
    the ValueError cases fire at both layers."""
    from roreg_amd import hip, icp, synth
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    p0, p1, Tg = synth.make_dense_pair(43, 6000)
    T0 = O.perturb(Tg, 2.0, 0.03, 43)
    eng = RegistrationEngine(default_config(), None, None)
    c0, c1 = (eng.attach_points(CloudState(before=None), p) for p in (p0, p1))
    g0, g1 = hip.IcpGrid(icp.device_points(p0), 0.1), hip.IcpGrid(icp.device_points(p1), 0.1)
    n0, n1 = hip.icp_normals(g0, 0.2), hip.icp_normals(g1, 0.2)
    for method in RC.METHODS:
        opts = dict(max_dist=0.1, max_iter=20, method=method, loss='cauchy', loss_scale=0.02)
        one = icp.refine(p0, p1, T0, **opts)
        assert one.status in ('converged', 'max_iter') and one.iters > 1 and one.inliers > 1000 and max(O.pose_error(one.T, Tg)) < 0.05
        low = _batch(method, [(g0, g1, n0, n1, _dev(T0))], 0.1, max_iter=20, loss='cauchy', scale=0.02)
        many = _host(eng.icp_many([(c0, c1, _dev(T0))], 0.1, 20, method=method, loss='cauchy', loss_scale=0.02))
        for x in (low, many):
            assert _same_bits(x[0][0], one.T) and (int(x[1][0]), int(x[2][0])) == one[1:3] and _same_bits(np.float64(x[3][0]), np.float64(one.rmse))
        assert not _same_bits(icp.refine(p0, p1, T0, max_dist=0.1, max_iter=20, method=method).T, one.T)
        assert not _same_bits(icp.refine(p0, p1, T0, **dict(opts, loss_scale=0.01)).T, one.T)
        both = icp.refine([(p0, p1, T0), (p1, p0, np.linalg.inv(T0))], **opts)
        assert _same_bits(both[0].T, one.T) and both[1].status in ('converged', 'max_iter') and both[1].iters > 1
    for kw in (dict(method='plane', loss='l1', loss_scale=0.1), dict(method='plane', loss='tukey'), dict(method='gicp', loss='tukey', loss_scale=0.0),
               dict(method='gicp', loss='gm', loss_scale=float('nan')), dict(method='point', loss='tukey', loss_scale=0.03), dict(loss='huber', loss_scale=0.03)):
        with pytest.raises(ValueError):
            icp.refine(p0, p1, T0, max_dist=0.1, **kw)
        with pytest.raises(ValueError):
            eng.icp_many([(c0, c1, _dev(T0))], 0.1, **kw)
    # fpfh.register(icp=dict(...)): the dict reaches icp.refine
    from roreg_amd import fpfh
    import _fpfh_cases as FK
    q0, q1, Tq = FK.terrain_pair(0)
    fr = fpfh.register(q0, q1, voxel=FK.TERRAIN_VOXEL, icp=dict(method='plane', max_dist=0.1, loss='tukey', loss_scale=0.03))
    fp = fpfh.register(q0, q1, voxel=FK.TERRAIN_VOXEL, icp=dict(method='plane', max_dist=0.1))
    assert fr.icp.status in ('converged', 'max_iter') and _same_bits(fr.trans, fp.trans) and not _same_bits(fr.trans_icp, fp.trans_icp)
