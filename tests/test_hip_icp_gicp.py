"""Plane-to-plane (generalized) ICP on the device (csrc/icp.hip icp_gicp_kernel, "v6i") against its numpy definition
(tests/_icp_gicp_oracle.py).  The input families are tests/_icp_gicp_cases.py; tests/test_icp_gicp_oracle.py asserts on the CPU that each
family meets the conditions that make it exercise its branch.  The normal tables handed to the device AND to the oracle are the device's own
(hip.icp_normals, pinned to its oracle by tests/test_hip_icp_plane.py), downloaded once per cloud: the comparison is exact in its inputs.
GPU only."""
import numpy as np
import pytest
import torch

import _icp_cases as C
import _icp_gicp_cases as GC
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
from roreg_amd import synth

pytestmark = pytest.mark.gpu

_TABLES = {}


def _dev(T):
    return torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()


def _grid(p, d):
    from roreg_amd import hip
    return hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d)


def _table(name, p, radius, k=GC.MIN_NB):
    """The device's normal table of cloud `name` -> (device tensor, its host copy), computed once per (name, radius, k)."""
    from roreg_amd import hip
    key = (name, float(radius), int(k))
    if key not in _TABLES:
        t = hip.icp_normals(_grid(p, radius), radius, k)
        _TABLES[key] = (t, t.cpu().numpy())
    return _TABLES[key]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _status(s):
    from roreg_amd import hip
    return [hip.ICP_STATUS[int(v)] for v in s.cpu().numpy()]


def _host(out):
    return [[x.cpu().numpy() for x in v] if isinstance(v, list) else v.cpu().numpy() for v in out]


def _check_sums(stats, assign, want, name):
    """One iteration's sums against the oracle's: assignments and n equal, c to 1e-12, A and b within 1e-10 of their largest entry, sum d^T M d
    within 1e-10 of itself.  Each term carries at most a few tens of cond(S) 2^-53 <= 1e3 x 1.1e-16 and the summation of n <= 2e4 terms adds
    n 2^-53: both about 1e-12, so the bound leaves a factor 100 -> the worst observed fraction of the bound."""
    assert np.array_equal(assign, want['assign']), name
    assert int(stats[0]) == want['n'] == int((assign >= 0).sum()), name
    if want['n'] == 0:
        assert (stats == 0).all(), name
        return 0.0
    A, b = PO.upper(want['A']), want['b']
    err_c = np.abs(stats[1:4] - want['c']).max()
    frac = (np.abs(stats[4:25] - A).max() / (1e-10 * np.abs(A).max()), np.abs(stats[25:31] - b).max() / (1e-10 * np.abs(b).max()),
            abs(stats[31] - want['sum_md']) / (1e-10 * want['sum_md']))
    print(f'{name}: n = {want["n"]}, |c - c_oracle| = {err_c:.2e}; A, b, sum d^T M d at {frac[0]:.2e}, {frac[1]:.2e}, {frac[2]:.2e} of their 1e-10 bounds')
    assert err_c <= 1e-12 and max(frac) <= 1.0, name
    return max(frac)


def _check_against(want, T, iters, inliers, rmse, status, assign=None, name='', tol=1e-9):
    """The bar of the other two methods' full runs: status, iteration count and inliers equal, T within 1e-9."""
    print(f'{name}: device {iters} iterations, {inliers} inliers, whitened rmse {rmse}, {status}; oracle {want.iters}, {want.inliers}, {want.rmse}, {want.status}; '
          f'max |T - T_oracle| = {np.abs(T - want.T).max():.3e}')
    assert (iters, status, inliers) == (want.iters, want.status, want.inliers), name
    assert np.abs(T - want.T).max() <= tol, name
    assert abs(rmse - want.rmse) <= tol or (np.isnan(rmse) and np.isnan(want.rmse)), name
    if assign is not None and want.assign is not None:
        assert np.array_equal(assign, want.assign), name
        assert inliers == int((want.assign >= 0).sum()), name               # nothing is skipped: inliers are the distance inliers


def _chunk_batch():
    """-> (cases, [(target grid, source grid, Nq, Np, T0)], [(Nq host, Np host)]): the chunk family with the device's tables"""
    cases = GC.chunk_pairs()
    g0 = _grid(cases[0][1], C.CHUNK_DIST)
    Nq = _table('chunk target', cases[0][1], GC.CHUNK_RADIUS)
    batch, host = [], []
    for name, _, p, T0 in cases:
        Np = _table('chunk ' + name, p, GC.CHUNK_RADIUS)
        batch.append((g0, _grid(p, C.CHUNK_DIST), Nq[0], Np[0], _dev(T0)))
        host.append((Nq[1], Np[1]))
    return cases, batch, host


# ---- 1: one iteration ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', GC.TIE_DISTS)
def test_one_gicp_iteration_from_a_given_transform(d):
    """max_iter = 1 on the pair with planted ties, both clouds' normals of radius 2 d from the device: the assignments and n are the
    oracle's, c within 1e-12, A, b and sum d^T M d within 1e-10 of their scale; the update is the oracle's solve of those sums."""
    from roreg_amd import hip
    p0, p1, T0 = PC.tie_pair()
    Nq, Np = _table('tie target', p0, 2 * d), _table('tie source', p1, 2 * d)
    want = GC.run_one(p0, p1, Nq[1], Np[1], T0, d)
    assert np.isin(want['assign'], np.arange(100, 1100)).sum() > 50 and not np.isin(want['assign'], np.arange(5000, 6000)).any()        # the ties went to the lowest row
    T, iters, inl, rmse, status, assign, stats = hip.icp_gicp_batch([(_grid(p0, d), _grid(p1, d), Nq[0], Np[0], _dev(T0))], d, max_iter=1, want_assign=True,
                                                                    want_stats=True)
    stats = stats[0].cpu().numpy()
    worst = _check_sums(stats, assign[0].cpu().numpy(), want, f'tie pair, d = {d}')
    print(f'd = {d}: worst fraction of the 1e-10 bound = {worst:.3e}')
    assert int(inl[0]) == want['n'] and int(iters[0]) == 1 and _status(status) == ['max_iter']
    assert abs(float(rmse[0]) - np.sqrt(want['sum_md'] / want['n'])) <= 1e-12
    x, lam = PO.solve(want['A'], want['b'], want['n'])
    Rn, tn = PO.update(T0[:3, :3], T0[:3, 3], want['c'], x)
    Td = T[0].cpu().numpy()
    assert np.abs(Td[:3, :3] - Rn).max() <= 1e-10 and np.abs(Td[:3, 3] - tn).max() <= 1e-10
    assert np.abs(Td[:3, :3] @ Td[:3, :3].T - np.eye(3)).max() <= 1e-14


# ---- 2: chunk edges --------------------------------------------------------------------------------------------------------------------------
def test_chunk_edges_one_iteration_and_full_runs():
    """Sources of 1, 1023, 1024, 1025 and 3073 points against a whole target, each source with its own table (the one-point source: a zero
    row; about half the rows of the 1023 .. 1025-point ones): one iteration's sums as in test 1, the full runs at the oracle's status,
    iteration count and transform -- the one-point source ends in no_support with T0 kept."""
    from roreg_amd import hip
    cases, batch, host = _chunk_batch()
    one = _host(hip.icp_gicp_batch(batch, C.CHUNK_DIST, max_iter=1, want_assign=True, want_stats=True))
    full = _host(hip.icp_gicp_batch(batch, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True))
    for i, ((name, q, p, T0), (Nq, Np)) in enumerate(zip(cases, host)):
        _check_sums(one[6][i], one[5][i], GC.run_one(q, p, Nq, Np, T0, C.CHUNK_DIST), name)
        want, trace = GC.run_full(q, p, Nq, Np, T0, C.CHUNK_DIST, C.CHUNK_ITER)
        assert GC.verdict_margin(trace) > 2.0, name
        _check_against(want, full[0][i], int(full[1][i]), int(full[2][i]), float(full[3][i]), _status(torch.from_numpy(full[4]))[i], full[5][i], name)
    assert _status(torch.from_numpy(full[4]))[0] == 'no_support' and _same_bits(full[0][0], cases[0][3])
    assert (host[0][1][:, :3] == 0).all() and 0.3 < (host[1][1][:, :3] != 0).any(1).mean() < 0.7


# ---- 3: full runs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', GC.CONV_RADII)
def test_full_runs_on_the_convergence_pair(radius):
    """From both starts at normal radius 0.2 and 0.1 (where the plane method cycles to max_iter): converged at the oracle's iteration count,
    T within 1e-9, inliers equal."""
    from roreg_amd import hip
    p0, p1, Tg = PC.conv_pair()
    Nq, Np = _table('conv target', p0, radius), _table('conv source', p1, radius)
    g0, g1 = _grid(p0, GC.CONV_DIST), _grid(p1, GC.CONV_DIST)
    starts = PC.conv_starts()
    T, iters, inl, rmse, status = _host(hip.icp_gicp_batch([(g0, g1, Nq[0], Np[0], _dev(T0)) for T0 in starts], GC.CONV_DIST, max_iter=GC.CONV_ITER))
    for s, T0 in enumerate(starts):
        want, trace = GC.run_full(p0, p1, Nq[1], Np[1], T0, GC.CONV_DIST, GC.CONV_ITER)
        e = O.pose_error(T[s], Tg)
        print(f'radius {radius}, start {s}: {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm from the ground truth, verdict margin {GC.verdict_margin(trace):.2f}')
        assert GC.verdict_margin(trace) > 2.0
        _check_against(want, T[s], int(iters[s]), int(inl[s]), float(rmse[s]), _status(torch.from_numpy(status))[s], name=f'radius {radius}, start {s}')
        assert want.status == 'converged' and want.iters < 10


def test_full_runs_on_planes_and_walls():
    """One, two and three exact planes (the plane method refuses the first two) and the noisy walls: the oracle's verdict, iteration count,
    inliers, T within 1e-9."""
    from roreg_amd import hip
    for n in GC.RANK_PLANES:
        tgt, src, Tg, T0 = PC.planes_pair(n)
        Nq, Np = _table(f'planes {n} target', tgt, GC.RANK_RADIUS), _table(f'planes {n} source', src, GC.RANK_RADIUS)
        want, trace = GC.run_full(tgt, src, Nq[1], Np[1], T0, GC.RANK_DIST, GC.RANK_ITER)
        T, iters, inl, rmse, status = _host(hip.icp_gicp_batch([(_grid(tgt, GC.RANK_DIST), _grid(src, GC.RANK_DIST), Nq[0], Np[0], _dev(T0))], GC.RANK_DIST,
                                                               max_iter=GC.RANK_ITER))
        assert GC.verdict_margin(trace) > 2.0 and want.status == 'converged'
        _check_against(want, T[0], int(iters[0]), int(inl[0]), float(rmse[0]), _status(torch.from_numpy(status))[0], name=f'{n} planes')
    for seed in GC.WALL_SEEDS:
        q, p, _, T0 = C.wall_pair(seed)
        Nq, Np = _table(f'wall {seed} target', q, GC.RANK_RADIUS), _table(f'wall {seed} source', p, GC.RANK_RADIUS)
        want, trace = GC.run_full(q, p, Nq[1], Np[1], T0, C.WALL_DIST, C.WALL_ITER)
        T, iters, inl, rmse, status = _host(hip.icp_gicp_batch([(_grid(q, C.WALL_DIST), _grid(p, C.WALL_DIST), Nq[0], Np[0], _dev(T0))], C.WALL_DIST,
                                                               max_iter=C.WALL_ITER))
        assert GC.verdict_margin(trace) > 2.0
        _check_against(want, T[0], int(iters[0]), int(inl[0]), float(rmse[0]), _status(torch.from_numpy(status))[0], name=f'wall seed {seed}')


# ---- 4: the sign of the normals ----------------------------------------------------------------------------------------------------------------
def test_the_sign_of_a_normal_changes_no_bit():
    """An arbitrary half of the rows of either table negated: n n^T is the same product and R (-n) = -(R n) exactly, so every output is the
    same bits."""
    from roreg_amd import hip
    cases, batch, host = _chunk_batch()
    g0, g1, Nq, Np, T0 = batch[4]
    rng = np.random.default_rng(0x51)
    base = _host(hip.icp_gicp_batch([batch[4]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True, want_stats=True))
    assert int(base[1][0]) > 1
    for flip_q, flip_p in ((True, False), (False, True), (True, True)):
        tabs = []
        for t, flip in ((Nq, flip_q), (Np, flip_p)):
            t = t.clone()
            if flip:
                rows = torch.from_numpy(rng.random(t.shape[0]) < 0.5).cuda()
                t[rows, :3] = -t[rows, :3]
                assert rows.any() and not rows.all()
            tabs.append(t)
        got = _host(hip.icp_gicp_batch([(g0, g1, tabs[0], tabs[1], T0)], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True, want_stats=True))
        for x, y in zip(base, got):
            assert _same_bits(x[0], y[0]) if isinstance(x, list) else _same_bits(x, y), (flip_q, flip_p)


# ---- 5: zero and mixed tables ------------------------------------------------------------------------------------------------------------------
def test_zero_and_half_valid_tables():
    """Both tables zero (the uniform weighting), and min_neighbors raised to the median neighbour count so that about half the rows of
    either table are zero: the oracle's result given the same tables, inliers = the distance inliers in both."""
    from roreg_amd import hip
    name, q, p, T0 = GC.chunk_pairs()[4]
    g0, g1 = _grid(q, C.CHUNK_DIST), _grid(p, C.CHUNK_DIST)
    Nq, Np = _table('chunk target', q, GC.CHUNK_RADIUS), _table('chunk ' + name, p, GC.CHUNK_RADIUS)
    kq, kp = int(np.median(Nq[1][:, 3])), int(np.median(Np[1][:, 3]))
    half = (_table('chunk target', q, GC.CHUNK_RADIUS, kq), _table('chunk ' + name, p, GC.CHUNK_RADIUS, kp))
    for h in half:
        share = (h[1][:, :3] != 0).any(1).mean()
        print(f'min_neighbors raised: {share * 100:.1f} % of the rows keep a normal')
        assert 0.3 < share < 0.7
    zero = ((torch.zeros_like(Nq[0]), np.zeros_like(Nq[1])), (torch.zeros_like(Np[0]), np.zeros_like(Np[1])))
    for label, (tq, tp) in (('zero tables', zero), ('half-valid tables', half)):
        one = _host(hip.icp_gicp_batch([(g0, g1, tq[0], tp[0], _dev(T0))], C.CHUNK_DIST, max_iter=1, want_assign=True, want_stats=True))
        _check_sums(one[6][0], one[5][0], GC.run_one(q, p, tq[1], tp[1], T0, C.CHUNK_DIST), label)
        assert int(one[2][0]) == int((one[5][0] >= 0).sum())
        full = _host(hip.icp_gicp_batch([(g0, g1, tq[0], tp[0], _dev(T0))], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_assign=True))
        want, trace = GC.run_full(q, p, tq[1], tp[1], T0, C.CHUNK_DIST, C.CHUNK_ITER)
        assert GC.verdict_margin(trace) > 2.0, label
        _check_against(want, full[0][0], int(full[1][0]), int(full[2][0]), float(full[3][0]), _status(torch.from_numpy(full[4]))[0], full[5][0], label)
        assert int(full[2][0]) == int((full[5][0] >= 0).sum()) > 1000


# ---- 6: batch independence ---------------------------------------------------------------------------------------------------------------------
def test_a_pairs_bits_do_not_depend_on_the_batch():
    """A pair alone, in a batch of seven of mixed sizes, and in the reversed batch: the same bits."""
    from roreg_amd import hip
    cases, batch, host = _chunk_batch()
    seven = batch + [batch[3], batch[1]]
    a = _host(hip.icp_gicp_batch(seven, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True))
    b = _host(hip.icp_gicp_batch(seven[::-1], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True))
    assert (a[1][1:5] > 1).all()
    for x, y in zip(a, b):
        assert _same_bits(x[::-1], y)
    for x in a:
        assert _same_bits(x[5], x[3]) and _same_bits(x[6], x[1])
    for i in (0, 3, 4):
        alone = _host(hip.icp_gicp_batch([batch[i]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True))
        for x, y in zip(a, alone):
            assert _same_bits(x[i:i + 1], y), cases[i][0]


# ---- 7: epsilon --------------------------------------------------------------------------------------------------------------------------------
def test_epsilon_against_the_oracle_and_its_validation():
    """epsilon 1e-3, 1e-2 and 1 in one batch against the oracle; epsilon = 1 gives the bits of the zero-table run (kappa = 0 and a zero normal
    both leave S = 2 I exactly); 0, a negative value, a value above 1 and NaN are refused."""
    from roreg_amd import hip
    name, q, p, T0 = GC.chunk_pairs()[4]
    g0, g1 = _grid(q, C.CHUNK_DIST), _grid(p, C.CHUNK_DIST)
    Nq, Np = _table('chunk target', q, GC.CHUNK_RADIUS), _table('chunk ' + name, p, GC.CHUNK_RADIUS)
    batch = [(g0, g1, Nq[0], Np[0], _dev(T0), eps) for eps in GC.EPSILONS] + [(g0, g1, torch.zeros_like(Nq[0]), torch.zeros_like(Np[0]), _dev(T0))]
    one = _host(hip.icp_gicp_batch(batch, C.CHUNK_DIST, max_iter=1, want_assign=True, want_stats=True))
    full = _host(hip.icp_gicp_batch(batch, C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True))
    for i, eps in enumerate(GC.EPSILONS):
        _check_sums(one[6][i], one[5][i], GC.run_one(q, p, Nq[1], Np[1], T0, C.CHUNK_DIST, eps), f'epsilon {eps}')
        want, trace = GC.run_full(q, p, Nq[1], Np[1], T0, C.CHUNK_DIST, C.CHUNK_ITER, eps)
        assert GC.verdict_margin(trace) > 2.0, eps
        _check_against(want, full[0][i], int(full[1][i]), int(full[2][i]), float(full[3][i]), _status(torch.from_numpy(full[4]))[i], name=f'epsilon {eps}')
    assert not _same_bits(one[6][0], one[6][1]) and not _same_bits(one[6][1], one[6][2])
    for out in (one, full):                                          # row 2: epsilon = 1; row 3: zero tables at the default epsilon
        for k in (0, 1, 2, 3, 4, len(out) - 1):
            assert _same_bits(out[k][2], out[k][3]), k
    default = _host(hip.icp_gicp_batch([batch[0][:5]], C.CHUNK_DIST, max_iter=C.CHUNK_ITER, want_stats=True))
    assert all(_same_bits(x[:1], y) for x, y in zip(full, default))          # 1e-3 is the default
    for bad in (0.0, -1e-3, 1.0 + 1e-12, 2.0, float('nan'), float('inf')):
        with pytest.raises(hip.HipError):
            hip.icp_gicp_batch([(g0, g1, Nq[0], Np[0], _dev(T0), bad)], C.CHUNK_DIST, max_iter=1)


# ---- 8: the public surface ---------------------------------------------------------------------------------------------------------------------
def _same_result(a, b):
    return _same_bits(a.T, b.T) and a[1:3] == b[1:3] and a.status == b.status and _same_bits(np.float64(a.rmse), np.float64(b.rmse))


def test_refine_gicp_through_every_route(monkeypatch):
    """icp.refine(method='gicp') -- which raises ValueError without the feature -- gives the same bits for one pair, in a list that shares
    its arrays (each gridded and given a normal table once), on clouds downsampled by voxel= or beforehand, and through
    RegistrationEngine.icp_many; a mis-shaped or misaligned source table is refused."""
    from roreg_amd import hip, icp, voxel
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    p0, p1, Tg = synth.make_dense_pair(43, 6000)
    T0 = O.perturb(Tg, 2.0, 0.03, 43)
    opts = dict(max_dist=0.1, max_iter=20, method='gicp')
    one = icp.refine(p0, p1, T0, **opts)
    assert one.status == 'converged' and 1 < one.iters < 12 and one.inliers > 1000 and max(O.pose_error(one.T, Tg)) < 0.05
    # against the low-level entry with tables of the default radius 2 max_dist
    g0, g1 = _grid(p0, 0.1), _grid(p1, 0.1)
    low = hip.icp_gicp_batch([(g0, g1, hip.icp_normals(g0, 0.2), hip.icp_normals(g1, 0.2), _dev(T0))], 0.1, max_iter=20)
    assert _same_result(one, icp.results_to_host(*low)[0])
    # a list with shared arrays: two grids and two tables for two pairs
    calls = {'grid': 0, 'normals': 0}
    real_grid, real_normals = hip.IcpGrid, hip.icp_normals
    monkeypatch.setattr(hip, 'IcpGrid', lambda *a, **k: (calls.__setitem__('grid', calls['grid'] + 1), real_grid(*a, **k))[1])
    monkeypatch.setattr(hip, 'icp_normals', lambda *a, **k: (calls.__setitem__('normals', calls['normals'] + 1), real_normals(*a, **k))[1])
    both = icp.refine([(p0, p1, T0), (p1, p0, np.linalg.inv(T0))], **opts)
    monkeypatch.undo()
    assert calls == {'grid': 2, 'normals': 2}
    assert _same_result(both[0], one) and both[1].status == 'converged'
    assert _same_result(icp.refine(p0, p1, T0, gicp_epsilon=1e-3, normal_radius=0.2, **opts), one)
    assert not _same_bits(icp.refine(p0, p1, T0, gicp_epsilon=1e-2, **opts).T, one.T)
    # voxel=: the refinement of the clouds downsampled on the device
    v0, v1 = voxel.downsample(p0, 0.05).points, voxel.downsample(p1, 0.05).points
    rv = icp.refine(p0, p1, T0, voxel=0.05, **opts)
    assert _same_result(rv, icp.refine(v0, v1, T0, **opts)) and 200 < rv.inliers < one.inliers and rv.status == 'converged'
    # the engine: cached grids and tables, the source's table too
    eng = RegistrationEngine(default_config(), None, None)
    c0, c1 = (eng.attach_points(CloudState(before=None), p) for p in (p0, p1))
    items = [(c0, c1, _dev(T0)), (c1, c0, _dev(np.linalg.inv(T0)))]
    out = eng.icp_many(items, 0.1, 20, method='gicp')
    assert set(c0.normals) == {(0.2, 6)} and set(c1.normals) == {(0.2, 6)} and len(c0.grids) == 1
    ptr = c1.normals[(0.2, 6)].data_ptr()
    out2 = eng.icp_many(items, 0.1, 20, method='gicp', gicp_epsilon=1e-3)
    assert c1.normals[(0.2, 6)].data_ptr() == ptr and len(c1.normals) == 1
    for x, y in zip(out, out2):
        assert torch.equal(x, y)
    for g, w in zip(icp.results_to_host(*out), both):
        assert _same_result(g, w)
    with pytest.raises(ValueError):
        eng.icp_many(items, 0.1, method='gicpp')
    with pytest.raises(ValueError):
        icp.refine(p0, p1, T0, max_dist=0.1, method='generalized')
    # tables that do not fit their cloud
    Nq, Np = hip.icp_normals(g0, 0.2), hip.icp_normals(g1, 0.2)
    shifted = torch.zeros(Np.numel() + 1, dtype=torch.float64, device='cuda')[1:].view(-1, 4)
    shifted.copy_(Np)
    assert shifted.data_ptr() % 32 == 8
    for bad_q, bad_p in ((Nq, Np[:-1]), (Nq, Np[:, :3].contiguous()), (Nq, shifted), (Nq, Np.float()), (Nq[:-1], Np), (Nq, None)):
        with pytest.raises(hip.HipError):
            hip.icp_gicp_batch([(g0, g1, bad_q, bad_p, _dev(T0))], 0.1, max_iter=1)


# ---- 9: the other methods ----------------------------------------------------------------------------------------------------------------------
def test_point_and_plane_results_do_not_change_around_a_gicp_call():
    """method='point' and method='plane' on one case each, before and after a gicp call on the same grids and tables: the same bits (the
    guard on their bits against the parent commit is tests/test_hip_icp_edges.py with icp_parent_bits.npz; this one is about the dispatch)."""
    from roreg_amd import hip
    p0, p1, Tg = synth.make_dense_pair(41, 5000)
    T0 = O.perturb(Tg, 2.0, 0.03, 41)
    g0, g1 = _grid(p0, 0.1), _grid(p1, 0.1)
    Nq, Np = hip.icp_normals(g0, 0.2), hip.icp_normals(g1, 0.2)
    point = lambda: _host(hip.icp_batch([(g0, g1, _dev(T0))], 0.1, max_iter=12, want_stats=True))
    plane = lambda: _host(hip.icp_plane_batch([(g0, g1, Nq, _dev(T0))], 0.1, max_iter=12, want_stats=True))
    before = (point(), plane())
    gicp = _host(hip.icp_gicp_batch([(g0, g1, Nq, Np, _dev(T0))], 0.1, max_iter=12, want_stats=True))
    after = (point(), plane())
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert _same_bits(x, y)
    assert int(gicp[1][0]) > 1 and not _same_bits(gicp[0], before[1][0]) and not _same_bits(gicp[0], before[0][0])
    want = O.icp(p0, p1, T0, 0.1, max_iter=12)
    assert int(before[0][1][0]) == want.iters and np.abs(before[0][0][0] - want.T).max() <= 1e-9


def test_run_scene_and_run_distributed_carry_the_gicp_refinement(tmp_path):
    """run_scene's icp= dict passes method='gicp' and gicp_epsilon through (both clouds of a pair get their table, once per cloud); and
    run_distributed.evaluate at world size 1 writes {ET}_icp_gicp/ and an '-icp-gicp' block whose table holds icp.refine(method='gicp')'s
    results, beside no {ET}_icp/ and no {ET}_icp_plane/."""
    import os
    from conftest import load_golden
    from test_hip_icp import _cfg_and_nets, _dense_scene
    from roreg_amd import distributed as D, icp, run_distributed as RD_
    from roreg_amd.engine import RegistrationEngine
    z = load_golden('pipeline_mutual_yohoo')
    opts = dict(max_dist=0.1, max_iter=15, method='gicp', normal_radius=0.2, gicp_epsilon=2e-3)
    cfg, gf, et = _cfg_and_nets(tmp_path, z, ET='yohoo', testset='synth')
    keynum = int(z['keynum'])
    ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
    dense = _dense_scene(ds, 6000, 31)
    keys = [ds.get_kps(i) for i in ds.pc_ids]
    eng = RegistrationEngine(cfg, gf, et)
    np.random.seed(99)
    ready = {}
    res = eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=keynum, max_iter=1000, points=dense, icp=opts, ready=ready)
    want = icp.refine([(dense[int(r.id0)], dense[int(r.id1)], r.trans) for r in res], **opts)
    for r, w in zip(res, want):
        print(r.id0, r.id1, r.icp_iters, r.icp_inliers, r.icp_rmse, r.icp_status)
        assert _same_bits(r.trans_icp, w.T) and (r.icp_iters, r.icp_inliers, r.icp_status) == (w.iters, w.inliers, w.status)
        assert _same_bits(np.float64(r.icp_rmse), np.float64(w.rmse))
    assert any(r.icp_iters > 1 for r in res)
    in_pairs = {int(i) for r in res for i in (r.id0, r.id1)}
    assert all(len(ready[i].normals) == 1 for i in in_pairs)          # targets AND sources
    other = icp.refine([(dense[int(r.id0)], dense[int(r.id1)], r.trans) for r in res], **dict(opts, gicp_epsilon=1e-3))
    assert any(not _same_bits(a.T, b.T) for a, b in zip(want, other))          # the epsilon arrived
    # run_distributed
    ds.write_inputs(cfg.output_cache_fn)
    ds.gt_dir = f'{tmp_path}/nonexistent/{ds.name}/gt.log'
    ds.get_pc = lambda i: dense[int(i)]
    out = RD_.evaluate(cfg, {'wholesetname': 'synth', 'scene0': ds}, RegistrationEngine(cfg, gf, et), rank=0, world=1, seed=3, icp=opts)
    log = open(f'{cfg.base_dir}/results.log').read().splitlines()
    assert log[7] == log[0] + '-icp-gicp' and log[10].startswith('registration recall(pointdsc)')
    base = f'{cfg.output_cache_fn}/{ds.name}/match_{cfg.keynum}'
    assert os.path.isdir(f'{base}/yohoo_icp_gicp') and not os.path.exists(f'{base}/yohoo_icp') and not os.path.exists(f'{base}/yohoo_icp_plane')
    sub, sub_icp = f'yohoo/{cfg.max_iter}iters', f'yohoo_icp_gicp/{cfg.max_iter}iters'
    coarse = {f'{a}-{b}': np.load(f'{base}/{sub}/{a}-{b}.npz')['trans'] for a, b in ds.pair_ids}
    want = icp.refine([(dense[int(a)], dense[int(b)], coarse[f'{a}-{b}']) for a, b in ds.pair_ids], **opts)
    rows = {(r['id0'], r['id1']): r for r in D.unpack_rows(out['icp']['table'])}
    for (a, b), w in zip(ds.pair_ids, want):
        row = rows[(a, b)]
        assert _same_bits(row['trans'][:3], w.T[:3]) and row['n_match'] == w.inliers and row['recalltime'] == w.iters
        f = np.load(f'{base}/{sub_icp}/{a}-{b}.npz')
        assert _same_bits(f['trans'][:3], w.T[:3]) and int(f['recalltime']) == w.iters and int(f['inliers']) == w.inliers
    assert os.path.exists(f'{base}/{sub_icp}/pre.log') and out['icp']['pairs'] == len(ds.pair_ids)
