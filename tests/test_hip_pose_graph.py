"""The pose-graph optimiser on the device (csrc/pose_graph.hip "v6h") against its numpy restatement (tests/_pose_graph_oracle.py) on the
seeded families of tests/_pose_graph_cases.py, whose conditions tests/test_pose_graph_oracle.py asserts on the CPU.  GPU only.

Tolerances.  One round's pieces: e, J, w within 1e-12 max(1, |t|_max) (short float64 formulas); H and g entrywise within 1e-12 of the oracle's
sum of absolute values sum w |J|^T |Lambda| |J| (resp. |e|), a bound that holds for any order of summation of the SAME terms; the terms
contain e and J, which two correct evaluations round differently -- both go through three 3-term products and two differences of numbers
of size |t|_max, 16 roundings at the most -- so the bars also admit that: r = 16 2^-53 max(1, |t|_max) times sum w |J|^T |Lambda| 1 for g and
times sum w (|J|^T |Lambda| 1 1^T + 1 1^T |Lambda| |J|) for H.  For H that adds 1-2 % to an ordinary entry's bar; it is the whole bar where the
exact entry is 0 (the off-diagonal of R_E^T n R_E on a node whose edges the start satisfies exactly: sum |.| is 1e-12 there and the entry is
rounding noise of 1e-13).  For g it is a third of the bar on a graph with residuals (5e-3 here) and the whole bar on a tree (2/1), where e
itself is rounding noise.  delta within 8 n 2^-53 cond_2(A) |delta| of numpy.linalg.solve on the oracle's A with the device's g as the right
side: g has its own check above, and on a tree it is noise that no two evaluations share.  Whole runs: the decisions and the iteration count equal the oracle's,
costs to 1e-10 relative, poses to 1e-9 (the ICP tests' bar for whole runs).

Sizes of the solve kernel's loops (hip.PG_PANEL = 32 columns per Cholesky panel, hip.PG_TILE = 64 rows per trailing tile, 2 PG_TILE = 128
rows per LDS stage of the panel below the diagonal block; n = 6 (C - 1) moves in steps of one node's block): _pose_graph_cases.SOLVE_EDGES
names n = 24, 30 | 36 around the panel width, 90, 96 | 102 around one tile behind the first panel, 156 | 162, 168 around one stage.  The
panel is staged through LDS 128 rows at a time whatever n is: there is no second path and hence no LDS panel limit to straddle."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import _pose_graph_cases as K
import _pose_graph_oracle as O
from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _graph(g, tau=None, anchor=0, use_init=True, **opt):
    from roreg_amd import hip
    init = g.get('init') if use_init else None
    return hip.PgGraph(g['C'], g['edges'], _dev(g['T']), _dev(g['Lam']), None if init is None else _dev(init), anchor, tau, **opt)


def _host(dev, b=0, E=None, C=None):
    """graph b of a PgDev -> dict of numpy arrays"""
    n0, e0 = dev.node0[b], dev.edge0[b]
    n1 = dev.node0[b + 1] if b + 1 < len(dev.node0) else dev.poses.shape[0]
    e1 = dev.edge0[b + 1] if b + 1 < len(dev.edge0) else dev.weights.shape[0]
    iters = int(dev.iters[b].item())
    from roreg_amd import hip
    return dict(poses=dev.poses[n0:n1].cpu().numpy(), cost0=float(dev.cost[b, 0].item()), cost=float(dev.cost[b, 1].item()), iters=iters,
                status=hip.PG_STATUS[int(dev.status[b].item())], weights=dev.weights[e0:e1].cpu().numpy(), chi2=dev.chi2[e0:e1].cpu().numpy(),
                history=dev.history[b, :iters].cpu().numpy(), reached=dev.reached[b])


def _run(g, max_iter=100, **kw):
    from roreg_amd import hip
    return _host(hip.pg_optimize_batch([_graph(g, **kw)], max_iter))


_oracle = {}


def _ref(key, g, tau=None, anchor=0, **kw):
    if key not in _oracle:
        G = O.Graph(g['C'], g['edges'], g['T'], g['Lam'], anchor=anchor, tau=tau)
        _oracle[key] = (G, G.optimize(init=g.get('init'), **kw))
    return _oracle[key]


def _same_run(got, ref, name):
    print(f"{name}: {got['status']} in {got['iters']} rounds (oracle {ref['iters']}), decisions {got['history'][:, 3].astype(int).tolist()}, "
          f"cost {got['cost']!r} (oracle {ref['cost']!r}), max |pose - oracle| {np.abs(got['poses'] - ref['poses']).max():.2e}")
    assert got['status'] == ref['status'] and got['iters'] == ref['iters'], name
    assert np.array_equal(got['history'][:, 3], ref['history'][:, 3]), name
    for col in (0, 1):
        a, b = got['history'][:, col], ref['history'][:, col]
        ok = np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(a[ok] - b[ok]) <= 1e-10 * np.abs(b[ok])).all(), name
    assert np.array_equal(got['history'][:, 2], ref['history'][:, 2]), name                       # lambda: exact powers of ten of lambda0
    assert abs(got['cost'] - ref['cost']) <= 1e-10 * abs(ref['cost']) and abs(got['cost0'] - ref['cost0']) <= 1e-10 * abs(ref['cost0']), name
    assert np.abs(got['poses'] - ref['poses']).max() <= 1e-9, name
    assert np.abs(got['weights'] - ref['weights']).max() <= 1e-9 and (np.abs(got['chi2'] - ref['chi2']) <= 1e-9 * (1 + ref['chi2'])).all(), name


PIECES = [('2/1', lambda: K.ring_graph(1, 2, 1), None)] + [(f'{C}/{E}', (lambda C=C, E=E: K.matched(C, E)), None) for C, E in K.MATCHED[0:]] + \
         [(f'{name} C={C}', (lambda C=C: K.solve_edge(C)), None) for name, C in K.SOLVE_EDGES.items()] + \
         [('12/21 outliers tau', lambda: K.with_outliers(12, 21), K.TAU)]


@pytest.mark.parametrize('name,make,tau', PIECES, ids=[p[0] for p in PIECES])
def test_one_rounds_pieces(name, make, tau):
    from roreg_amd import hip
    g = make()
    dev = hip.pg_optimize_batch([_graph(g, tau=tau)], max_iter=1, want_pieces=True)
    lin, H, gv, delta = (v.cpu().numpy() for v in dev.pieces)
    G = O.Graph(g['C'], g['edges'], g['T'], g['Lam'], tau=tau)
    P0 = O.initial_poses(g['C'], g['edges'], g['T'], 0)
    e, chi2, w, Ji, Jj = G.linearise(P0)
    de, dchi2, dw, dJi, dJj = hip.pg_dense_jacobians(lin)
    bar = 1e-12 * max(1.0, np.abs(P0[:, :3, 3]).max(), np.abs(g['T'][:, :3, 3]).max())
    worst = max(np.abs(de - e).max(), np.abs(dJi - Ji).max(), np.abs(dJj - Jj).max(), np.abs(dw - w).max())
    n = G.n
    Href, gref, Habs, gabs = G.assemble(P0)
    Hd = H.reshape(n, n)
    low = np.tril(np.ones((n, n), bool))
    tmax = max(1.0, np.abs(P0[:, :3, 3]).max(), np.abs(g['T'][:, :3, 3]).max())
    Hbar = 1e-12 * Habs + 16 * EPS * tmax * G.H_sensitivity(P0)
    fH = (np.abs(Hd - Href)[low] / (Hbar[low] + 1e-300)).max()
    gbar = 1e-12 * gabs + 16 * EPS * tmax * G.g_sensitivity(P0)
    fg = (np.abs(gv - gref) / (gbar + 1e-300)).max()
    A = G.damped(Href, 1e-3)
    want = np.linalg.solve(A, -gv)
    cond = np.linalg.cond(A)
    fd = np.linalg.norm(delta - want) / (8 * n * EPS * cond * np.linalg.norm(want))
    print(f'{name}: n = {n}, e/J/w error {worst:.2e} = {worst / bar:.3f} of its bar, H {fH:.3e}, g {fg:.3e}, delta {fd:.3e} of theirs (cond {cond:.2e})')
    assert worst <= bar
    assert (np.abs(Hd - Href)[low] <= Hbar[low]).all() and (np.abs(gv - gref) <= gbar).all()
    assert np.linalg.norm(delta - want) <= 8 * n * EPS * cond * np.linalg.norm(want)


WHOLE = [(f'matched {C}/{E}', (lambda C=C, E=E: K.matched(C, E)), None) for C, E in K.MATCHED] + \
        [(f'outliers {C}/{E} tau', (lambda C=C, E=E: K.with_outliers(C, E)), K.TAU) for C, E in K.OUTLIERS] + \
        [(f'outliers {C}/{E} plain', (lambda C=C, E=E: K.with_outliers(C, E)), None) for C, E in K.OUTLIERS] + \
        [(f'solve {name} C={C}', (lambda C=C: K.solve_edge(C)), None) for name, C in K.SOLVE_EDGES.items()] + \
        [('far start', K.far_start, None)]


@pytest.mark.parametrize('name,make,tau', WHOLE, ids=[p[0] for p in WHOLE])
def test_whole_runs_match_the_oracle_round_for_round(name, make, tau):
    g = make()
    ref = _ref((name, tau), g, tau=tau)[1]
    got = _run(g, tau=tau)
    _same_run(got, ref, name)
    if name == 'far start':
        assert (got['history'][:, 3] == O.DEC_REJECT).sum() >= 1


def test_exactly_satisfiable_graphs_reach_the_truth():
    for name, g in (('tree 8', K.tree(21, 8)), ('tree 40', K.tree(23, 40)), ('loop 12/21', K.noise_free_loop(22, 12, 21)), ('loop 33/72', K.noise_free_loop(24, 33, 72))):
        got = _run(g)
        print(f"{name}: {got['status']} in {got['iters']} rounds, cost {got['cost0']:.3e} -> {got['cost']:.3e}, max |pose - truth| {np.abs(got['poses'] - g['truth']).max():.2e}")
        assert got['status'] == 'converged' and np.abs(got['poses'] - g['truth']).max() <= 1e-9, name
    g = K.ring_graph(1, 2, 1)                        # the smallest tree: its one noisy edge is met exactly, the cost goes to 0 and the step size stops the run
    got = _run(g)
    want = O.initial_poses(2, g['edges'], g['T'], 0)
    print(f"2/1: {got['status']} in {got['iters']} rounds, cost {got['cost']:.3e}")
    assert got['status'] == 'converged' and got['iters'] <= 4 and np.abs(got['poses'] - want).max() <= 1e-9


@pytest.mark.parametrize('CE', list(K.OUTLIERS))
def test_outliers_are_voted_down(CE):
    """The thresholds tests/test_pose_graph_oracle.py asserts on the oracle's run of the same seeds."""
    C, E = CE
    g = K.with_outliers(C, E)
    got, plain = _run(g, tau=K.TAU), _run(g)
    out = np.zeros(E, bool); out[g['outliers']] = True
    err = lambda P: (max(np.rad2deg(np.arccos(np.clip((np.trace(a[:3, :3].T @ b[:3, :3]) - 1) / 2, -1, 1))) for a, b in zip(P, g['truth'])),
                     float(np.abs(P[:, :3, 3] - g['truth'][:, :3, 3]).max()))
    er, ep = err(got['poses']), err(plain['poses'])
    print(f"{C}/{E}: outlier weights <= {got['weights'][out].max():.2e}, inlier weights >= {got['weights'][~out].min():.3f}, "
          f"error {er[0]:.2f} deg / {er[1] * 100:.1f} cm with tau, {ep[0]:.2f} deg / {ep[1] * 100:.1f} cm without")
    assert got['weights'][out].max() < 0.05 and got['weights'][~out].min() > 0.5
    assert er[0] < ep[0] and er[1] < ep[1]


def test_bits_do_not_depend_on_the_batch():
    from roreg_amd import hip
    gs = [K.matched(12, 21), K.matched(3, 3), K.solve_edge(28), K.with_outliers(12, 21), K.ring_graph(1, 2, 1)]
    alone = [_host(hip.pg_optimize_batch([_graph(g, tau=K.TAU)], 100)) for g in gs]
    for order in (list(range(5)), list(range(5))[::-1]):
        dev = hip.pg_optimize_batch([_graph(gs[k], tau=K.TAU) for k in order], 100)
        for b, k in enumerate(order):
            got = _host(dev, b)
            for f in ('poses', 'weights', 'chi2', 'history'):
                assert _bits(got[f]) == _bits(alone[k][f]), (order, k, f)
            assert (got['iters'], got['status']) == (alone[k]['iters'], alone[k]['status'])
            assert _bits(np.float64([got['cost0'], got['cost']])) == _bits(np.float64([alone[k]['cost0'], alone[k]['cost']]))


def test_anchor_elsewhere_keeps_its_pose_bitwise():
    g = K.matched(12, 21)
    g['init'] = K.perturbed(g['truth'], 77, 2.0, 0.05, anchor=-1)            # every pose moved, the anchors' too
    for anchor in (5, 11):
        got = _run(g, anchor=anchor)
        ref = _ref(('anchor', anchor), g, anchor=anchor)[1]
        _same_run(got, ref, f'anchor {anchor}')
        assert _bits(got['poses'][anchor]) == _bits(g['init'][anchor])


def _small(edges, seed=9, C=None, noise=True):
    """a graph on given edges with consistent noisy transforms"""
    rng = np.random.default_rng(seed)
    C = C or int(np.max(edges)) + 1
    truth = np.stack([np.eye(4)] + [K.random_pose(rng, 90.0, 1.5) for _ in range(C - 1)])
    T = np.stack([O.rigid_inv(truth[i]) @ truth[j] @ (K.random_pose(rng, 0.5, 0.005) if noise else np.eye(4)) for i, j in edges])
    return dict(C=C, edges=np.asarray(edges, np.int64), T=T, Lam=np.stack([K.information(rng) for _ in edges]), truth=truth)


def test_duplicate_edges_both_orientations_and_a_leaf():
    g = _small([(0, 1), (1, 0), (0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 2), (5, 3)])          # node 5 is a leaf, entered against its edge's direction
    _same_run(_run(g), _ref(('dup',), g)[1], 'duplicates + leaf')


def test_unreachable_nodes_keep_their_pose():
    g = _small([(0, 1), (1, 2), (2, 0), (4, 5)], C=7)                                           # 3 has no edge, 4-5 is a component of its own, 6 none
    g['init'] = K.perturbed(g['truth'], 5, 3.0, 0.05, anchor=-1)
    got = _run(g)
    ref = _ref(('unreach',), g)[1]
    _same_run(got, ref, 'unreachable')
    assert got['reached'].tolist() == [True, True, True, False, False, False, False]
    assert _bits(got['poses'][3:]) == _bits(g['init'][3:]) and got['weights'][3] == 0.0
    free = _run(g, use_init=False)                                                                 # without init they sit at the identity
    assert all(_bits(free['poses'][c]) == _bits(np.eye(4)) for c in (0, 3, 4, 5, 6)) and free['status'] == 'converged'


def test_edges_without_information():
    g = _small([(0, 1), (1, 2), (2, 0), (0, 2)])
    g['Lam'][3] = 0.0
    for tau in (None, K.TAU):
        got = _run(g, tau=tau)
        _same_run(got, _ref(('lam0', tau), g, tau=tau)[1], f'Lambda = 0, tau {tau}')
        assert got['weights'][3] == 0.0 and (got['weights'][:3] > 0).all()
    h = _small([(0, 1), (1, 2), (2, 0), (3, 1)])                                                 # node 3's only edge carries no information
    h['Lam'][3] = 0.0
    got = _run(h)
    ref = _ref(('lam0 leaf',), h)[1]
    print('a node without information:', got['status'], got['iters'], got['history'][:, 2:].tolist())
    assert got['status'] == 'stalled' == ref['status'] and got['iters'] == ref['iters'] == 16 and (got['history'][:, 3] == O.DEC_PIVOT).all()
    assert np.isfinite(got['poses']).all() and np.abs(got['poses'] - ref['poses']).max() <= 1e-12


def test_max_iter_zero_and_nonfinite_input():
    g = K.matched(12, 21)
    got = _run(g, max_iter=0)
    G = O.Graph(g['C'], g['edges'], g['T'], g['Lam'])
    P0 = O.initial_poses(g['C'], g['edges'], g['T'], 0)
    assert got['status'] == 'max_iter' and got['iters'] == 0 and got['cost0'] == got['cost'] and abs(got['cost'] - G.cost(P0)) <= 1e-10 * G.cost(P0)
    assert np.abs(got['poses'] - P0).max() <= 1e-12 and np.abs(got['chi2'] - G.edge_terms(P0)[1]).max() <= 1e-9 * G.edge_terms(P0)[1].max()
    one = _run(g, max_iter=1)
    assert one['status'] == 'max_iter' and one['iters'] == 1 and one['history'][0, 3] == O.DEC_ACCEPT
    bad = dict(g, T=g['T'].copy(), init=K.perturbed(g['truth'], 3, 1.0, 0.01))
    bad['T'][7, 1, 2] = np.nan
    got = _run(bad)
    assert got['status'] == 'nonfinite' and got['iters'] == 0 and np.isnan(got['cost0']) and np.isnan(got['cost'])
    assert _bits(got['poses']) == _bits(bad['init'])
    # its neighbour in the batch is not disturbed
    from roreg_amd import hip
    both = hip.pg_optimize_batch([_graph(bad), _graph(dict(g, init=bad['init']))], 100)
    assert _host(both, 0)['status'] == 'nonfinite' and _bits(_host(both, 1)['poses']) == _bits(_run(dict(g, init=bad['init']))['poses'])


def test_residual_of_179_99_degrees():
    from roreg_amd import hip
    from roreg_amd.utils import RR_cal
    rng = np.random.default_rng(17)
    for trial in range(6):
        Pi, Pj = K.random_pose(rng, 120.0, 1.0), K.random_pose(rng, 120.0, 1.0)
        Eres = K.pose(K.rot(rng.standard_normal(3), 179.99), rng.uniform(-0.2, 0.2, 3))
        T = O.rigid_inv(Pi) @ Pj @ O.rigid_inv(Eres)                      # inv(T) inv(Pi) Pj = Eres
        L = K.information(rng)
        g = dict(C=2, edges=np.array([[0, 1]]), T=T[None], Lam=L[None], init=np.stack([Pi, Pj]))
        dev = hip.pg_optimize_batch([_graph(g)], 1, want_pieces=True)
        e = dev.pieces[0].cpu().numpy()[0, :6]
        Ehost = np.linalg.inv(T) @ np.linalg.inv(Pi) @ Pj
        want = np.concatenate([Ehost[:3, 3], RR_cal.mat2quat(Ehost[:3, :3])[1:]])
        chi2 = RR_cal.computeTransformationErr(Ehost, L) * L[0, 0]
        print(f'179.99 degrees, trial {trial}: |e - mat2quat| {np.abs(e - want).max():.2e}, chi2 {dev.pieces[0][0, 6].item()!r} against {chi2!r}')
        assert np.abs(e - want).max() <= 1e-12 and abs(dev.pieces[0][0, 6].item() - chi2) <= 1e-12 * chi2


def test_the_largest_graph_and_one_node_too_many():
    from roreg_amd import hip
    C = hip.PG_MAX_NODES
    g = K.ring_graph(256, C, 2 * C)
    dev = hip.pg_optimize_batch([_graph(g)], 1, want_pieces=True)
    got = _host(dev)
    G = O.Graph(g['C'], g['edges'], g['T'], g['Lam'])
    P0 = O.initial_poses(C, g['edges'], g['T'], 0)
    H, gr, _, _ = G.assemble(P0)
    A = G.damped(H, 1e-3)
    delta = dev.pieces[3].cpu().numpy()
    want = np.linalg.solve(A, -dev.pieces[2].cpu().numpy())
    n, cond = G.n, np.linalg.cond(A)
    P1 = G.apply(P0, want)
    c0, c1 = G.cost(P0), G.cost(P1)
    slack = 4.0 * np.linalg.norm(G.assemble(P1)[1]) * np.linalg.norm(delta - want)        # c' moves by grad c(P') . (delta - want), grad c = 2 g
    print(f'C = {C}: n = {n}, delta {np.linalg.norm(delta - want) / (8 * n * EPS * cond * np.linalg.norm(want)):.3e} of its bar (cond {cond:.2e}), '
          f'c {got["history"][0, 0]!r} -> {got["history"][0, 1]!r} (oracle {c0!r} -> {c1!r})')
    assert n == 1530 and np.linalg.norm(delta - want) <= 8 * n * EPS * cond * np.linalg.norm(want)
    assert abs(got['history'][0, 0] - c0) <= 1e-10 * c0 and abs(got['history'][0, 1] - c1) <= 1e-10 * c1 + slack and got['history'][0, 3] == O.DEC_ACCEPT
    big = K.ring_graph(257, C + 1, C + 1)
    with pytest.raises(hip.HipError):
        hip.pg_optimize_batch([_graph(big)], 1)


def test_public_interface_equals_the_binding():
    from roreg_amd import hip, pose_graph
    g, h = K.matched(12, 21), K.far_start()
    r = pose_graph.optimize(g['C'], g['edges'], g['T'], g['Lam'], robust_tau=K.TAU)
    got = _run(g, tau=K.TAU)
    assert _bits(r.poses) == _bits(got['poses']) and _bits(r.weights) == _bits(got['weights']) and _bits(r.chi2) == _bits(got['chi2'])
    assert (r.iters, r.status, r.cost0, r.cost) == (got['iters'], got['status'], got['cost0'], got['cost']) and _bits(r.history) == _bits(got['history'])
    assert r.reached.all() and r.history.shape == (r.iters, 4)
    rs = pose_graph.optimize([(h['C'], h['edges'], h['T'], h['Lam'], h['init']), (g['C'], g['edges'], g['T'], g['Lam'], g['truth'], 3)])
    assert _bits(rs[0].poses) == _bits(_run(h)['poses']) and _bits(rs[1].poses) == _bits(_run(dict(g, init=g['truth']), anchor=3)['poses'])
    pairs = [(0, 1), (4, 2)]
    Tij = pose_graph.implied_pairs(r.poses, pairs)
    assert np.abs(Tij[1] - np.linalg.inv(r.poses[4]) @ r.poses[2]).max() == 0 and Tij.shape == (2, 4, 4)


def _views(n_views, n, seed):
    """n_views dense views of one surface: (clouds float32 [n,3], poses world <- cloud)."""
    rng = np.random.default_rng(seed)
    world = synth.make_dense_pair(seed, 3 * n, noise=0.0)[0].astype(np.float64)
    poses = [np.eye(4)] + [K.random_pose(rng, 25.0, 0.3) for _ in range(n_views - 1)]
    clouds = []
    for P in poses:
        x = world[rng.permutation(world.shape[0])[:n]] + rng.normal(0, 0.002, (n, 3))
        clouds.append(np.ascontiguousarray((x - P[:3, 3]) @ P[:3, :3], np.float32))
    return clouds, np.stack(poses)


def _dense_scene(ds, n, seed):
    """Dense clouds consistent with a synth.make_scene scene's poses: cloud c sees world points x_w at R_g^T (x_w - t_c)."""
    from roreg_amd.group import tables
    rng = np.random.default_rng(seed)
    world = synth.make_dense_pair(seed, 3 * n, noise=0.0)[0].astype(np.float64) + np.array([2.0, 1.5, 0.0])
    out = {}
    for c, (g, t) in enumerate(ds.poses):
        x = world[rng.permutation(world.shape[0])[:n]] + rng.normal(0, 0.002, (n, 3))
        out[c] = np.ascontiguousarray((x - t) @ tables().R[g], np.float32)
    return out


def test_engine_optimize_poses_on_a_dense_scene():
    from roreg_amd.engine import CloudState, RegistrationEngine
    eng = RegistrationEngine(default_config(), None, None)
    clouds, poses = _views(4, 3000, 41)
    states = [eng.attach_points(CloudState(before=None), c) for c in clouds]
    pairs = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2)]
    T = np.stack([np.linalg.inv(poses[i]) @ poses[j] for i, j in pairs])
    T[1] = T[1] @ K.pose(K.rot((1, 2, 3), 3.0), np.zeros(3))                               # one pair 3 degrees off
    r = eng.optimize_poses(states, pairs, T, max_dist=0.1)
    print(f'optimize_poses: {r.status} in {r.iters} rounds, cost {r.cost0:.4e} -> {r.cost:.4e}, weights {r.weights.tolist()}')
    assert r.status == 'converged' and r.cost < r.cost0 and np.isfinite(r.weights).all() and np.isfinite(r.poses).all() and r.reached.all()
    rt = eng.optimize_poses(states, pairs, _dev(T), max_dist=0.1, robust_tau=0.05, max_iter=50)
    assert np.isfinite(rt.weights).all() and (rt.weights > 0).all() and (rt.weights <= 1).all() and rt.cost < rt.cost0


def test_run_distributed_multiway_writes_the_poses(tmp_path):
    """run_distributed.evaluate at world size 1 on a synthetic scene with dense clouds: the multiway step writes multiway_poses.log under
    output_cache_fn (nothing under the dataset directory), RR_cal.read_trajectory reads the poses back bit for bit, and the pairwise results
    are what they are without it."""
    from roreg_amd import run_distributed as RD_
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.network import name2network
    from roreg_amd.utils import RR_cal
    z = load_golden('pipeline_mutual_yohoo')
    root = tmp_path / 'mw'
    root.mkdir()
    cfg = default_config(output_cache_fn=f'{root}/cache', model_fn=f'{root}/ckpt', base_dir=str(root), SO3_related_files=None, keynum=int(z['keynum']),
                         bs_GF=50, bs_ET=40, ET='yohoo', testset='synth')
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
    ds.write_inputs(cfg.output_cache_fn)
    data = root / 'data'
    data.mkdir()
    from roreg_amd.test.estimator import pre_log_entry
    ds.gt_dir = f'{data}/gt.log'
    with open(ds.gt_dir, 'w') as f:
        for a, b in ds.pair_ids:
            f.write(pre_log_entry(a, b, len(ds.pc_ids), np.concatenate([ds.get_transform(a, b).astype(np.float64), [[0, 0, 0, 1]]])))
    dense = _dense_scene(ds, 4000, 31)
    ds.get_pc = lambda i, dense=dense: dense[int(i)]
    datasets = {'wholesetname': 'synth', 'scene0': ds}
    eng = RegistrationEngine(cfg, gf, et)
    out = RD_.evaluate(cfg, datasets, eng, rank=0, world=1, seed=3, multiway=dict(max_dist=0.05, tau=0.1))
    plain = RD_.evaluate(cfg, datasets, eng, rank=0, world=1, seed=3)
    assert set(out) - set(plain) == {'multiway'} and all(out[k] == plain[k] or (np.isnan(out[k]) and np.isnan(plain[k])) for k in plain)
    path = out['multiway']['files'][ds.name]
    assert path == f'{cfg.output_cache_fn}/{ds.name}/multiway_poses.log' and os.path.exists(path) and os.listdir(data) == ['gt.log']
    keys, poses = RR_cal.read_trajectory(path)
    assert keys[:, 0].tolist() == [str(int(c)) for c in ds.pc_ids] and poses.shape == (len(ds.pc_ids), 4, 4)
    assert _bits(poses) == _bits(out['multiway']['poses'][ds.name])
    assert np.isfinite(poses).all() and _bits(poses[0]) == _bits(np.eye(4)) and 0.0 <= out['multiway']['rr'] <= 1.0
    log = open(f'{cfg.base_dir}/results.log').read()
    assert '-multiway' in log and f"(pairwise {out['rr']:.5f})" in log
    print('multiway:', out['multiway'])
