"""Dense ICP refinement, the parts that need no GPU: the numpy oracle (tests/_icp_oracle.py) against scipy's k-d tree and against its own
unpruned search, its convergence on the input the GPU tests use, the synthetic dense pair, the work list, and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _icp_cases as C
import _icp_oracle as O
from roreg_amd import synth


@pytest.fixture(scope='module')
def conv_pair():
    return synth.make_dense_pair(O.CONV_SEED, O.CONV_N)


def test_dense_pair_is_seeded_and_consistent_with_its_ground_truth():
    p0, p1, T = synth.make_dense_pair(4, 6000)
    q0, q1, T2 = synth.make_dense_pair(4, 6000)
    assert p0.dtype == np.float32 and p0.shape == (6000, 3) and p1.shape == (6000, 3)
    assert np.array_equal(p0, q0) and np.array_equal(p1, q1) and np.array_equal(T, T2)
    assert not np.array_equal(p0, synth.make_dense_pair(5, 6000)[0])
    R = T[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
    # under the ground truth the shared surface points of the two views coincide up to the noise (2 mm per coordinate and view)
    a, d2 = O.nearest(p0.astype(np.float64), O.transform(p1.astype(np.float64), R, T[:3, 3]), 0.02)
    near = np.sqrt(d2[a >= 0])
    assert (a >= 0).sum() > 1500 and np.median(near) < 0.012
    # the views are partial: view 0 ends at x = a, view 1 (in the world frame) starts at x = -a
    w1 = O.transform(p1.astype(np.float64), R, T[:3, 3])
    assert p0[:, 0].max() < 0.85 and p0[:, 0].min() < -1.9 and w1[:, 0].min() > -0.85 and w1[:, 0].max() > 1.9


def test_oracle_pruned_search_is_the_full_search_and_ties_go_to_the_lowest_row():
    p0, p1, T = synth.make_dense_pair(3, 3000)
    Q = p0.astype(np.float64)
    Q[5] = Q[100]; Q[7] = Q[100]                              # rows 5, 7 and 100 are one point
    Pt = O.transform(p1.astype(np.float64), T[:3, :3], T[:3, 3])
    Pt[3] = Q[100]                                            # a query on top of it, and one that is nowhere
    Pt[9] = np.nan
    for d in (0.03, 0.1, 0.5):
        a, b = O.nearest(Q, Pt, d)
        a2, b2 = O.nearest_full(Q, Pt, d)
        assert np.array_equal(a, a2) and np.array_equal(b[a >= 0], b2[a >= 0])
        assert a[3] == 5 and b[3] == 0.0 and a[9] == -1
        assert not np.isin(a, [7, 100]).any()


def _scipy_nn(Q):
    from scipy.spatial import cKDTree
    tree = cKDTree(Q)
    seen = {}

    def nn(Q_, Pt, d):
        dist, idx = tree.query(Pt, k=2, distance_upper_bound=d * (1 + 1e-9), workers=1)
        first = np.where(idx[:, 0] < Q.shape[0], idx[:, 0], 0)
        e = Q[first] - Pt
        d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        ok = (idx[:, 0] < Q.shape[0]) & (d2 <= d * d)
        seen['tied'] = np.isfinite(dist[:, 1]) & (dist[:, 0] == dist[:, 1])
        return np.where(ok, first, -1).astype(np.int32), np.where(ok, d2, np.inf)
    return nn, seen


def test_oracle_against_scipy_kdtree(conv_pair):
    """cKDTree.query(distance_upper_bound=d) finds the assignments of the brute-force search wherever the nearest distance is not exactly
    tied, and the two iterations end at the same transform to 1e-12."""
    pytest.importorskip('scipy')
    p0, p1, Tg = conv_pair
    Q, P = p0.astype(np.float64), p1.astype(np.float64)
    T0 = O.perturb(Tg, 3.0, 0.05, O.CONV_SEED)
    nn, seen = _scipy_nn(Q)
    one = O.iterate(Q, P, T0[:3, :3], T0[:3, 3], 0.05)
    two = O.iterate(Q, P, T0[:3, :3], T0[:3, 3], 0.05, nn)
    free = ~seen['tied']
    assert free.sum() > 0.99 * free.shape[0] and one['n'] > 3000
    assert np.array_equal(one['assign'][free], two['assign'][free])
    a = O.icp(p0, p1, T0, 0.05, max_iter=50)
    b = O.icp(p0, p1, T0, 0.05, max_iter=50, nn=nn)
    print('oracle', a.iters, a.inliers, a.rmse, a.status, '| scipy', b.iters, b.inliers, b.rmse, b.status, '| max |dT|', np.abs(a.T - b.T).max())
    assert a.iters == b.iters and a.inliers == b.inliers and a.status == b.status
    assert np.abs(a.T - b.T).max() <= 1e-12


def test_oracle_convergence_on_the_gpu_tests_input(conv_pair):
    """The condition on the convergence tests' input: at d = 0.05 the oracle reaches < 0.05 degrees and < 2 mm from both starts (3 degrees
    / 5 cm and 5 degrees / 10 cm off the ground truth) within 50 iterations, at the same fixed point."""
    p0, p1, Tg = conv_pair
    ends = []
    for deg, shift in O.CONV_STARTS:
        T0 = O.perturb(Tg, deg, shift, O.CONV_SEED)
        e0 = O.pose_error(T0, Tg)
        assert abs(e0[0] - deg) < 1e-9 and abs(e0[1] - shift) < 1e-12
        r = O.icp(p0, p1, T0, 0.05, max_iter=50)
        e = O.pose_error(r.T, Tg)
        print(f'start {deg} deg / {shift} m -> {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm, {r.iters} iterations, {r.inliers} inliers, rmse {r.rmse * 1e3:.2f} mm, {r.status}')
        assert r.status == 'converged' and r.iters < 50
        assert e[0] < 0.05 and e[1] < 0.002
        R = r.T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1) < 1e-13
        ends.append(r.T)
    assert np.abs(ends[0] - ends[1]).max() < 1e-4


def test_oracle_stop_rules():
    p0, p1, Tg = synth.make_dense_pair(2, 2000)
    Tn = np.full((4, 4), np.nan); Tn[3] = [0, 0, 0, 1]
    r = O.icp(p0, p1, Tn, 0.1)
    assert r.status == 'nonfinite' and r.iters == 0 and r.inliers == 0 and np.isnan(r.rmse) and np.array_equal(r.T, Tn, equal_nan=True)
    far = Tg.copy(); far[:3, 3] += 100.0
    r = O.icp(p0, p1, far, 0.1)
    assert r.status == 'no_support' and r.iters == 1 and r.inliers == 0 and np.isnan(r.rmse) and np.array_equal(r.T, far)
    r = O.icp(p0[:2], p0[:2], np.eye(4), 0.1)
    assert r.status == 'no_support' and r.inliers == 2 and np.array_equal(r.T, np.eye(4))
    line = np.stack([np.linspace(0, 1, 50), np.zeros(50), np.zeros(50)], 1).astype(np.float32)          # collinear: rank(H) = 1
    r = O.icp(line, line, np.eye(4), 0.1)
    assert r.status == 'no_support' and r.inliers == 50
    r = O.icp(p0, p1, O.perturb(Tg, 3.0, 0.05, 1), 0.1, max_iter=2)
    assert r.status == 'max_iter' and r.iters == 2


def test_work_list_gives_every_pair_its_own_slots_and_one_stream():
    from roreg_amd import hip
    sizes = [50000, 1, 1024, 1025, 0, 300000, 4096, 77, 20000, 20000, 9]
    slot0, work, total = hip.icp_work_list(sizes)
    chunks = [-(-n // hip.ICP_CHUNK) for n in sizes]
    assert total == sum(chunks) and np.array_equal(slot0, np.concatenate([[0], np.cumsum(chunks)[:-1]]))
    real = work[work[:, 0] >= 0]
    assert sorted(map(tuple, real.tolist())) == [(p, c) for p in range(len(sizes)) for c in range(chunks[p])]        # each (pair, chunk) once
    assert work.shape[0] % 8 == 0 and (work[work[:, 0] < 0] == -1).all()
    for p in range(len(sizes)):                                # eight pairs or more: a pair's rows sit in one of the eight interleaved streams
        assert len(set(np.flatnonzero(work[:, 0] == p) % 8)) <= 1
    # a pair's slot count and chunk numbering are the pair's own: the same in any other batch
    s2, w2, _ = hip.icp_work_list([sizes[5]])
    assert s2[0] == 0 and sorted(w2[w2[:, 0] == 0, 1].tolist()) == list(range(chunks[5]))
    assert len(set(np.flatnonzero(w2[:, 0] == 0) % 8)) == 8     # a lone pair is spread over all streams
    s3, w3, t3 = hip.icp_work_list([0, 0])
    assert t3 == 0 and w3.shape == (0, 2)


def test_icp_entries_are_declared_bound_and_exported():
    """include/roreg_hip.h declares the dense-ICP entries (marked v6c, additions under version 6), roreg_amd/_abi.py has their prototypes
    and task layouts, and the cross-compiled library exports them."""
    from roreg_amd import hip, _abi
    header = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert 'v6c' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(roreg_\w+)\s*\(', code))
    names = {'roreg_icp_grid_size', 'roreg_icp_grid_build', 'roreg_icp_batch_workspace', 'roreg_icp_batch'}
    assert names <= declared and names <= set(_abi.PROTOTYPES)
    assert 'roreg_icp_task' in code and 'roreg_icp_grid_desc' in code
    assert int(re.search(r'#define\s+ROREG_ABI_VERSION\s+(\d+)', header).group(1)) == 6 == _abi.ABI_VERSION
    L = hip.lib()
    for name in names:
        assert hasattr(L, name), f'{name} is not exported'
    assert L.roreg_abi_version() == 6
    assert _abi._ICP_GRID_DESC.itemsize == 64 and _abi._ICP_TASK.itemsize == 32
    # the host half works without a GPU: cell edge = the smallest d 2^s that keeps the table within 2^24 cells over the padded box
    room = np.array([[-2.0, -1.5, 0.0], [2.0, 1.5, 2.5]])
    desc, nbytes, ws = hip.icp_grid_desc(room, 1000, 0.05)
    assert desc['edge'][0] == 0.05 and tuple(desc['dims'][0]) == (83, 63, 53) and desc['cells'][0] == 83 * 63 * 53
    assert np.allclose(desc['origin'][0], room[0] - 0.05) and nbytes == 64 + 16 * 1000 + 4 * (83 * 63 * 53 + 2) and ws >= 16 * 1000
    big = np.array([[-40.0, -40.0, -40.0], [40.0, 40.0, 40.0]])
    d2 = hip.icp_grid_desc(big, 10, 0.05)[0]
    assert d2['edge'][0] == 0.4 and d2['cells'][0] <= 2 ** 24 and hip.icp_grid_desc(big, 10, 0.05 / 2)[0]['edge'][0] == 0.4
    assert hip.icp_grid_desc(np.zeros((2, 3)), 0, 0.1)[0]['cells'][0] == 27


# ---- the input families of tests/test_hip_icp_edges.py (tests/_icp_cases.py): each family's conditions, from the oracle alone ---------------
def test_solve_family_conditions():
    """Every source point is an inlier, no nearest neighbour is decided by less than 1e-6 relative, at least a quarter of the solved pairs
    take the determinant fix, at least a tenth of all pairs are rejected by rank, no pair sits where the rank verdict is arbitrary (at most
    2 % were dropped for that), and H spans more than twelve decades."""
    pairs, refs, dropped = C.solve_family()
    assert len(pairs) + dropped == C.SOLVE_PAIRS and dropped <= 0.02 * C.SOLVE_PAIRS
    assert all(3 <= c['P'].shape[0] <= 8 and c['Q'].shape == c['P'].shape for c in pairs)
    assert all(r['it']['n'] == c['P'].shape[0] and (r['it']['assign'] >= 0).all() for c, r in zip(pairs, refs))
    margin = min(float(((r['d2'][:, 1] - r['d2'][:, 0]) / r['d2'][:, 1]).min()) for r in refs)
    solved = [r for r in refs if r['R'] is not None]
    reflected = sum(r['sign'] < 0 for r in solved)
    ratio = np.array([r['S'][1] / r['S'][0] for r in refs])
    s1 = np.array([r['S'][0] for r in refs])
    print(f'{len(pairs)} pairs ({dropped} dropped), {len(solved)} solved, {reflected} with det(U V^T) = -1, {len(refs) - len(solved)} rejected by rank, smallest tie '
          f'margin {margin:.2e}, sigma1 from {s1.min():.1e} to {s1.max():.1e}, bound from {min(map(C.solve_bound, solved)):.1e} to {max(map(C.solve_bound, solved)):.1e}')
    assert margin >= 1e-6
    assert reflected >= 0.25 * len(solved) and len(refs) - len(solved) >= 0.10 * len(refs)
    assert not ((ratio >= C.SOLVE_BAND[0]) & (ratio <= C.SOLVE_BAND[1])).any()
    assert all(r['status'] == ('no_support' if q <= 1e-10 else 'max_iter') for r, q in zip(refs, ratio))
    assert s1.max() / s1.min() > 1e12
    for r in solved:                                           # the oracle's own rotations are proper, the reflected ones too
        assert np.abs(r['R'] @ r['R'].T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(r['R']) - 1) < 1e-13
    # every family is solved with both determinant signs, except the two collinear ones, which are rejected
    for f in range(len(C.SOLVE_FAMILIES)):
        signs = {r['sign'] for c, r in zip(pairs, refs) if c['family'] == f and r['R'] is not None}
        assert signs == (set() if C.SOLVE_FAMILIES[f][1] < 1e-6 else {-1.0, 1.0}), f


def test_solve_full_is_solve_with_its_factors():
    pairs, refs, _ = C.solve_family()
    for r in refs[:40]:
        one = O.solve(r['it']['H'], r['it']['cq'], r['it']['cp'])
        assert (one is None) == (r['R'] is None)
        if one is not None:
            assert np.array_equal(one[0], r['R']) and np.array_equal(one[1], r['t'])
    assert O.solve_full(np.full((3, 3), np.nan), np.zeros(3), np.zeros(3))[0] is None


@pytest.mark.parametrize('dims', C.GRID_DIMS)
def test_grid_family_gives_the_chosen_tables(dims):
    """max_dist = 1 over the box [0, dims - 2.5]: exactly these dims at edge 1.0, and the word counts the scan's boundaries are about."""
    from roreg_amd import hip
    p, box = C.grid_case(dims)
    desc = hip.icp_grid_desc(box, p.shape[0], 1.0)[0]
    assert tuple(int(v) for v in desc['dims'][0]) == dims and desc['edge'][0] == 1.0 and int(desc['cells'][0]) == int(np.prod(dims))
    assert np.array_equal(desc['origin'][0], [-1.0, -1.0, -1.0])
    assert (p >= 0).all() and (p <= box[1]).all() and p.dtype == np.float32
    order, starts, cid = C.grid_expected(p, desc['origin'][0], 1.0, dims)
    assert starts[-1] == p.shape[0] and starts.shape[0] == np.prod(dims) + 1
    if dims == (3, 3, 3):
        assert p.shape[0] == 1 and cid[0] == 13
        return
    interior = lambda c: (c[2] * dims[1] + c[1]) * dims[0] + c[0]
    first, last = interior((1, 1, 1)), interior(tuple(v - 2 for v in dims))
    assert cid.min() == first and cid.max() == last                      # the padding cells stay empty
    assert (cid == first).sum() >= 250 and (cid == last).sum() >= 250 and np.array_equal(p[100:140], p[2000:2040])
    assert len(np.unique(cid)) > (500 if np.prod(dims) > 5000 else 100)


def test_grid_family_sits_on_the_scan_boundaries():
    words = [int(np.prod(d)) + 1 for d in C.GRID_DIMS]
    blocks = [-(-w // 4096) for w in words]
    assert words[1] == 4096 and words[2] == 4097 and blocks == [1, 1, 2, 256, 257, 4097] and words[5] == 2 ** 24 + 1


def test_chunk_family_oracle_results():
    """The oracle's side of the chunk family: which sizes converge, which have no support."""
    ref = dict(zip([c[0] for c in C.chunk_pairs()], C.chunk_reference()))
    for n in (1, 2, 3):
        assert ref[f'src{n}'].status == 'no_support' and ref[f'src{n}'].iters == 1 and ref[f'src{n}'].inliers < 3
    assert [ref[f'src{n}'].inliers for n in (63, 64, 65)] == [27, 28, 29] and [ref[f'src{n}'].inliers for n in (1023, 1024, 1025)] == [500, 500, 501]
    for n in C.CHUNK_SRC_N[3:]:
        assert ref[f'src{n}'].status == 'converged' and 1 < ref[f'src{n}'].iters < C.CHUNK_ITER
    assert ref['src2047'].inliers > 1000 and ref['src3073'].inliers > 1500
    for n in (1, 2):
        assert (ref[f'tgt{n}'].status, ref[f'tgt{n}'].iters, ref[f'tgt{n}'].inliers) == ('no_support', 1, 0)
    assert (ref['tgt3'].status, ref['tgt3'].iters, ref['tgt3'].inliers) == ('no_support', 1, 3)           # three inliers of ONE target point: H = 0
    for n in (64, 1025):                                       # many source points per target point: a slow tail, all CHUNK_ITER searches run
        assert ref[f'tgt{n}'].status == 'max_iter' and ref[f'tgt{n}'].iters == C.CHUNK_ITER and ref[f'tgt{n}'].inliers > n
    print({k: (v.iters, v.inliers, v.status) for k, v in ref.items()})


@pytest.mark.parametrize('base', C.THR_BASES)
def test_threshold_family_conditions(base):
    """At least 100 queries at d2 == d^2 exactly (all inliers), at least 100 that one float32 step of one coordinate makes outliers, corner
    queries on both sides of d^2, and exact ties at the threshold that go to the lowest row."""
    d = C.THR_DIST
    Q, P, kind = C.threshold_case(base)
    a, d2 = C.threshold_reference(base)
    assert np.array_equal(Q[:27] * 64, np.round(Q[:27] * 64)) and Q.dtype == P.dtype == np.float32
    exact = d2 == d * d
    assert exact.sum() >= 100 and (a[exact] >= 0).all() and exact[kind == C.KIND_FACE].all() and exact[kind == C.KIND_TIE].all()
    beyond = kind == C.KIND_BEYOND
    assert beyond.sum() >= 100 and (a[beyond] < 0).all()
    step = np.abs(P[beyond].astype(np.float64) - P[kind == C.KIND_FACE].astype(np.float64)).sum(1)       # one float32 step of one coordinate
    assert (step > 0).all() and (step <= np.spacing(np.abs(P[beyond]).max(1))).all()
    corner = kind == C.KIND_CORNER
    assert (a[corner] >= 0).sum() >= 100 and (a[corner] < 0).sum() >= 100
    assert np.array_equal(a[corner & (a >= 0)], np.repeat(np.arange(27), len(C.THR_CORNERS) * 8)[(a >= 0)[corner]])
    assert np.array_equal(a[kind == C.KIND_TIE], [27, 29, 31, 33, 35, 37])
    # the lattice points lie on cell faces of the grids of all three radii: a face query's target is in the neighbouring cell
    for g in C.THR_GRID_DISTS:
        c = (Q[:27].astype(np.float64) - (Q[:27].min(0) - g)) / g
        assert np.array_equal(c, np.round(c))


def test_wall_family_passes_through_the_determinant_fix():
    assert len(C.WALL_SEEDS) >= 2
    for seed in C.WALL_SEEDS:
        q, p, Tg, T0 = C.wall_pair(seed)
        assert q.shape == (1200, 3) and p.shape == (960, 3)
        signs = C.det_signs(q, p, T0, C.WALL_DIST, C.WALL_ITER)
        want = C.wall_reference(seed)
        print(seed, signs, want.iters, want.inliers, want.status)
        assert -1.0 in signs and len(signs) == want.iters and want.status == 'converged' and want.inliers > 900
        R = want.T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1) < 1e-13
        e = O.pose_error(want.T, Tg)
        assert e[0] < 0.5 and e[1] < 0.01                      # (in-plane motion is constrained by the square's outline only)
