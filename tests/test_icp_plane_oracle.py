"""Point-to-plane ICP, the parts that need no GPU: the numpy oracle (tests/_icp_plane_oracle.py) against its own unpruned neighbourhoods, the
conditions under which each input family of tests/_icp_plane_cases.py reaches its branch, the oracle's convergence against the point method
on the convergence pair, and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _icp_cases as C
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
from roreg_amd import synth


def _ratio(lam):
    return lam[:, 1] / np.where(lam[:, 2] > 0, lam[:, 2], 1.0)


def _clear_of_validity_threshold(ref):
    """No neighbourhood with lambda_mid / lambda_max within a decade of 1e-8 (an all-zero C, one repeated point, is clear: its ratio is 0 / 0,
    invalid by lambda_mid > 1e-8 lambda_max whatever rounding does)."""
    r = _ratio(ref.lam)
    return not (((r > 1e-9) & (r < 1e-7)) & (ref.lam[:, 2] > 0)).any()


def test_pruned_neighbourhoods_are_the_brute_force_ones():
    p = synth.make_dense_pair(3, 3000)[0]
    p[5] = p[100]; p[7] = p[100]
    for r in (0.05, 0.1, 0.3):
        a, b = PO.normals(p, r), PO.normals_full(p, r)
        assert np.array_equal(a.counts, b.counts) and np.array_equal(a.valid, b.valid)
        assert a.counts[5] == a.counts[100] == a.counts[7] >= 3
        assert np.abs(a.lam - b.lam).max() <= 1e-12 * a.lam.max()
        ok = a.valid & (PO.gap_ratio(a.lam) >= 1e-3)
        assert PO.angle_to(a.normals[ok], b.normals[ok]).max() <= 1e-10
        assert (a.normals[~a.valid] == 0).all() and np.abs((a.normals[a.valid] ** 2).sum(1) - 1).max() < 1e-14
    assert 0 < PO.normals(p, 0.05).valid.mean() < 1                # both verdicts occur


def test_normals_do_not_depend_on_where_the_cloud_sits():
    """The offsets y = x_j - x_i of float32 coordinates are exact, so a cloud moved by a representable shift gives the same table."""
    p = (np.round(synth.make_dense_pair(3, 1500)[0] * 1024) / 1024).astype(np.float32)         # multiples of 2^-10: a shift by 64 is exact
    a, b = PO.normals_full(p, 0.2), PO.normals_full(p + np.float32(64.0), 0.2)
    assert np.array_equal(a.table, b.table)


def test_dense_family_exclusion_shares():
    ref = PC.dense_reference()
    gap = PO.gap_ratio(ref.lam)
    left_out = (gap[ref.valid] < 1e-3).mean()
    print(f'dense: {ref.valid.mean() * 100:.2f} % valid, counts {ref.counts.min()}..{ref.counts.max()}, {left_out * 100:.4f} % of the valid left out by the gap rule')
    assert left_out <= 1e-4
    assert _clear_of_validity_threshold(ref)
    assert 0.99 < ref.valid.mean() < 1.0 and (ref.counts[~ref.valid] < PC.MIN_NB).any()
    assert np.array_equal(ref.counts[200:260], ref.counts[7000:7060]) and (ref.counts[200:260] >= 2).all()
    conv = PC.conv_normals(PC.CYCLE_RADIUS)
    print(f'convergence pair, radius 0.1: {conv.valid.mean() * 100:.2f} % valid, {(PO.gap_ratio(conv.lam)[conv.valid] < 1e-2).mean() * 100:.3f} % with a gap ratio below 1e-2')
    assert 0.99 < conv.valid.mean() < 1.0 and PC.conv_normals(PC.CONV_RADIUS).valid.all()


@pytest.mark.parametrize('base', PC.LAT_BASES)
def test_lattice_family_conditions(base):
    """At every centre: the 6 face and the 24 corner neighbours at exactly r are in, the 30 one float32 step beyond are out, in exact arithmetic
    (every d2 is a sum of exactly representable squares)."""
    p, kind, owner = PC.lattice_case(base)
    ref = PC.lattice_reference(base)
    assert np.unique(p, axis=0).shape[0] == p.shape[0]
    x = p.astype(np.float64)
    for c in range(27):
        sat = np.flatnonzero((owner == c) & (kind != PC.KIND_CENTRE))
        y = x[sat] - x[c]
        d2 = (y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]
        at = np.isin(kind[sat], (PC.KIND_FACE, PC.KIND_CORNER))
        assert at.sum() == 30 and (d2[at] == PC.LAT_R ** 2).all() and (~at).sum() == 30 and (d2[~at] > PC.LAT_R ** 2).all()
        assert ref.counts[c] == 31
    assert _clear_of_validity_threshold(ref)
    assert np.array_equal(PO.normals(p, PC.LAT_R).counts, ref.counts)
    # the neighbours sit in other cells of the walked grids: across a face and across a corner of the r grid
    cell = np.floor((x - (x.min(0) - PC.LAT_R)) / PC.LAT_R)
    face, corner = kind == PC.KIND_FACE, kind == PC.KIND_CORNER
    assert (np.abs(cell[face] - cell[owner[face]]).sum(1) == 1).all()                          # every face neighbour: the next cell along its axis
    assert ((np.abs(cell[corner] - cell[owner[corner]]) == 1).all(1).reshape(27, -1).sum(1) >= 3).all()   # per centre: corner neighbours in the diagonal cell


def test_small_family_reaches_valid_too_few_and_collinear():
    for n in PC.SMALL_N:
        ref = PO.normals_full(PC.small_cloud(n), PC.SMALL_R)
        assert _clear_of_validity_threshold(ref)
        if n < PC.MIN_NB:
            assert not ref.valid.any() and (ref.counts <= n).all()
        if n >= 63:
            assert ref.valid.any() and (ref.counts >= PC.MIN_NB).any()
    assert (PO.normals_full(PC.small_cloud(6), 10.0).counts == 6).all() and PO.normals_full(PC.small_cloud(6), 10.0).valid.all()        # m == k is valid
    ref = PO.normals_full(PC.copies_cloud(), PC.SMALL_R)
    assert (ref.counts == 50).all() and not ref.valid.any() and (ref.lam == 0).all() and (ref.table[:, :3] == 0).all()
    ref = PO.normals_full(PC.collinear_cloud(), PC.SMALL_R)
    assert (ref.counts >= PC.MIN_NB).all() and not ref.valid.any() and (_ratio(ref.lam) < 1e-12).all()
    for p, nrm in PC.coplanar_clouds():
        ref = PO.normals_full(p, PC.SMALL_R)
        assert ref.valid.all() and (ref.counts >= PC.MIN_NB).all() and _clear_of_validity_threshold(ref)
        assert (np.abs(ref.lam[:, 0]) <= 1e-15 * ref.lam[:, 2]).all()
        assert PO.angle_to(ref.normals, np.broadcast_to(nrm, ref.normals.shape)).max() <= 1e-15
    assert (PO.normals_full(PC.coplanar_clouds()[0][0], PC.SMALL_R).lam[:, 0] == 0).all()


def test_tie_family_has_ties_and_invalid_normals_among_its_inliers():
    p0, p1, T0 = PC.tie_pair()
    for d in PC.TIE_DISTS:
        it = PC.tie_reference(d)
        assert np.isin(it['assign'], np.arange(100, 1100)).sum() > 50 and not np.isin(it['assign'], np.arange(5000, 6000)).any()
        assert 6 <= it['n_valid'] <= it['n']
        print(f'd = {d}: {it["n"]} distance inliers, {it["n_valid"]} with a valid normal, cond(A) = {np.linalg.cond(it["A"]):.1f}')
    assert PC.tie_reference(0.05)['n_valid'] < PC.tie_reference(0.05)['n']           # radius 0.1 leaves some targets without a normal
    assert _clear_of_validity_threshold(PC.tie_normals(0.05)) and _clear_of_validity_threshold(PC.tie_normals(0.1))


def test_plane_oracle_converges_in_fewer_iterations_than_the_point_oracle():
    Tg = PC.conv_pair()[2]
    for s in range(2):
        r, trace = PC.conv_reference(s, PC.CONV_RADIUS, PC.CONV_ITER)
        p = PC.conv_point_reference(s)
        e, ep = O.pose_error(r.T, Tg), O.pose_error(p.T, Tg)
        print(f'start {s}: plane {r.iters} iterations, {e[0]:.4f} deg / {e[1] * 1e3:.2f} mm from the ground truth; point {p.iters} iterations, '
              f'{ep[0]:.4f} deg / {ep[1] * 1e3:.2f} mm; cond(A) = {trace[-1]["lam"][-1] / trace[-1]["lam"][0]:.1f}')
        assert r.status == 'converged' and p.status == 'converged' and r.iters < p.iters
        assert e[0] < ep[0] and e[1] < ep[1]
        R = r.T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1) < 1e-13


def test_cycle_case_ends_in_max_iter():
    """Normal radius 0.1 from the first start: the run settles into a cycle between two assignment sets whose constant rotation step is
    below tol_deg and whose translation step is above tol_t -- both tolerances must hold, so it runs to max_iter."""
    r, trace = PC.conv_reference(0, PC.CYCLE_RADIUS, PC.CYCLE_ITER)
    assert r.status == 'max_iter' and r.iters == PC.CYCLE_ITER
    tail = trace[-8:]
    print('cycle steps:', [(f'{x["step_deg"]:.3e}', f'{x["step_t"]:.3e}') for x in tail[-3:]])
    assert all(x['step_deg'] < 1e-4 and x['step_t'] > 1e-6 for x in tail)
    assert all(abs(x['step_deg'] - tail[0]['step_deg']) < 1e-3 * tail[0]['step_deg'] for x in tail)


def test_rank_families():
    """One exact plane: three zero eigenvalues of A; two: one; three orthogonal planes: none, and the run converges.  The noisy wall's
    lambda_min / lambda_max is decades clear of 1e-10 in every iteration."""
    zero = {1: 3, 2: 1, 3: 0}
    for n in PC.RANK_PLANES:
        r, trace = PC.planes_reference(n)
        nrm = PC.planes_normals(n)
        assert nrm.valid.all() and (np.abs(nrm.normals).max(1) >= 1 - 1e-15).all()              # every normal is an axis
        lam = trace[0]['lam']
        assert int((lam <= 1e-12 * lam[-1]).sum()) == zero[n] and (lam[zero[n]:] > 1e-3 * lam[-1]).all()
        if n < 3:
            assert r.status == 'no_support' and r.iters == 1 and r.inliers >= 6 and np.array_equal(r.T, PC.planes_pair(n)[3])
        else:
            e = O.pose_error(r.T, PC.planes_pair(n)[2])
            print(f'three planes: {r.iters} iterations, {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm from the ground truth')
            assert r.status == 'converged' and e[0] < 0.02 and e[1] < 5e-4
    for seed in PC.WALL_SEEDS:
        r, trace = PC.wall_reference(seed)
        ratios = [x['lam'][0] / x['lam'][-1] for x in trace]
        print(f'wall seed {seed}: {r.iters} iterations, {r.status}, lambda_min / lambda_max in [{min(ratios):.1e}, {max(ratios):.1e}]')
        assert min(ratios) > 1e-9 and r.status in ('converged', 'max_iter')


def test_chunk_family_oracle_results():
    refs = PC.chunk_reference()
    names = [c[0] for c in PC.chunk_pairs()]
    assert names == [f'src{n}' for n in PC.CHUNK_SRC_N]
    assert refs[0][1].status == 'no_support' and refs[0][1].inliers < 6
    for it, r in refs[1:]:
        assert r.status == 'converged' and 6 <= it['n_valid'] <= it['n'] and r.iters < C.CHUNK_ITER


def test_oracle_stop_rules_and_update():
    p0, p1, Tg = synth.make_dense_pair(2, 2000)
    N = PO.normals(p0, 0.3).table
    Tn = np.full((4, 4), np.nan); Tn[3] = [0, 0, 0, 1]
    r = PO.icp(p0, p1, N, Tn, 0.1)
    assert r.status == 'nonfinite' and r.iters == 0 and np.array_equal(r.T, Tn, equal_nan=True)
    far = Tg.copy(); far[:3, 3] += 100.0
    r = PO.icp(p0, p1, N, far, 0.1)
    assert r.status == 'no_support' and r.iters == 1 and r.inliers == 0 and np.isnan(r.rmse) and np.array_equal(r.T, far)
    r = PO.icp(p0, p1, np.zeros_like(N), Tg, 0.1)                  # no valid normal anywhere
    assert r.status == 'no_support' and r.inliers == 0 and np.array_equal(r.T, Tg)
    r = PO.icp(p0, p1, N, O.perturb(Tg, 3.0, 0.05, 1), 0.1, max_iter=2)
    assert r.status == 'max_iter' and r.iters == 2
    # exp([w]x): a rotation about w by |w|, the series branch continuous with the closed form
    w = np.array([0.3, -0.2, 0.1])
    dR = PO.rodrigues(w)
    assert np.abs(dR @ dR.T - np.eye(3)).max() < 1e-15 and np.abs(dR @ w - w).max() < 1e-16
    assert abs(np.rad2deg(np.sqrt((w * w).sum())) - O.rotation_step_deg(dR, np.eye(3))) < 1e-12
    assert np.abs(PO.rodrigues(w * 0.9999e-8 / 0.374) - PO.rodrigues(w * 1.0001e-8 / 0.374)).max() < 1e-11
    # one Gauss-Newton step from a small exact offset of a full-rank scene lands on it
    tgt, src, Tgp, _ = PC.planes_pair(3)
    Np = PC.planes_normals(3).table
    clean = ((tgt[::2].astype(np.float64) - Tgp[:3, 3]) @ Tgp[:3, :3]).astype(np.float32)
    r = PO.icp(tgt, clean, Np, O.perturb(Tgp, 0.01, 1e-4, 3), 0.1, max_iter=3)
    assert max(O.pose_error(r.T, Tgp)) < 1e-6


def test_plane_entries_are_declared_bound_and_exported():
    from roreg_amd import hip, icp, _abi
    header = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert 'v6d' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(roreg_\w+)\s*\(', code))
    names = {'roreg_icp_normals', 'roreg_icp_plane_batch_workspace', 'roreg_icp_plane_batch'}
    assert names <= declared and names <= set(_abi.PROTOTYPES) and 'roreg_icp_plane_task' in code
    assert int(re.search(r'#define\s+ROREG_ABI_VERSION\s+(\d+)', header).group(1)) == 6 == _abi.ABI_VERSION
    L = hip.lib()
    for name in names:
        assert hasattr(L, name), f'{name} is not exported'
    assert _abi._ICP_PLANE_TASK.itemsize == 40 and _abi._ICP_TASK.itemsize == 32
    assert _abi.PROTOTYPES['roreg_icp_plane_batch'] == _abi.PROTOTYPES['roreg_icp_batch']
    assert hip.PROFILE_SLOTS['icp_plane'] == 7 and hip.PROFILE_SLOTS['icp_search'] == 6
    assert L.roreg_icp_plane_batch_workspace(3, 10) >= 3 * (32 + 128) + 10 * (8 + 29) * 8 + 10 * 1024 * 4
    with pytest.raises(ValueError):
        icp.refine(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.eye(4), max_dist=0.1, method='planes')
