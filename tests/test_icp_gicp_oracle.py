"""Plane-to-plane (generalized) ICP, the parts that need no GPU: the C-ABI declarations, the numpy oracle (tests/_icp_gicp_oracle.py) against
independent statements of what it sums, the conditions under which each input family of tests/_icp_gicp_cases.py reaches its branch, and the
plain-C++ weight matrix of csrc/icp_math.h in a stand-alone host program under the host sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _icp_cases as C
import _icp_gicp_cases as GC
import _icp_gicp_oracle as GO
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
from roreg_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _unit(rng, k):
    v = rng.standard_normal((k, 3))
    return v / np.sqrt((v * v).sum(1))[:, None]


def test_gicp_entries_are_declared_bound_and_exported():
    from roreg_amd import hip, icp, _abi
    header = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert 'v6i' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(roreg_\w+)\s*\(', code))
    names = {'roreg_icp_gicp_batch_workspace', 'roreg_icp_gicp_batch'}
    assert names <= declared and names <= set(_abi.PROTOTYPES) and 'roreg_icp_gicp_task' in code
    assert int(re.search(r'#define\s+ROREG_ABI_VERSION\s+(\d+)', header).group(1)) == 6 == _abi.ABI_VERSION
    L = hip.lib()
    for name in names:
        assert hasattr(L, name), f'{name} is not exported'
    assert L.roreg_abi_version() == 6
    # the record: the header's field order, 56 bytes, epsilon a double at offset 40
    body = re.search(r'typedef struct roreg_icp_gicp_task \{(.*?)\}', code, flags=re.S).group(1)
    assert re.findall(r'(\w+);', body) == ['tgt_grid', 'src_grid', 'tgt_normals', 'src_normals', 'T0', 'epsilon', 'n_src', 'slot0']
    assert _abi._ICP_GICP_TASK.names == ('tgt_grid', 'src_grid', 'tgt_normals', 'src_normals', 'T0', 'epsilon', 'n_src', 'slot0')
    assert _abi._ICP_GICP_TASK.itemsize == 56 and _abi._ICP_GICP_TASK.fields['epsilon'][1] == 40 and _abi._ICP_GICP_TASK.fields['epsilon'][0] == np.float64
    assert _abi._ICP_PLANE_TASK.itemsize == 40 and _abi._ICP_TASK.itemsize == 32
    assert _abi.PROTOTYPES['roreg_icp_gicp_batch'] == _abi.PROTOTYPES['roreg_icp_plane_batch']
    assert _abi.PROTOTYPES['roreg_icp_gicp_batch_workspace'] == _abi.PROTOTYPES['roreg_icp_plane_batch_workspace']
    assert L.roreg_icp_gicp_batch_workspace(3, 10) == L.roreg_icp_plane_batch_workspace(3, 10)          # the same slot layout
    assert len(hip.PROFILE_SLOTS) == 9 and hip.PROFILE_SLOTS['icp_plane'] == 7                             # no new profile slot
    assert icp.METHODS == ('point', 'plane', 'gicp') and 'icp_gicp_batch' in hip.__dict__
    with pytest.raises(ValueError):
        icp.refine(np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.eye(4), max_dist=0.1, method='gicpp')
    assert 'whitened' in icp.IcpResult.__doc__.lower()


def test_covariance_identity_and_closed_form_inverse():
    """V diag(1, 1, eps) V^T with n the eigenvector of eps is I - (1 - eps) n n^T; the weight is the inverse of C_q + R C_p R^T built that way;
    the closed-form inverse holds against numpy.linalg.inv where S is worst conditioned (n_q = +-m), at eps = 1e-3 and 1e-6."""
    rng = np.random.default_rng(0x61c)
    n, m = _unit(rng, 400), _unit(rng, 400)
    for eps in (1e-3, 1e-6, 0.3, 1.0):
        C_of = []
        for v in (n, m):
            # an orthonormal frame with v as its third axis
            u = np.cross(v, _unit(rng, v.shape[0])); u /= np.sqrt((u * u).sum(1))[:, None]
            w = np.cross(v, u)
            V = np.stack([u, w, v], 2)
            Cv = V @ np.diag([1.0, 1.0, eps])[None] @ V.transpose(0, 2, 1)
            assert np.abs(Cv - (np.eye(3)[None] - (1 - eps) * v[:, :, None] * v[:, None, :])).max() <= 1e-15
            C_of.append(Cv)
        M = GO.weights(n, m, eps)                                     # (asserts against numpy.linalg.inv inside)
        assert np.abs(M - np.linalg.inv(C_of[0] + C_of[1])).max() <= 1e-12 * np.abs(M).max()
        for other in (n, -n):                                         # eigenvalues 2, 2, 2 eps
            Mw = GO.weights(n, other, eps)
            assert np.abs(np.linalg.eigvalsh(Mw) - np.array([0.5, 0.5, 0.5 / eps])[None]).max() <= 1e-9 * 0.5 / eps
            assert np.array_equal(Mw, GO.weights(n, n, eps))          # the sign of a normal is not in n n^T
    zero = np.zeros((5, 3))
    assert np.array_equal(GO.weights(zero, zero, 1e-3), np.broadcast_to(0.5 * np.eye(3), (5, 3, 3)))
    assert np.array_equal(GO.weights(n, m, 1.0), np.broadcast_to(0.5 * np.eye(3), (400, 3, 3)))


def test_sums_are_the_whitened_gauss_newton_model():
    """With the assignments and M held fixed, the cost f(w, v) = sum r^T M r of the residuals r = dR (p' - c) + c + v - q, dR = exp([w]x), is
    f0 - 2 b^T x + x^T A x to second order: checked with true rotations at |x| = 1e-5, and f0 = sum d^T M d; every inlier counts."""
    p0, p1, Tg = synth.make_dense_pair(2, 1500)
    T0 = O.perturb(Tg, 1.0, 0.02, 2)
    Q, P = PO.widen(p0), PO.widen(p1)
    Nq, Np = PO.normals(p0, 0.3).table, PO.normals(p1, 0.3).table
    Np[::7, :3] = 0.0; Nq[::5, :3] = 0.0                              # some rows without a normal on either side
    R, t = T0[:3, :3], T0[:3, 3]
    it = GO.iterate(Q, P, Nq, Np, R, t, 0.1)
    sel = it['assign'] >= 0
    assert it['n'] == int(sel.sum()) > 300 and (Nq[it['assign'][sel], :3] == 0).all(1).any() and (Np[sel, :3] == 0).all(1).any()
    assert np.array_equal(it['assign'], O.nearest(Q, O.transform(P, R, t), 0.1)[0])
    M = GO.weights(Nq[it['assign'][sel], :3], Np[sel, :3] @ R.T, GO.EPSILON)
    pt, q = O.transform(P[sel], R, t), Q[it['assign'][sel]]

    def cost(x):
        r = (pt - it['c']) @ PO.rodrigues(x[:3]).T + it['c'] + x[3:] - q
        return float(np.einsum('ki,kij,kj->', r, M, r))
    f0 = cost(np.zeros(6))
    assert abs(f0 - it['sum_md']) <= 1e-12 * f0
    assert np.abs(it['A'] - it['A'].T).max() <= 1e-12 * np.abs(it['A']).max() and np.linalg.eigvalsh(it['A']).min() > 0
    rng = np.random.default_rng(5)
    for _ in range(6):
        x = rng.standard_normal(6); x *= 1e-5 / np.sqrt((x * x).sum())
        model = f0 - 2.0 * it['b'] @ x + x @ it['A'] @ x
        lin = abs(2.0 * it['b'] @ x)
        assert abs(cost(x) - model) <= 1e-3 * lin + 1e-9 * f0, (cost(x) - f0, model - f0)           # third order in |x|, against a first-order term
    # the translation block of J^T M J is M itself
    assert np.abs(it['A'][3:, 3:] - M.sum(0)).max() <= 1e-12 * np.abs(M).max() * it['n']


@pytest.mark.parametrize('radius', GC.CONV_RADII)
def test_conv_family_converges_where_the_plane_method_cycles_and_ends_closer(radius):
    """The convergence pair, d = 0.1, from both starts: converged in fewer than 10 iterations at either normal radius (the plane method runs
    to max_iter at 0.1), cond(A) stays small, and the end is closer to the ground truth than the plane method's (radius 0.2, where it
    converges) and the point method's."""
    Tg = PC.conv_pair()[2]
    for s in range(2):
        r, trace = GC.conv_reference(s, radius)
        cond = max(x['lam'][-1] / x['lam'][0] for x in trace)
        e = O.pose_error(r.T, Tg)
        print(f'radius {radius}, start {s}: {r.status} in {r.iters} iterations, {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm from the ground truth, cond(A) <= {cond:.1f}, '
              f'{r.inliers} inliers, whitened rmse {r.rmse:.5f}, verdict margin {GC.verdict_margin(trace):.2f}')
        assert r.status == 'converged' and r.iters < 10 and cond < 20
        assert GC.verdict_margin(trace) > 2.0
        assert r.inliers == int((r.assign >= 0).sum())
        if radius == PC.CYCLE_RADIUS:
            plane, _ = PC.conv_reference(s, PC.CONV_RADIUS, PC.CONV_ITER)
            point = PC.conv_point_reference(s)
            ep, ept = O.pose_error(plane.T, Tg), O.pose_error(point.T, Tg)
            print(f'    plane (radius {PC.CONV_RADIUS}): {plane.iters} iterations, {ep[0]:.4f} deg / {ep[1] * 1e3:.3f} mm; point: {point.iters} iterations, {ept[0]:.4f} deg / {ept[1] * 1e3:.3f} mm')
            assert e[0] < ep[0] and e[1] < ep[1] and e[0] < ept[0] and e[1] < ept[1]
            assert r.iters < plane.iters < point.iters
    if radius == PC.CYCLE_RADIUS:
        assert PC.conv_reference(0, PC.CYCLE_RADIUS, PC.CYCLE_ITER)[0].status == 'max_iter'            # what the plane method does here
        assert 0.99 < GC.conv_source_normals(radius).valid.mean() < 1.0                                  # some source rows carry no normal


def test_rank_families_converge_with_the_support_ratio_clear():
    """One, two and three exact planes: epsilon regularises what the plane method refuses (rank 3 and 5), every run converges with
    lambda_min / lambda_max decades above 1e-10; the noisy walls too.  No verdict within a factor 2 of a tolerance."""
    for n in GC.RANK_PLANES:
        r, trace = GC.planes_reference(n)
        ratio = min(x['lam'][0] / x['lam'][-1] for x in trace)
        e = O.pose_error(r.T, PC.planes_pair(n)[2])
        print(f'{n} planes: {r.status} in {r.iters} iterations, lambda_min / lambda_max >= {ratio:.2e}, {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm from the ground truth, '
              f'margin {GC.verdict_margin(trace):.2f}')
        assert r.status == 'converged' and ratio > 1e-10 and ratio > 1e-5 and GC.verdict_margin(trace) > 2.0
        assert GC.planes_source_normals(n).valid.all()
        if n < 3:
            assert PC.planes_reference(n)[0].status == 'no_support'
    assert min(x['lam'][0] / x['lam'][-1] for x in GC.planes_reference(1)[1]) < 1e-3                    # (the single plane is the weakest: about 1.7e-4)
    for seed in GC.WALL_SEEDS:
        r, trace = GC.wall_reference(seed)
        ratio = min(x['lam'][0] / x['lam'][-1] for x in trace)
        print(f'wall seed {seed}: {r.status} in {r.iters} iterations, lambda_min / lambda_max >= {ratio:.2e}, margin {GC.verdict_margin(trace):.2f}')
        assert r.status == 'converged' and ratio > 1e-5 and GC.verdict_margin(trace) > 2.0 and r.inliers == 960


def test_chunk_family_oracle_results():
    refs = GC.chunk_reference()
    names = [c[0] for c in GC.chunk_pairs()]
    assert names == [f'src{n}' for n in GC.CHUNK_SRC_N] == ['src1', 'src1023', 'src1024', 'src1025', 'src3073']
    it, r, trace = refs[0]
    assert r.status == 'no_support' and r.iters == 1 and r.inliers < 6 and np.array_equal(r.T, GC.chunk_pairs()[0][3])
    for (it, r, trace), Np in zip(refs[1:], GC.chunk_source_normals()[1:]):
        print(f'{r.inliers} inliers: {r.status} in {r.iters} iterations, margin {GC.verdict_margin(trace):.2f}, {Np.valid.mean() * 100:.1f} % of the source rows carry a normal')
        assert r.status == 'converged' and r.iters < C.CHUNK_ITER and it['n'] >= 6 and GC.verdict_margin(trace) > 2.0
    assert not GC.chunk_source_normals()[0].valid.any() and 0.3 < GC.chunk_source_normals()[1].valid.mean() < 0.7


def test_epsilon_one_and_zero_tables_are_the_uniform_weighting():
    """kappa = 0 and all-zero tables both make S = 2 I exactly: identical sums, M = I / 2, and the translation block of A is n / 2 I."""
    _, q, p, T0 = GC.chunk_pairs()[4]
    Nq, Np = GC.chunk_normals().table, GC.chunk_source_normals()[4].table
    a = GC.run_one(q, p, Nq, Np, T0, C.CHUNK_DIST, epsilon=1.0)
    b = GC.run_one(q, p, np.zeros_like(Nq), np.zeros_like(Np), T0, C.CHUNK_DIST)
    for k in ('assign', 'n', 'c', 'A', 'b', 'sum_md'):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a['A'][3:, 3:], 0.5 * a['n'] * np.eye(3))
    pt = O.transform(PO.widen(p), T0[:3, :3], T0[:3, 3]); sel = a['assign'] >= 0
    assert abs(a['sum_md'] - 0.5 * ((pt[sel] - PO.widen(q)[a['assign'][sel]]) ** 2).sum()) <= 1e-12 * a['sum_md']
    c = GC.run_one(q, p, Nq, Np, T0, C.CHUNK_DIST)
    assert np.array_equal(a['assign'], c['assign']) and not np.array_equal(a['A'], c['A'])
    ra, rb = GC.run_full(q, p, Nq, Np, T0, C.CHUNK_DIST, C.CHUNK_ITER, epsilon=1.0)[0], GC.run_full(q, p, 0 * Nq, 0 * Np, T0, C.CHUNK_DIST, C.CHUNK_ITER)[0]
    assert np.array_equal(ra.T, rb.T) and ra[1:5] == rb[1:5]


def test_oracle_stop_rules():
    p0, p1, Tg = synth.make_dense_pair(2, 2000)
    Nq, Np = PO.normals(p0, 0.3).table, PO.normals(p1, 0.3).table
    Tn = np.full((4, 4), np.nan); Tn[3] = [0, 0, 0, 1]
    r = GO.icp(p0, p1, Nq, Np, Tn, 0.1)
    assert r.status == 'nonfinite' and r.iters == 0 and np.array_equal(r.T, Tn, equal_nan=True)
    far = Tg.copy(); far[:3, 3] += 100.0
    r = GO.icp(p0, p1, Nq, Np, far, 0.1)
    assert r.status == 'no_support' and r.iters == 1 and r.inliers == 0 and np.isnan(r.rmse) and np.array_equal(r.T, far)
    r = GO.icp(p0, p1, np.zeros_like(Nq), np.zeros_like(Np), O.perturb(Tg, 1.0, 0.02, 1), 0.1)         # no normal anywhere: still a full-rank problem
    assert r.status == 'converged' and r.inliers > 100
    r = GO.icp(p0, p1, Nq, Np, O.perturb(Tg, 3.0, 0.05, 1), 0.1, max_iter=2)
    assert r.status == 'max_iter' and r.iters == 2


def test_weight_matrix_in_a_host_program_under_sanitizers(tmp_path):
    """csrc/icp_math.h gicp_weight / inverse_sym3 compiled into a stand-alone host program (tests/_icp_gicp_math_check.cpp, its own main) with
    AddressSanitizer and UndefinedBehaviorSanitizer: S S^-1 = I on seeded unit-normal pairs, n_q = +-m and zero normals at eps = 1e-3, 1e-6."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'icp_gicp_math_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                           '-I' + os.path.join(ROOT, 'roreg_amd', 'csrc'), os.path.join(HERE, '_icp_gicp_math_check.cpp'), '-o', exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and p.stdout.strip().endswith('ok'), p.stdout + p.stderr
