"""Robust losses in the point-to-plane and plane-to-plane ICP ("v6p"), the parts that need no GPU: the C-ABI declarations, the numpy oracle
(tests/_icp_robust_oracle.py) against independent statements of the four weights, csrc/icp_math.h's robust_weight in a stand-alone host
program under the host sanitizers, value by value against the oracle, the argument checks of the Python layers and the command line, and the
conditions under which each input family of tests/_icp_robust_cases.py reaches what the GPU tests (tests/test_hip_icp_robust.py) use it for."""
import argparse
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _icp_cases as C
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
import _icp_robust_cases as RC
import _icp_robust_oracle as RO

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ('roreg_icp_plane_robust_batch_workspace', 'roreg_icp_plane_robust_batch', 'roreg_icp_gicp_robust_batch_workspace', 'roreg_icp_gicp_robust_batch')


def test_robust_entries_are_declared_bound_and_exported():
    from roreg_amd import hip, icp, _abi
    header = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert 'v6p' in header
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    declared = set(re.findall(r'\b(roreg_\w+)\s*\(', code))
    assert set(NAMES) <= declared and set(NAMES) <= set(_abi.PROTOTYPES)
    assert int(re.search(r'#define\s+ROREG_ABI_VERSION\s+(\d+)', header).group(1)) == 6 == _abi.ABI_VERSION
    L = hip.lib()
    for name in NAMES:
        assert hasattr(L, name), f'{name} is not exported'
    # the records: the existing record's fields, then scale, loss, reserved; the existing records unchanged
    for struct, dtype, base in (('roreg_icp_plane_robust_task', _abi._ICP_PLANE_ROBUST_TASK, _abi._ICP_PLANE_TASK),
                                ('roreg_icp_gicp_robust_task', _abi._ICP_GICP_ROBUST_TASK, _abi._ICP_GICP_TASK)):
        body = re.search(r'typedef struct %s \{(.*?)\}' % struct, code, flags=re.S).group(1)
        assert tuple(re.findall(r'(\w+);', body)) == dtype.names == base.names + ('scale', 'loss', 'reserved')
        assert dtype.itemsize == base.itemsize + 16 and dtype.fields['scale'] == (np.dtype(np.float64), base.itemsize)
        assert dtype.fields['loss'] == (np.dtype(np.int32), base.itemsize + 8)
        for name in base.names:
            assert dtype.fields[name] == base.fields[name]
    assert _abi._ICP_PLANE_TASK.itemsize == 40 and _abi._ICP_GICP_TASK.itemsize == 56
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r'ROREG_ICP_LOSS_(\w+)\s*=\s*(\d+)', code))
    assert enum == dict(_abi._ICP_LOSS, none=0) and hip.ICP_LOSSES == RO.LOSSES == ('huber', 'cauchy', 'gm', 'tukey')
    for name in ('roreg_icp_plane_robust_batch', 'roreg_icp_gicp_robust_batch'):
        assert _abi.PROTOTYPES[name] == _abi.PROTOTYPES['roreg_icp_plane_batch']
        assert _abi.PROTOTYPES[name + '_workspace'] == _abi.PROTOTYPES['roreg_icp_plane_batch_workspace']
        assert getattr(L, name + '_workspace')(3, 10) == L.roreg_icp_plane_batch_workspace(3, 10)          # the same 29-word slots
    assert len(hip.PROFILE_SLOTS) == 9                                                                   # no new profile slot
    assert 'unweighted' in icp.IcpResult.__doc__.lower()


def test_the_four_weights_against_their_definitions():
    """Each weight against a direct statement of it on a seeded sweep, its value at u = 0 and |u| = 1, continuity across |u| = 1, symmetry in
    the sign of r, and no NaN anywhere from r = 0 to an overflowing u^2."""
    rng = np.random.default_rng(0x6c)
    k = 0.03
    r = np.concatenate([rng.normal(0, 0.05, 20000), [0.0, -0.0, k, -k, np.nextafter(k, 1), np.nextafter(k, 0), 1e200, -1e200, np.inf, -np.inf]])
    u = r / k
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        want = {'huber': np.where(np.abs(u) <= 1, 1.0, 1.0 / np.abs(u)), 'cauchy': 1.0 / (1.0 + u ** 2), 'gm': (1.0 / (1.0 + u ** 2)) ** 2,
                'tukey': np.where(np.abs(u) <= 1, (1.0 - u ** 2) ** 2, 0.0)}
    at_one = {'huber': 1.0, 'cauchy': 0.5, 'gm': 0.25, 'tukey': 0.0}
    for loss in RO.LOSSES:
        w = RO.weight(loss, r, k)
        assert np.isfinite(w).all() and (w >= 0).all() and (w <= 1).all(), loss
        assert np.array_equal(w, want[loss]), loss
        assert np.array_equal(w, RO.weight(loss, -r, k)), loss
        assert RO.weight(loss, 0.0, k) == 1.0 and RO.weight(loss, k, k) == at_one[loss], loss
        both = RO.weight(loss, np.array([np.nextafter(k, 0), np.nextafter(k, 1)]), k)
        assert np.abs(both - at_one[loss]).max() <= 1e-15, loss                       # continuous: no decision rests on the last bit of r
        assert (RO.weight(loss, np.array([1e200, -1e200, np.inf]), k) == 0.0).all() or loss == 'huber'
    assert np.array_equal(RO.weight('huber', np.array([1e200, np.inf]), k), [k / 1e200, 0.0])
    assert np.array_equal(RO.weight(None, r, None), np.ones_like(r))
    # where both normals agree the gicp residual is the distance along the normal: d = s n, M = diag-like with 1 / (2 eps) along n
    eps = 1e-3
    assert abs(RO.gicp_residual(0.02 ** 2 / (2 * eps), eps) - 0.02) <= 1e-17


def _edge_table():
    """Rows (r, k, q, epsilon): the issue's edge values for every k in (1e-300, 0.03, 1, 1e300) -- r = +-0, |r| = k exactly and one ulp either
    side, r = +-1e200 k (beyond 1e308: +-inf) --, and a seeded sweep."""
    rows = []
    for k in (1e-300, 0.03, 1.0, 1e300):
        with np.errstate(over='ignore'):
            big = np.float64(1e200) * np.float64(k)
        for r in (0.0, -0.0, k, -k, np.nextafter(k, np.inf), np.nextafter(k, 0.0), -np.nextafter(k, np.inf), -np.nextafter(k, 0.0), big, -big):
            rows.append((r, k, abs(r), 1e-3))
    rows += [(0.01, 0.03, -1e-30, 1e-3), (0.01, 0.03, 0.0, 1.0), (0.01, 0.03, 1e308, 1.0), (0.01, 0.03, 4e-300, 1e-3)]
    rng = np.random.default_rng(0x7b1)
    n = 4000
    k = 10.0 ** rng.uniform(-4, 1, n)
    sweep = np.stack([rng.normal(0, 1, n) * k * 10.0 ** rng.uniform(-2, 2, n), k, rng.uniform(0, 10, n) ** 2, 10.0 ** rng.uniform(-6, 0, n)], 1)
    return np.ascontiguousarray(np.concatenate([np.array(rows, np.float64), sweep]), np.float64)


def test_robust_weight_header_under_the_sanitizers(tmp_path):
    """csrc/icp_math.h compiled into a stand-alone host program (tests/_icp_robust_math_check.cpp, its own main) with AddressSanitizer and
    UndefinedBehaviorSanitizer: robust_weight of every kind and gicp_residual over the edge table equal the oracle's, bit for bit."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'icp_robust_math_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                           '-I' + os.path.join(ROOT, 'roreg_amd', 'csrc'), os.path.join(HERE, '_icp_robust_math_check.cpp'), '-o', exe])
    table = _edge_table()
    path = str(tmp_path / 'table.f64')
    table.tofile(path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().split('\n')
    assert int(lines[-1]) == table.shape[0]
    got = np.array([[int(v, 16) for v in ln.split()] for ln in lines[:-1]], np.uint64).view(np.float64)
    want = np.stack([RO.weight(loss, table[:, 0], table[:, 1]) if loss else np.ones(table.shape[0]) for loss in (None,) + RO.LOSSES]
                    + [RO.gicp_residual(table[:, 2], table[:, 3])], 1)
    assert got.shape == want.shape and not np.isnan(got).any() and not np.isnan(want).any()
    bad = np.nonzero((got != want).any(1))[0]                      # (every value compared exactly; +0 and -0 are one value)
    assert bad.size == 0, f'{len(bad)} rows differ, the first: row {bad[0]} {table[bad[0]]} got {got[bad[0]]} want {want[bad[0]]}'
    # the table reaches what it is for: both sides of |u| = 1, exact ones, exact zeros from an infinite u^2, huber's 1 / |u| there
    u = np.abs(table[:, 0] / table[:, 1])
    assert (u == 1).sum() >= 8 and ((u > 1) & (u < 1 + 1e-15)).sum() >= 8 and ((u < 1) & (u > 1 - 1e-15)).sum() >= 8 and np.isinf(u).sum() >= 2
    assert (got[u >= 1e150][:, 2:5] == 0).all() and (got[u == 1e200][:, 1] == 1e-200).all() and (got[:, 0] == 1).all()


def test_argument_checks_of_the_python_layers():
    """icp.refine and icp.check_loss refuse an unknown loss, a missing, non-positive or non-finite scale, a scale without a loss and a loss
    with method='point' -- before anything touches the device."""
    from roreg_amd import icp
    z = np.zeros((4, 3), np.float32)
    for kw in (dict(method='plane', loss='l1', loss_scale=0.1), dict(method='plane', loss='tukey'), dict(method='plane', loss='tukey', loss_scale=0.0),
               dict(method='gicp', loss='huber', loss_scale=-1.0), dict(method='gicp', loss='gm', loss_scale=float('nan')),
               dict(method='plane', loss='cauchy', loss_scale=float('inf')), dict(method='point', loss='tukey', loss_scale=0.03),
               dict(loss='tukey', loss_scale=0.03), dict(method='plane', loss_scale=0.03)):
        with pytest.raises(ValueError):
            icp.refine(z, z, np.eye(4), max_dist=0.1, **kw)
    assert icp.check_loss('point', None, None) == {} and icp.check_loss('plane', 'tukey', 0.03) == dict(loss='tukey', scale=0.03)


def _parse(argv):
    from roreg_amd import run_distributed as RD
    parser = argparse.ArgumentParser()
    parser.add_argument('--ransac_ird', type=float, default=0.07)
    RD.add_icp_arguments(parser)
    return RD.icp_options(parser.parse_args(argv))


def test_command_line_carries_the_loss_to_the_icp_dict():
    """--icp_loss tukey --icp_loss_scale 0.03 reaches the dict run_distributed.evaluate hands to icp_many, under plane and gicp; it is refused
    under --icp_method point (the default) and without a scale; folder and label carry the loss; without the flags the dict is what it was."""
    from roreg_amd import run_distributed as RD
    icp = _parse(['--icp', '--icp_method', 'plane', '--icp_loss', 'tukey', '--icp_loss_scale', '0.03'])
    assert icp == dict(max_dist=0.07, max_iter=30, method='plane', normal_radius=None, loss='tukey', loss_scale=0.03)
    assert RD.icp_suffix(icp) == '_plane_tukey0.03'
    icp = _parse(['--icp', '--icp_method', 'gicp', '--icp_loss', 'huber', '--icp_loss_scale', '0.01', '--icp_dist', '0.1'])
    assert icp == dict(max_dist=0.1, max_iter=30, method='gicp', normal_radius=None, gicp_epsilon=1e-3, loss='huber', loss_scale=0.01)
    assert RD.icp_suffix(icp) == '_gicp_huber0.01'
    for bad in (['--icp', '--icp_method', 'point', '--icp_loss', 'tukey', '--icp_loss_scale', '0.03'], ['--icp', '--icp_loss', 'tukey', '--icp_loss_scale', '0.03'],
                ['--icp', '--icp_method', 'plane', '--icp_loss', 'tukey'], ['--icp', '--icp_method', 'plane', '--icp_loss_scale', '0.03'],
                ['--icp', '--icp_method', 'plane', '--icp_loss', 'tukey', '--icp_loss_scale', '-1']):
        with pytest.raises(ValueError):
            _parse(bad)
    with pytest.raises(SystemExit):
        _parse(['--icp', '--icp_method', 'plane', '--icp_loss', 'l1', '--icp_loss_scale', '0.03'])
    assert _parse(['--icp']) == dict(max_dist=0.07, max_iter=30) and _parse([]) is None
    assert _parse(['--icp', '--icp_method', 'gicp']) == dict(max_dist=0.07, max_iter=30, method='gicp', normal_radius=None, gicp_epsilon=1e-3)
    assert [RD.icp_suffix(d) for d in (dict(), dict(method='plane'), dict(method='gicp'))] == ['', '_plane', '_gicp']


def test_without_a_loss_the_oracle_is_the_unweighted_one():
    """loss None: the sums of PO.iterate and GO.iterate (a product by 1.0 is exact; the matrix product may associate differently) and the
    full run of PO.icp, on the 3073-point chunk pair."""
    import _icp_gicp_cases as GC
    import _icp_gicp_oracle as GO
    name, q, p, T0 = PC.chunk_pairs()[4]
    Nq, Np = PC.chunk_normals().table, PO.normals(p, PC.CHUNK_RADIUS, PC.MIN_NB).table
    Q, P = PO.widen(q), PO.widen(p)
    a, b = PO.iterate(Q, P, Nq, T0[:3, :3], T0[:3, 3], C.CHUNK_DIST), RO.iterate_plane(Q, P, Nq, T0[:3, :3], T0[:3, 3], C.CHUNK_DIST)
    assert np.array_equal(a['assign'], b['assign']) and a['n_valid'] == b['n_valid'] > 1000 and a['sum_e2'] == b['sum_e2'] and np.array_equal(a['c'], b['c'])
    assert np.abs(a['A'] - b['A']).max() <= 1e-13 * np.abs(a['A']).max() and np.abs(a['b'] - b['b']).max() <= 1e-13 * np.abs(a['b']).max()
    g, h = GO.iterate(Q, P, Nq, Np, T0[:3, :3], T0[:3, 3], C.CHUNK_DIST), RO.iterate_gicp(Q, P, Nq, Np, T0[:3, :3], T0[:3, 3], C.CHUNK_DIST)
    assert g['n'] == h['n'] and abs(g['sum_md'] - h['sum_md']) <= 1e-13 * g['sum_md']
    assert np.abs(g['A'] - h['A']).max() <= 1e-13 * np.abs(g['A']).max() and np.abs(g['b'] - h['b']).max() <= 1e-13 * np.abs(g['b']).max()
    want, got = PO.icp(q, p, Nq, T0, C.CHUNK_DIST, max_iter=C.CHUNK_ITER), RO.icp_plane(q, p, Nq, T0, C.CHUNK_DIST, max_iter=C.CHUNK_ITER)
    assert (want.iters, want.status, want.inliers) == (got.iters, got.status, got.inliers) and np.abs(want.T - got.T).max() <= 1e-12
    # and a loss changes the sums: huber's A is smaller in the positive-definite order, the count and sum e^2 are not touched
    r = RO.iterate_plane(Q, P, Nq, T0[:3, :3], T0[:3, 3], C.CHUNK_DIST, 'huber', 0.01)
    assert r['n_valid'] == b['n_valid'] and r['sum_e2'] == b['sum_e2'] and np.linalg.eigvalsh(b['A'] - r['A']).min() > 0


@pytest.mark.parametrize('method', RC.METHODS)
def test_one_iteration_family_has_residuals_on_both_sides_of_the_scale(method):
    """On the tie pair at d = 0.1 and scale 0.01, under either method, at least a tenth of the counted residuals lie on each side of the
    scale -- for every loss (the residuals do not depend on it) --, the four losses give four different A, and n_valid and sum e^2 are those of
    the run without a loss."""
    plain = RC.tie_reference(method, None)
    seen = []
    for loss in RC.LOSSES:
        it = RC.tie_reference(method, loss)
        inside, outside = RC.sides(it, RC.ONE_SCALE)
        print(f'{method} {loss}: n_valid {it["n_valid"]}, {inside * 100:.1f} % of the residuals within the scale, mean weight {it["w"].mean():.3f}')
        assert inside >= RC.ONE_SHARE and outside >= RC.ONE_SHARE
        assert it['n_valid'] == plain['n_valid'] > 5000 and it['sum_e2'] == plain['sum_e2'] and np.array_equal(it['assign'], plain['assign'])
        assert 0.1 < it['w'].mean() < 0.95 and np.linalg.eigvalsh(plain['A'] - it['A']).min() > 0
        seen.append(it['A'])
    assert all(np.abs(a - b).max() > 1e-3 * np.abs(a).max() for i, a in enumerate(seen) for b in seen[i + 1:])


@pytest.mark.parametrize('method', RC.METHODS)
def test_convergence_family_keeps_clear_of_the_tolerances(method):
    """Every loss from both starts: the oracle converges before max_iter and every step of its trace is at least 1 % away from tol_deg and
    tol_t, so that the device's verdict cannot differ by rounding."""
    for loss in RC.LOSSES:
        for start in (0, 1):
            res, trace = RC.conv_reference(method, loss, start)
            margin = RC.verdict_margin(trace)
            print(f'{method} {loss} start {start}: {res.iters} iterations, {res.status}, {res.inliers} inliers, margin {margin:.3f}')
            assert margin >= RC.MARGIN and res.status == 'converged' and 1 < res.iters < RC.CONV_ITER


def test_wall_family_keeps_clear_of_the_tolerances():
    for seed in C.WALL_SEEDS:
        res, trace = RC.wall_reference(seed)
        print(f'wall seed {seed}: {res.iters} iterations, {res.status}, margin {RC.verdict_margin(trace):.3f}')
        assert RC.verdict_margin(trace) >= RC.MARGIN and res.iters > 1


@pytest.mark.parametrize('seed', RC.OUT_SEEDS)
def test_outlier_family_a_redescending_loss_removes_the_bias(seed):
    """Plane ICP without a loss ends at least 5 mm from the truth (the raised patch, inside the gate, pulls it); with tukey at 0.03 it ends at
    no more than one tenth of that run's translation error AND rotation error."""
    q, p, Tg = RC.outlier_pair(seed)
    assert q.shape == p.shape == (RC.OUT_N, 3) and q.dtype == p.dtype == np.float32
    plain, _ = RC.outlier_reference(seed, None)
    robust, trace = RC.outlier_reference(seed, RC.OUT_LOSS)
    (deg0, t0), (deg1, t1) = O.pose_error(plain.T, Tg), O.pose_error(robust.T, Tg)
    print(f'seed {seed}: no loss {plain.iters} searches ({plain.status}), {deg0:.4f} deg / {t0 * 1e3:.2f} mm; {RC.OUT_LOSS} {RC.OUT_SCALE}: {robust.iters} searches '
          f'({robust.status}), {deg1:.4f} deg / {t1 * 1e3:.3f} mm = 1 / {deg0 / deg1:.1f} and 1 / {t0 / t1:.1f}; margin {RC.verdict_margin(trace):.2f}')
    assert t0 * 1e3 >= RC.OUT_PLAIN_MM
    assert t1 <= RC.OUT_FACTOR * t0 and deg1 <= RC.OUT_FACTOR * deg0
    assert robust.status == 'converged' and RC.verdict_margin(trace) >= RC.MARGIN
    assert robust.inliers == plain.inliers or abs(robust.inliers - plain.inliers) < 0.05 * plain.inliers          # the gate, not the loss, counts
