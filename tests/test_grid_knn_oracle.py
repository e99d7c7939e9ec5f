"""CPU checks of the grid k-nearest-neighbour search and the outlier filters: the numpy oracle against a plain double
loop, the conditions every input family of tests/_grid_knn_cases.py is there for, the C header against the ctypes table, csrc/knn_list.h in a
stand-alone host program under the sanitizers, and the argument checks that need no device."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import _grid_knn_cases as KC          # noqa: E402
import _grid_knn_oracle as KO         # noqa: E402


def _same(a, b):
    return (np.array_equal(a.idx, b.idx) and np.array_equal(a.d2.view(np.int64), b.d2.view(np.int64)) and np.array_equal(a.count, b.count)
            and np.array_equal(a.mean.view(np.int64), b.mean.view(np.int64)))


SMALL = [c for c in KC.CASES if c[0] in ('box', 'lattice', 'duplicate', 'ray') and KC.case(*c)[0].shape[0] <= 300]


@pytest.mark.parametrize('c', SMALL, ids=KC.case_id)
def test_vectorised_oracle_equals_the_double_loop(c):
    pts, r = KC.case(*c)
    for k in (1, 8, 20):
        assert _same(KC.reference(c[0], c[1], k), KO.knn_loops(pts, k, r)), (c, k)
    assert _same(KO.knn(pts, 5, np.inf), KO.knn_loops(pts, 5, np.inf))


def test_vectorised_oracle_equals_the_double_loop_on_foreign_queries():
    pts, q, _ = KC.foreign_case()
    sel = np.arange(0, q.shape[0], 9)
    rows = np.where(np.arange(sel.shape[0]) % 2 == 0, 3 * np.arange(sel.shape[0]), -1).astype(np.int32)
    assert _same(KO.knn(pts, 8, KC.FOREIGN_R, q[sel], rows), KO.knn_loops(pts, 8, KC.FOREIGN_R, q[sel], rows))
    own = KC.reference('box', KC.FOREIGN_N, 8)
    sub = KC.subset_rows(pts.shape[0])
    again = KO.knn(pts, 8, KC.FOREIGN_R, pts[sub], sub)
    assert _same(again, KO.Knn(own.idx[sub], own.d2[sub], own.count[sub], own.mean[sub]))


def test_box_family_has_short_and_long_rows():
    for n in KC.BOX_N:
        cnt = KC.reference('box', n, 32).count
        assert cnt.shape == (n,)
        if n >= 255:
            assert 20 < cnt.mean() < 40, (n, cnt.mean())
            # rows beyond k at every list length, rows short of k at 20 and 32 in every box; the emptiest ball holds 6 to 9 rows, so a list
            # of 8 that never fills occurs in the boxes of 255 and 257 points (and of 1, 2, 5, 63 and 65)
            for k in KC.KS:
                assert (cnt > k).any(), (n, k)
            assert (cnt < 20).any() and (cnt < 32).any(), (n, cnt.min())
    assert all((KC.reference('box', n, 32).count < 8).any() for n in (63, 65, 255, 257))
    assert KC.reference('box', 1, 8).count.tolist() == [0] and np.isinf(KC.reference('box', 1, 8).mean).all()


def test_lattice_family_is_decided_by_the_tie_rule():
    for base in KC.LAT_BASES:
        pts, kind, owner = KC.PC.lattice_case(base)
        ref = KC.reference('lattice', base, 32)
        thr2 = KC.LAT_R * KC.LAT_R
        cen = np.nonzero(kind == KC.PC.KIND_CENTRE)[0]
        # a centre's ball: its 6 face and 24 corner neighbours at exactly d2 == r^2 (the ones a step beyond are out), nothing else
        assert (ref.count[cen] == 30).all()
        assert (ref.d2[cen, :30] == thr2).all() and np.isinf(ref.d2[cen, 30:]).all()
        assert (np.diff(ref.idx[cen, :30].astype(np.int64), axis=1) > 0).all()              # all tied: ascending row
        got_kinds = kind[ref.idx[cen, :30]]
        assert ((got_kinds == KC.PC.KIND_FACE).sum(1) == 6).all() and ((got_kinds == KC.PC.KIND_CORNER).sum(1) == 24).all()
        # cut at k = 8 the list is the 8 lowest rows of 30 tied candidates
        assert np.array_equal(KC.reference('lattice', base, 8).idx[cen], ref.idx[cen, :8])


def test_duplicate_family_lists_the_copies_not_the_row_itself():
    pts, r = KC.case('duplicate')
    ref = KC.reference('duplicate', None, 8)
    for i, j in ((10, 200), (39, 229), (200, 10)):
        assert ref.idx[i, 0] == j and ref.d2[i, 0] == 0.0
    assert (ref.idx != np.arange(pts.shape[0])[:, None]).all()


def test_cluster_and_ray_families():
    ref = KC.reference('cluster', None, 32)
    assert (ref.count == KC.FK.CLUSTER_N - 1).all() and (ref.idx >= 0).all()
    up, down = KC.reference('ray', 'ascending', 32), KC.reference('ray', 'descending', 32)
    n = KC.RAY_N
    assert (up.count[[0, n - 1]] > 32).all() and (up.count[n // 2] > 64)
    # the same geometry: the lists of the two storage orders are each other's under row -> n - 1 - row
    assert np.array_equal(up.d2[::-1], down.d2)
    assert np.array_equal(up.idx[0, :4], [1, 2, 3, 4]) and np.array_equal(down.idx[n - 1, :4], [n - 2, n - 3, n - 4, n - 5])
    assert np.array_equal(up.idx[5, :4], [4, 6, 3, 7])                                       # exact ties on both sides: the lower row first


def test_foreign_family():
    pts, q, kind = KC.foreign_case()
    lo, hi = pts.min(0), pts.max(0)
    assert ((q[kind == 0] >= lo) & (q[kind == 0] <= hi)).all()
    out = (q[kind == 1] < lo) | (q[kind == 1] > hi)
    assert (out.sum(1) == 1).all() and out.any(0).all() and (q[kind == 1] < lo).any(0).all() and (q[kind == 1] > hi).any(0).all()
    ref = KC.foreign_reference(8)
    assert (ref.count[kind == 1] > 0).sum() > 60                                             # the ball reaches back into the box
    far = kind == 2
    assert (ref.count[far] == 0).all() and (ref.idx[far] == -1).all() and np.isinf(ref.d2[far]).all() and np.isinf(ref.mean[far]).all()


def test_terrain_family():
    ref = KC.reference('terrain', None, KC.TERRAIN_K)
    assert ref.count.shape[0] == 6054 and (ref.count > KC.TERRAIN_K).all() and np.isfinite(ref.mean).all()


@pytest.mark.parametrize('seed', KC.OUT_SEEDS)
def test_outlier_family_conditions(seed):
    """What the statistical filter is held to on the device rests on these: the far injected points go, the surface stays, no score sits at the
    threshold (so the mask comparison leaves out no row), and the escalation of neighbors.knn has rows to revisit."""
    from roreg_amd import neighbors
    pts, n = KC.outlier_cloud(seed)
    assert pts.shape[0] == n + n // 20 and pts.dtype == np.float32
    ref = KC.outlier_reference(seed)
    far = KC.outlier_far_rows(seed)
    removed_far = int((~ref.mask[far]).sum())
    surface_removed = int((~ref.mask[:n]).sum())
    rel = float(np.abs(ref.score - ref.T).min() / ref.T)
    kth = float(np.sqrt(KC.outlier_nearest(seed).d2[:, -1].max()))
    box = np.stack([pts.min(0), pts.max(0)]).astype(np.float64)
    r0 = KC.OUT_START_RADIUS if KC.OUT_START_RADIUS is not None else neighbors.start_radius(box, pts.shape[0], KC.OUT_NB)
    short = int((KC.outlier_nearest(seed).d2[:, -1] > r0 * r0).sum())
    print(f'seed {seed}: {removed_far} / {far.size} far injected points removed, {surface_removed} surface rows removed, nearest score {rel:.2e} of T away, '
          f'largest {KC.OUT_NB}th-neighbour distance {kth:.3f}, {short} rows short at the starting radius {r0:.4f}')
    assert far.size >= 200 and removed_far >= 0.95 * far.size
    assert surface_removed <= 0.01 * n
    assert rel > 1e-6
    assert short >= 50
    assert kth > 4 * r0                                                                     # several rounds of doubling


def test_header_declares_what_the_ctypes_table_binds():
    from roreg_amd import _abi
    header = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert re.search(r'#define\s+ROREG_ABI_VERSION\s+6\b', header) and _abi.ABI_VERSION == 6
    m = re.search(r'int\s+roreg_grid_knn\s*\(([^;]*)\)\s*;', re.sub(r'/\*.*?\*/', '', header, flags=re.S))
    assert m, 'roreg_grid_knn is not declared'
    args = [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')]
    assert args == ['const void *grid', 'int n', 'int k', 'double radius', 'const float *queries', 'const int32_t *self_rows', 'int m', 'int32_t *idx_out',
                    'double *d2_out', 'int32_t *count_out', 'double *mean_dist_out', 'void *stream']
    from ctypes import c_double, c_int, c_void_p
    want = [c_void_p if '*' in a else (c_double if a.startswith('double') else c_int) for a in args]
    assert _abi.PROTOTYPES['roreg_grid_knn'] == (c_int, want)
    assert 'v6q' in header and 'grid_knn.hip' in open(os.path.join(ROOT, 'roreg_amd', 'csrc', 'Makefile')).read()


def _streams():
    rng = np.random.default_rng(0x6e11)
    n = 211                                                                                 # prime: 'mix' is a permutation of the rows
    return {'random': rng.uniform(0.0, 1.0, n), 'coarse': rng.integers(0, 6, n).astype(np.float64), 'tied': np.full(n, 0.25),
            'ascending': np.arange(n, dtype=np.float64), 'descending': np.arange(n, dtype=np.float64)[::-1].copy()}


def test_knn_list_header_under_the_sanitizers(tmp_path):
    """csrc/knn_list.h compiled into a stand-alone host program (tests/_knn_list_check.cpp, its own main) with AddressSanitizer and
    UndefinedBehaviorSanitizer: random, coarse (many ties), all-tied, ascending and descending streams, rows ascending, descending and permuted,
    K in {8, 16, 32} and capacities below K, the list compared with a sorted reference after every offer."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'knn_list_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                           '-I' + os.path.join(ROOT, 'roreg_amd', 'csrc'), os.path.join(HERE, '_knn_list_check.cpp'), '-o', exe])
    for name, v in _streams().items():
        path = str(tmp_path / f'{name}.f64')
        v.tofile(path)
        for rows in ('up', 'down', 'mix'):
            p = subprocess.run([exe, path, rows], capture_output=True, text=True, timeout=120)
            assert p.returncode == 0 and p.stdout.startswith('ok '), (name, rows, p.stdout[-2000:] + p.stderr[-2000:])
            assert int(p.stdout.split()[1]) > 10000


def test_grid_knn_refuses_bad_arguments_before_any_device_call():
    import torch
    from roreg_amd import hip
    grid = types.SimpleNamespace(n=10, buf=None)                                             # never reached
    q = torch.zeros((4, 3), dtype=torch.float32)
    for kw in (dict(k=0), dict(k=33), dict(k=-1), dict(k=2.5), dict(k=True), dict(k='8'), dict(radius=0.0), dict(radius=-1.0), dict(radius=float('inf')),
               dict(radius=float('nan')), dict(radius='x'), dict(self_rows=torch.zeros(10, dtype=torch.int32)), dict(queries=q.double()),
               dict(queries=torch.zeros((4, 2), dtype=torch.float32)), dict(queries=torch.zeros(12, dtype=torch.float32)), dict(queries=np.zeros((4, 3), np.float32)),
               dict(queries=q, self_rows=torch.zeros(4, dtype=torch.int64)), dict(queries=q, self_rows=torch.zeros(5, dtype=torch.int32)),
               dict(queries=torch.tensor([[0.0, float('nan'), 0.0]])), dict(queries=torch.tensor([[0.0, float('inf'), 0.0]]))):
        args = dict(k=8, radius=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            hip.grid_knn(grid, **args)
    assert hip.GRID_KNN_MAX_K == 32


def test_outlier_arguments():
    from roreg_amd import icp, outliers
    from roreg_amd.engine import split_icp_outliers
    assert outliers.check_args(None) is None
    assert outliers.check_args(dict(kind='statistical')) == dict(kind='statistical', nb_neighbors=20, std_ratio=2.0)
    assert outliers.check_args(dict(kind='radius', radius=0.1, min_neighbors=40)) == dict(kind='radius', radius=0.1, min_neighbors=40)
    with pytest.raises(ValueError, match='limited to 32'):
        outliers.check_args(dict(kind='statistical', nb_neighbors=33))
    with pytest.raises(ValueError, match='limited to 32'):
        outliers.statistical(np.zeros((5, 3), np.float32), nb_neighbors=40)
    for bad in (dict(), dict(kind='median'), 'statistical', dict(kind='statistical', nb_neighbors=0), dict(kind='statistical', nb_neighbors=2.5),
                dict(kind='statistical', std_ratio=-1.0), dict(kind='statistical', std_ratio=float('nan')), dict(kind='statistical', radius=0.1),
                dict(kind='radius'), dict(kind='radius', radius=0.1), dict(kind='radius', radius=0.0, min_neighbors=3), dict(kind='radius', radius=0.1, min_neighbors=0),
                dict(kind='radius', radius=0.1, min_neighbors=3, nb_neighbors=4)):
        with pytest.raises(ValueError):
            outliers.check_args(bad)
        with pytest.raises(ValueError):
            icp.refine(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), np.eye(4), max_dist=0.1, outliers=bad)
    spec = dict(kind='statistical', nb_neighbors=16, std_ratio=1.0)
    assert split_icp_outliers({'max_dist': 0.1}) == ({'max_dist': 0.1}, None)
    assert split_icp_outliers({'max_dist': 0.1, 'outliers': spec}) == ({'max_dist': 0.1}, spec)
    with pytest.raises(ValueError):
        split_icp_outliers({'outliers': dict(kind='radius')})
    assert 'statistical' in outliers.describe(spec) and '16' in outliers.describe(spec)
    assert '0.1' in outliers.describe(dict(kind='radius', radius=0.1, min_neighbors=40)) and '40' in outliers.describe(dict(kind='radius', radius=0.1, min_neighbors=40))


def _parse(argv):
    from roreg_amd import run_distributed as RD
    parser = argparse.ArgumentParser()
    parser.add_argument('--ransac_ird', type=float, default=0.07)
    RD.add_icp_arguments(parser)
    return RD.icp_options(parser.parse_args(argv))


def test_command_line_carries_the_filter_and_refuses_what_it_must():
    from roreg_amd import run_distributed as RD
    icp = _parse(['--icp', '--icp_outlier_nb', '16', '--icp_outlier_std', '1.0'])
    assert icp == dict(max_dist=0.07, max_iter=30, outliers=dict(kind='statistical', nb_neighbors=16, std_ratio=1.0))
    assert RD.icp_suffix(icp) == ''                                                          # directories and labels stay
    icp = _parse(['--icp', '--icp_method', 'plane', '--icp_voxel', '0.025', '--icp_outlier_radius', '0.1', '--icp_outlier_min', '40'])
    assert icp['outliers'] == dict(kind='radius', radius=0.1, min_neighbors=40) and icp['voxel'] == 0.025 and RD.icp_suffix(icp) == '_plane'
    for bad in (['--icp_outlier_nb', '16', '--icp_outlier_std', '1.0'],                      # without --icp
                ['--icp_outlier_radius', '0.1', '--icp_outlier_min', '4'],
                ['--icp', '--icp_outlier_nb', '16', '--icp_outlier_std', '1.0', '--icp_outlier_radius', '0.1', '--icp_outlier_min', '4'],     # both kinds
                ['--icp', '--icp_outlier_nb', '16', '--icp_outlier_radius', '0.1'],
                ['--icp', '--icp_outlier_nb', '16'], ['--icp', '--icp_outlier_std', '1.0'], ['--icp', '--icp_outlier_radius', '0.1'], ['--icp', '--icp_outlier_min', '4'],
                ['--icp', '--icp_outlier_nb', '33', '--icp_outlier_std', '1.0'], ['--icp', '--icp_outlier_radius', '-0.1', '--icp_outlier_min', '4']):
        with pytest.raises(ValueError):
            _parse(bad)
    assert _parse(['--icp']) == dict(max_dist=0.07, max_iter=30) and _parse([]) is None
    src = open(os.path.join(ROOT, 'roreg_amd', 'run_distributed.py')).read()
    assert 'outlier removal                  : ' in src


def test_start_radius_is_host_arithmetic():
    from roreg_amd import neighbors
    box = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 4.0]])
    r = neighbors.start_radius(box, 1000, 16)
    assert np.isclose(4.0 / 3.0 * np.pi * r ** 3 * 1000 / 8.0, 16.0)
    assert neighbors.start_radius(np.zeros((2, 3)), 5, 3) == 1.0                             # every point the same
    flat = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]])
    assert neighbors.start_radius(flat, 100, 8) == pytest.approx(1e-3 * np.sqrt(2.0))


def test_results_log_block_names_the_filter(tmp_path):
    """run_distributed's '-icp' block: one more line names the outlier filter (as one names the voxel); without a filter the block is what it was;
    the directory and the label do not carry it."""
    from types import SimpleNamespace as NS
    from roreg_amd import distributed as D
    from roreg_amd import run_distributed as RD
    cfg = NS(output_cache_fn=f'{tmp_path}/cache', keynum=5000, ET='yohoo', max_iter=1000, base_dir=str(tmp_path), tau_1=0.05)
    ds = NS(name='synth/scene0', pair_ids=[('0', '1')], pc_ids=['0', '1'], get_transform=lambda a, b: np.eye(4))
    table = D.pack_rows(0, [NS(id0='0', id1='1', n_match=100, recalltime=5, trans=np.eye(4), ir=0.01)])
    spec = dict(kind='statistical', nb_neighbors=16, std_ratio=1.0)
    RD._write_icp(cfg, {'s': ds}, ['s'], table, 'label', '_plane', (0.025, 'centroid'), spec)
    RD._write_icp(cfg, {'s': ds}, ['s'], table, 'label', '_plane', None, dict(kind='radius', radius=0.1, min_neighbors=40))
    RD._write_icp(cfg, {'s': ds}, ['s'], table, 'label', '_plane')
    blocks = open(f'{tmp_path}/results.log').read().split('label-icp-plane\n')[1:]
    assert len(blocks) == 3
    assert blocks[0].split('\n')[:2] == ['voxel downsampling               : 0.025 (centroid)', 'outlier removal                  : statistical, 16 neighbours, std ratio 1']
    assert blocks[1].split('\n')[0] == 'outlier removal                  : radius 0.1, at least 40 neighbours'
    assert 'outlier' not in blocks[2] and blocks[2].startswith('rotation error(pointdsc)')
    assert os.listdir(f'{tmp_path}/cache/synth/scene0/match_5000') == ['yohoo_icp_plane']
