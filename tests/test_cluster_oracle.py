"""The DBSCAN oracle (tests/_cluster_oracle.py) against itself and the input families of tests/_cluster_cases.py against the conditions that name
them, on the CPU; the argument checks of the cluster filter and its command line.  tests/test_hip_cluster.py runs the same families on the device."""
import argparse
import os
import types

import numpy as np
import pytest

import _cluster_cases as CC
import _cluster_oracle as CO
import _grid_knn_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('case', CC.SMALL_CASES, ids=CC.case_id)
def test_the_two_oracle_forms_agree(case):
    pts, eps, min_points = CC.case(*case)
    a, b = CC.reference(*case), CO.dbscan_loops(pts, eps, min_points)
    assert a.labels.dtype == np.int32 and a.core.dtype == np.uint8 and a.sizes.dtype == np.int32 and a.sizes.shape == a.labels.shape
    assert np.array_equal(a.labels, b.labels) and np.array_equal(a.core, b.core) and np.array_equal(a.sizes, b.sizes) and a.n_border == b.n_border
    c = CO.n_clusters(a)
    assert int(a.sizes.sum()) == int((a.labels >= 0).sum()) and (a.sizes[c:] == 0).all() and (a.sizes[:c] > 0).all()
    lowest = [int(np.nonzero((a.labels == k) & (a.core == 1))[0][0]) for k in range(c)]      # numbered by ascending lowest core row
    assert lowest == sorted(lowest)


def test_box_family_has_clusters_noise_and_border_rows():
    for n in CC.BOX_N:
        one, four = CC.reference('box', (n, 1)), CC.reference('box', (n, 4))
        assert one.core.all() and one.n_border == 0 and (one.labels >= 0).all()              # min_points 1: connected components
        if n >= 63:
            assert CO.n_clusters(one) > 1 and four.n_border > 0 and (four.labels < 0).any() and CO.n_clusters(four) >= 1
    assert CO.n_clusters(CC.reference('box', (1025, 4))) > 1
    ball = np.bincount(CO.pairs(CO.widen(CC.box_case(1025)), CC.box_eps(1025))[0]).mean()
    assert 3.0 < ball < 5.5, ball


@pytest.mark.parametrize('order', CC.CHAIN_ORDERS)
def test_chain_family(order):
    """one component of 4,097 rows whose links are all at exactly d2 == eps^2; the widened link cuts it in two; min_points 3 leaves the ends as
    border rows"""
    line = CC.chain_line().astype(np.float64)
    assert (CO._d2(line[:-1], line[1:]) == CC.CHAIN_EPS ** 2).all()
    rows = CC.chain_rows(order)
    assert np.array_equal(CC.chain_case(order)[rows], CC.chain_line())
    full = CC.reference('chain', order)
    assert CO.n_clusters(full) == 1 and full.sizes[0] == CC.CHAIN_N and full.core.all()
    gline = CC.chain_line(True).astype(np.float64)
    link = CO._d2(gline[:-1], gline[1:])
    assert link[CC.CHAIN_GAP] == float(CC.CHAIN_WIDE) ** 2 > CC.CHAIN_EPS ** 2 and (np.delete(link, CC.CHAIN_GAP) == CC.CHAIN_EPS ** 2).all()
    gap = CC.reference('chain_gap', order)
    assert CO.n_clusters(gap) == 2 and sorted(gap.sizes[:2]) == sorted((CC.CHAIN_GAP + 1, CC.CHAIN_N - CC.CHAIN_GAP - 1))
    assert len(set(gap.labels[rows[:CC.CHAIN_GAP + 1]])) == 1 and len(set(gap.labels[rows[CC.CHAIN_GAP + 1:]])) == 1
    ends = CC.reference('chain_ends', order)
    assert CO.n_clusters(ends) == 1 and ends.sizes[0] == CC.CHAIN_N and ends.n_border == 2
    assert np.array_equal(np.sort(np.nonzero(ends.core == 0)[0]), np.sort(rows[[0, -1]]))
    if order == 'descending':                                    # the root is the far end of the line
        assert rows[-1] == 0


@pytest.mark.parametrize('base', CC.LAT_BASES)
def test_lattice_family(base):
    """at 31 only the centres are core (themselves, 6 face and 24 corner neighbours at exactly r): 27 clusters of 31, the rows one step beyond
    are noise"""
    import _icp_plane_cases as PC
    pts, kind, owner = PC.lattice_case(base)[:3]
    kind, owner = np.asarray(kind), np.asarray(owner)
    res = CC.reference('lattice', (base, 31))
    assert CO.n_clusters(res) == 27 and (res.sizes[:27] == 31).all()
    assert np.array_equal(np.nonzero(res.core)[0], np.nonzero(kind == PC.KIND_CENTRE)[0])
    at_r = (kind == PC.KIND_FACE) | (kind == PC.KIND_CORNER)
    assert np.array_equal(res.labels[at_r], res.labels[owner[at_r]]) and (res.labels[(kind == PC.KIND_FACE_BEYOND) | (kind == PC.KIND_CORNER_BEYOND)] == -1).all()
    assert CO.n_clusters(CC.reference('lattice', (base, 1))) == 27


def test_duplicate_family():
    pts, site, copies = CC.duplicate_case()
    res = CC.reference('duplicate')
    dense = copies[site] >= CC.DUP_MIN_POINTS
    assert np.array_equal(res.core.astype(bool), dense) and np.array_equal(res.labels >= 0, dense) and res.n_border == 0
    assert CO.n_clusters(res) == int((copies >= CC.DUP_MIN_POINTS).sum())
    for s in range(CC.DUP_SITES):
        lab = set(res.labels[site == s])
        assert len(lab) == 1 and (lab == {-1} or res.sizes[lab.pop()] == copies[s])


def test_bridge_family():
    pts = CC.bridge_case().astype(np.float64)
    res = CC.reference('bridge')
    lab = res.labels
    assert CO.n_clusters(res) == 4 and res.n_border == 2 and res.core[CC.BRIDGE_NEAR] == 0 and res.core[CC.BRIDGE_TIE] == 0
    groups = [lab[list(g)] for g in (CC.BRIDGE_A, CC.BRIDGE_B, CC.BRIDGE_C, CC.BRIDGE_D)]
    assert all(len(set(g)) == 1 for g in groups) and [int(g[0]) for g in groups] == [0, 1, 2, 3]
    near = CO._d2(pts[CC.BRIDGE_NEAR], pts[[CC.BRIDGE_A_CORE, CC.BRIDGE_B_CORE]])
    assert near[0] == CC.BRIDGE_EPS ** 2 and near[1] < near[0] and CC.BRIDGE_A_CORE < CC.BRIDGE_B_CORE
    assert lab[CC.BRIDGE_NEAR] == lab[CC.BRIDGE_B_CORE]                                      # the nearer core, not the lower row
    tie = CO._d2(pts[CC.BRIDGE_TIE], pts[[CC.BRIDGE_C_CORE, CC.BRIDGE_D_CORE]])
    assert tie[0] == tie[1] == CC.BRIDGE_EPS ** 2 and CC.BRIDGE_D_CORE < CC.BRIDGE_C_CORE
    assert lab[CC.BRIDGE_TIE] == lab[CC.BRIDGE_D_CORE] == 3                                  # the lower ROW, not the lower cluster number
    assert np.array_equal(res.sizes[:4], [4, 5, 4, 5])


def test_none_and_empty():
    res = CC.reference('none')
    assert CO.n_clusters(res) == 0 and (res.labels == -1).all() and not res.core.any() and not res.sizes.any() and res.sizes.shape == (CC.NONE_N,)
    res = CC.reference('empty')
    assert CO.n_clusters(res) == 0 and res.labels.shape == (0,) and res.core.shape == (0,) and res.sizes.shape == (0,)


@pytest.mark.parametrize('min_points', CC.WIDE_MIN_POINTS)
def test_wide_family(min_points):
    res = CC.reference('wide', min_points)
    assert res.labels.shape == (40000,) and res.sizes[0] > 30000 and CO.n_clusters(res) > 1
    if min_points > 1:
        assert res.n_border > 100 and (res.labels < 0).any()


@pytest.mark.parametrize('seed', CC.BLOB_SEEDS)
def test_blobs_pass_the_statistical_filter_and_fall_to_the_cluster_filter(seed):
    pts, n = CC.blobs_cloud(seed)
    blob = np.arange(pts.shape[0]) >= n
    assert int(blob.sum()) == CC.BLOB_COUNT * CC.BLOB_POINTS == 320
    stat = KO.statistical(pts, CC.BLOB_STAT_NB, CC.BLOB_STAT_STD).mask
    mask, score = CO.cluster_mask(CC.reference('blobs', seed), CC.BLOB_MIN_SIZE)
    print(f'seed {seed}: n {n}, statistical keeps {int(stat[blob].sum())} of 320 blob rows and removes {int((~stat[~blob]).sum())} surface rows; '
          f'cluster keeps {int(mask[blob].sum())} blob rows and removes {int((~mask[~blob]).sum())} surface rows')
    assert stat[blob].sum() >= 0.95 * 320
    assert mask[blob].sum() == 0 and (~mask[~blob]).sum() <= 0.001 * n
    assert (score[mask] >= CC.BLOB_MIN_SIZE).all() and (score[blob] < CC.BLOB_MIN_SIZE).all()
    big, _ = CO.cluster_mask(CC.reference('blobs', seed), largest=True)
    assert big[blob].sum() == 0 and big.sum() == CC.reference('blobs', seed).sizes.max()


def test_cluster_mask_ties_go_to_the_lower_label():
    res = CO.Clusters(np.int32([1, 0, -1, 1, 0, 2]), np.uint8([1, 1, 0, 1, 1, 1]), np.int32([2, 2, 1, 0, 0, 0]), 0)
    mask, score = CO.cluster_mask(res, largest=True)
    assert np.array_equal(mask, [False, True, False, False, True, False]) and np.array_equal(score, [2, 2, 0, 2, 2, 1])
    assert np.array_equal(CO.cluster_mask(res, min_size=2)[0], [True, True, False, True, True, False])


def test_grid_dbscan_refuses_bad_arguments_before_any_device_call():
    from roreg_amd import cluster, hip
    grid = types.SimpleNamespace(n=10, buf=None)                                             # never reached
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float('inf')), dict(eps=float('nan')), dict(eps='x'), dict(eps=None), dict(eps=True),
               dict(min_points=0), dict(min_points=-1), dict(min_points=2.5), dict(min_points=True), dict(min_points='3'), dict(min_points=None),
               dict(min_points=2 ** 31), dict(grid=None), dict(grid=np.zeros((4, 3), np.float32))):
        args = dict(grid=grid, eps=0.1, min_points=3)
        args.update(kw)
        with pytest.raises(ValueError):
            hip.grid_dbscan(**args)
        if 'grid' not in kw:
            with pytest.raises(ValueError):
                cluster.dbscan(np.zeros((5, 3), np.float32), args['eps'], args['min_points'])
            with pytest.raises(ValueError):
                cluster.device_dbscan(None, args['eps'], args['min_points'])


def test_cluster_outlier_arguments():
    from roreg_amd import icp, outliers
    from roreg_amd.engine import split_icp_outliers
    assert outliers.KINDS == ('statistical', 'radius', 'cluster')
    spec = dict(kind='cluster', eps=0.08, min_points=6, min_size=100)
    assert outliers.check_args(spec) == dict(kind='cluster', eps=0.08, min_points=6, min_size=100, largest=False)
    assert outliers.check_args(dict(kind='cluster', eps=1, largest=True)) == dict(kind='cluster', eps=1.0, min_points=1, min_size=None, largest=True)
    assert outliers.check_args(outliers.check_args(spec)) == outliers.check_args(spec)       # a normalised dict is a valid one
    for bad in (dict(kind='cluster'), dict(kind='cluster', min_size=100),                    # a missing eps
                dict(kind='cluster', eps=0.08), dict(kind='cluster', eps=0.08, min_size=100, largest=True),     # neither / both of min_size and largest
                dict(kind='cluster', eps=0.08, largest=False), dict(kind='cluster', eps=0.08, min_size=None), dict(kind='cluster', eps=0.08, min_size=100, largest=1),
                dict(kind='cluster', eps=0.0, min_size=100), dict(kind='cluster', eps=-0.1, min_size=100), dict(kind='cluster', eps=float('nan'), min_size=100),
                dict(kind='cluster', eps=float('inf'), min_size=100), dict(kind='cluster', eps='0.1', min_size=100),
                dict(kind='cluster', eps=0.08, min_size=0), dict(kind='cluster', eps=0.08, min_size=-3), dict(kind='cluster', eps=0.08, min_size=2.5),
                dict(kind='cluster', eps=0.08, min_size=True), dict(kind='cluster', eps=0.08, min_size=100, min_points=0),
                dict(kind='cluster', eps=0.08, min_size=100, min_points=1.5), dict(kind='cluster', eps=0.08, min_size=100, min_points=None),
                dict(kind='cluster', eps=0.08, min_size=100, radius=0.1), dict(kind='cluster', eps=0.08, min_size=100, nb_neighbors=4),       # foreign keys
                dict(kind='radius', radius=0.1, min_neighbors=3, eps=0.1), dict(kind='statistical', min_size=100)):
        with pytest.raises(ValueError):
            outliers.check_args(bad)
        with pytest.raises(ValueError):
            icp.refine(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), np.eye(4), max_dist=0.1, outliers=bad)
    for kw in (dict(), dict(min_size=100, largest=True), dict(min_size=0), dict(min_size=100, min_points=0)):
        with pytest.raises(ValueError):
            outliers.cluster(np.zeros((5, 3), np.float32), 0.08, **kw)
    assert split_icp_outliers({'max_dist': 0.1, 'outliers': spec}) == ({'max_dist': 0.1}, outliers.check_args(spec))
    assert outliers.describe(spec) == 'cluster eps 0.08, min points 6, clusters of at least 100 points'
    assert outliers.describe(dict(kind='cluster', eps=0.1, largest=True)) == 'cluster eps 0.1, min points 1, the largest cluster'


def _parse(argv):
    from roreg_amd import run_distributed as RD
    parser = argparse.ArgumentParser()
    parser.add_argument('--ransac_ird', type=float, default=0.07)
    RD.add_icp_arguments(parser)
    return RD.icp_options(parser.parse_args(argv))


def test_command_line_carries_the_cluster_filter_and_refuses_what_it_must():
    from roreg_amd import run_distributed as RD
    icp = _parse(['--icp', '--icp_outlier_cluster_eps', '0.08', '--icp_outlier_cluster_min_size', '100'])
    assert icp == dict(max_dist=0.07, max_iter=30, outliers=dict(kind='cluster', eps=0.08, min_points=1, min_size=100, largest=False))
    assert RD.icp_suffix(icp) == ''                                                          # directories and labels stay
    icp = _parse(['--icp', '--icp_method', 'plane', '--icp_voxel', '0.025', '--icp_outlier_cluster_eps', '0.08', '--icp_outlier_cluster_min_size', '100',
                  '--icp_outlier_cluster_min_points', '6'])
    assert icp['outliers'] == dict(kind='cluster', eps=0.08, min_points=6, min_size=100, largest=False) and icp['voxel'] == 0.025 and RD.icp_suffix(icp) == '_plane'
    c = ['--icp_outlier_cluster_eps', '0.08', '--icp_outlier_cluster_min_size', '100']
    for bad in (c, c + ['--icp_outlier_cluster_min_points', '6'], ['--icp_outlier_cluster_min_points', '6'],                  # without --icp
                ['--icp'] + c + ['--icp_outlier_nb', '16', '--icp_outlier_std', '1.0'], ['--icp'] + c + ['--icp_outlier_radius', '0.1', '--icp_outlier_min', '4'],     # two filters
                ['--icp'] + c + ['--icp_outlier_nb', '16'], ['--icp', '--icp_outlier_cluster_min_points', '6', '--icp_outlier_radius', '0.1', '--icp_outlier_min', '4'],
                ['--icp', '--icp_outlier_cluster_eps', '0.08'], ['--icp', '--icp_outlier_cluster_min_size', '100'], ['--icp', '--icp_outlier_cluster_min_points', '6'],
                ['--icp', '--icp_outlier_cluster_eps', '0.08', '--icp_outlier_cluster_min_points', '6'],
                ['--icp', '--icp_outlier_cluster_eps', '-0.08', '--icp_outlier_cluster_min_size', '100'],
                ['--icp', '--icp_outlier_cluster_eps', '0.08', '--icp_outlier_cluster_min_size', '0'],
                ['--icp'] + c + ['--icp_outlier_cluster_min_points', '0']):
        with pytest.raises(ValueError):
            _parse(bad)
    assert _parse(['--icp']) == dict(max_dist=0.07, max_iter=30) and _parse([]) is None


def test_results_log_block_names_the_cluster_filter(tmp_path):
    from types import SimpleNamespace as NS
    from roreg_amd import distributed as D
    from roreg_amd import run_distributed as RD
    cfg = NS(output_cache_fn=f'{tmp_path}/cache', keynum=5000, ET='yohoo', max_iter=1000, base_dir=str(tmp_path), tau_1=0.05)
    ds = NS(name='synth/scene0', pair_ids=[('0', '1')], pc_ids=['0', '1'], get_transform=lambda a, b: np.eye(4))
    table = D.pack_rows(0, [NS(id0='0', id1='1', n_match=100, recalltime=5, trans=np.eye(4), ir=0.01)])
    RD._write_icp(cfg, {'s': ds}, ['s'], table, 'label', '', None, dict(kind='cluster', eps=0.08, min_points=6, min_size=100))
    block = open(f'{tmp_path}/results.log').read().split('label-icp\n')[1]
    assert block.split('\n')[0] == 'outlier removal                  : cluster eps 0.08, min points 6, clusters of at least 100 points'
