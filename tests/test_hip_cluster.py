"""The DBSCAN kernels (csrc/cluster.hip, "v6r"), roreg_amd/cluster.py and the cluster filter of roreg_amd/outliers.py on the device against
tests/_cluster_oracle.py, on the families of tests/_cluster_cases.py (tests/test_cluster_oracle.py checks the families' own conditions on the
CPU), and the layers that take outliers=dict(kind='cluster', ...).  Every comparison is exact: the outputs are integers."""
import numpy as np
import pytest
import torch

import _cluster_cases as CC
import _cluster_oracle as CO
import _fpfh_cases as FK
import _voxel_oracle as VO

pytestmark = pytest.mark.gpu


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _run(pts, eps, min_points, grid_dist):
    from roreg_amd import hip
    out = hip.grid_dbscan(hip.IcpGrid(_cuda(np.asarray(pts, np.float32).reshape(-1, 3)), grid_dist), eps, min_points)
    return tuple(v.cpu().numpy() for v in out)


def _assert_equals_oracle(got, want, what):
    labels, core, nc, sizes = got
    n = want.labels.shape[0]
    assert labels.dtype == np.int32 and core.dtype == np.uint8 and nc.dtype == np.int32 and sizes.dtype == np.int32
    assert labels.shape == (n,) and core.shape == (n,) and nc.shape == (1,) and sizes.shape == (n,)
    assert int(nc[0]) == CO.n_clusters(want), f'{what}: {int(nc[0])} clusters against {CO.n_clusters(want)}'
    bad = np.nonzero((labels != want.labels) | (core != want.core))[0]
    assert bad.size == 0, (f'{what}: {bad.size} of {n} rows differ, the first: row {bad[0]}, label {labels[bad[0]]} against {want.labels[bad[0]]}, '
                           f'core {core[bad[0]]} against {want.core[bad[0]]}')
    assert np.array_equal(sizes, want.sizes), what


@pytest.mark.parametrize('case', CC.CASES, ids=CC.case_id)
def test_labels_core_count_and_sizes_equal_the_oracle(case):
    """labels, core, n_clusters and sizes of every family, from grids built for eps, eps / 2 and 2 eps: the oracle's integers, and the same bytes
    from every grid"""
    pts, eps, min_points = CC.case(*case)
    want = CC.reference(*case)
    runs = [_run(pts, eps, min_points, d) for d in (eps, eps / 2, 2 * eps)]
    _assert_equals_oracle(runs[0], want, CC.case_id(case))
    for other in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other, runs[0]))


@pytest.mark.parametrize('min_points', CC.WIDE_MIN_POINTS)
def test_two_runs_of_wide_give_the_same_bytes(min_points):
    """many workgroups hook into the same components at once, in whatever order: the result does not show it"""
    from roreg_amd import hip
    pts, eps, _ = CC.case('wide', min_points)
    grid = hip.IcpGrid(_cuda(pts), eps)
    a = hip.grid_dbscan(grid, eps, min_points)
    b = hip.grid_dbscan(grid, eps, min_points)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(a[2].item()) == CO.n_clusters(CC.reference('wide', min_points))


def test_dbscan_of_a_host_cloud_and_of_its_voxels():
    """cluster.dbscan: a ClusterResult narrowed to the clusters; voxel=: the oracle on the voxel oracle's centroids"""
    from roreg_amd import cluster
    pts, eps, min_points = CC.case('blobs', 0)
    want = CC.reference('blobs', 0)
    res = cluster.dbscan(pts, eps, min_points)
    c = CO.n_clusters(want)
    assert res.n_clusters == c and res.labels.dtype == torch.int32 and res.core.dtype == torch.bool and tuple(res.sizes.shape) == (c,)
    assert np.array_equal(res.labels.cpu().numpy(), want.labels) and np.array_equal(res.core.cpu().numpy(), want.core.astype(bool))
    assert np.array_equal(res.sizes.cpu().numpy(), want.sizes[:c])
    big = cluster.largest(res).cpu().numpy()
    assert big.dtype == bool and np.array_equal(big, CO.cluster_mask(want, largest=True)[0])
    raw = FK.terrain_pair(1)[0]
    cen = np.ascontiguousarray(VO.downsample(raw, FK.TERRAIN_VOXEL).points, np.float32)
    for mp in (1, 6):
        want = CO.dbscan(cen, 0.08, mp)
        res = cluster.dbscan(raw, 0.08, mp, voxel=FK.TERRAIN_VOXEL)
        assert res.n_clusters == CO.n_clusters(want) and np.array_equal(res.labels.cpu().numpy(), want.labels)
        assert np.array_equal(res.core.cpu().numpy(), want.core.astype(bool)) and np.array_equal(res.sizes.cpu().numpy(), want.sizes[:res.n_clusters])


def test_largest_ties_go_to_the_lower_label_and_small_clouds():
    from roreg_amd import cluster, outliers
    pts, site, copies = CC.duplicate_case()
    res = cluster.dbscan(pts, CC.DUP_EPS, CC.DUP_MIN_POINTS)                                 # four clusters of five rows: a tie
    want = CC.reference('duplicate')
    assert int((want.sizes == want.sizes.max()).sum()) > 1
    assert np.array_equal(cluster.largest(res).cpu().numpy(), CO.cluster_mask(want, largest=True)[0])
    out = outliers.cluster(pts, CC.DUP_EPS, largest=True, min_points=CC.DUP_MIN_POINTS)
    assert np.array_equal(out.mask.cpu().numpy(), CO.cluster_mask(want, largest=True)[0])
    for name in ('none', 'empty'):
        p, eps, mp = CC.case(name)
        res = cluster.dbscan(p, eps, mp)
        assert res.n_clusters == 0 and tuple(res.sizes.shape) == (0,) and (res.labels.cpu().numpy() == -1).all() and not cluster.largest(res).cpu().numpy().any()
        for kw in (dict(min_size=1), dict(largest=True)):
            out = outliers.cluster(p, eps, min_points=mp, **kw)
            assert tuple(out.points.shape) == (0, 3) and not out.mask.cpu().numpy().any() and (out.score.cpu().numpy() == 0).all()


@pytest.mark.parametrize('seed', CC.BLOB_SEEDS)
def test_cluster_filter_mask_score_rows_and_points(seed):
    from roreg_amd import outliers
    pts, n = CC.blobs_cloud(seed)
    want = CC.reference('blobs', seed)
    for kw in (dict(min_size=CC.BLOB_MIN_SIZE), dict(min_size=41), dict(min_size=1), dict(largest=True)):
        mask, score = CO.cluster_mask(want, **kw)
        out = outliers.cluster(pts, CC.BLOB_EPS, min_points=CC.BLOB_MIN_POINTS, **kw)
        assert out.mask.dtype == torch.bool and out.score.dtype == torch.float64 and out.rows.dtype == torch.int64
        assert np.array_equal(out.mask.cpu().numpy(), mask) and np.array_equal(out.score.cpu().numpy(), score)
        assert np.array_equal(out.rows.cpu().numpy(), np.nonzero(mask)[0]) and np.array_equal(_bits(out.points), _bits(pts[mask]))
    out = outliers.cluster(pts, CC.BLOB_EPS, CC.BLOB_MIN_SIZE, CC.BLOB_MIN_POINTS)
    assert not out.mask.cpu().numpy()[n:].any() and (~out.mask.cpu().numpy()[:n]).sum() <= 0.001 * n


def _same_result(a, b):
    return (np.array_equal(_bits(np.float64(a.T)), _bits(np.float64(b.T))) and a.iters == b.iters and a.inliers == b.inliers and a.status == b.status
            and np.float64(a.rmse).tobytes() == np.float64(b.rmse).tobytes())


def test_refine_with_the_cluster_filter_equals_filtering_first():
    """icp.refine(outliers=dict(kind='cluster', ...)) on the blobs pair equals the composition done by hand: filter, then icp.refine on the kept
    points, bit for bit, alone and behind voxel=; attach_points keeps the same rows."""
    from roreg_amd import icp, outliers, voxel
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    src, n, tgt, Tg = CC.blobs_pair(0)
    spec = dict(kind='cluster', eps=CC.BLOB_EPS, min_points=CC.BLOB_MIN_POINTS, min_size=CC.BLOB_MIN_SIZE)
    f0 = outliers.cluster(src, CC.BLOB_EPS, CC.BLOB_MIN_SIZE, CC.BLOB_MIN_POINTS)
    f1 = outliers.cluster(tgt, CC.BLOB_EPS, CC.BLOB_MIN_SIZE, CC.BLOB_MIN_POINTS)
    want = CO.cluster_mask(CC.reference('blobs', 0), CC.BLOB_MIN_SIZE)[0]
    assert np.array_equal(f0.mask.cpu().numpy(), want) and 0 < int(f0.points.shape[0]) <= n
    for method in ('point', 'plane'):
        kw = dict(max_dist=0.5, max_iter=8, method=method, normal_radius=0.15)
        a = icp.refine(src, tgt, Tg, outliers=spec, **kw)
        b = icp.refine(f0.points, f1.points, Tg, **kw)
        assert _same_result(a, b) and a.inliers > 1000
    big = dict(kind='cluster', eps=CC.BLOB_EPS, min_points=CC.BLOB_MIN_POINTS, largest=True)
    g0, g1 = (outliers.cluster(p, CC.BLOB_EPS, largest=True, min_points=CC.BLOB_MIN_POINTS) for p in (src, tgt))
    assert _same_result(icp.refine(src, tgt, Tg, max_dist=0.1, max_iter=8, outliers=big), icp.refine(g0.points, g1.points, Tg, max_dist=0.1, max_iter=8))
    v = 0.1
    w0, w1 = voxel.downsample(src, v), voxel.downsample(tgt, v)
    vspec = dict(kind='cluster', eps=0.16, min_size=50)
    h0, h1 = outliers.cluster(w0.points, 0.16, 50), outliers.cluster(w1.points, 0.16, 50)
    assert 0 < int(h0.points.shape[0]) < w0.points.shape[0]
    assert _same_result(icp.refine(src, tgt, Tg, max_dist=0.2, max_iter=8, voxel=v, outliers=vspec), icp.refine(h0.points, h1.points, Tg, max_dist=0.2, max_iter=8))
    both = outliers.cluster(src, 0.16, 50, voxel=v)
    assert torch.equal(both.points, h0.points) and np.array_equal(both.rows.cpu().numpy(), w0.first[h0.rows.cpu().numpy()])
    eng = RegistrationEngine(default_config(), None, None)
    c = eng.attach_points(CloudState(before=None), src, outliers=spec)
    assert c.points_rows.dtype == torch.int64 and np.array_equal(c.points_rows.cpu().numpy(), np.nonzero(want)[0]) and np.array_equal(_bits(c.points), _bits(src[want]))
    c = eng.attach_points(CloudState(before=None), src, voxel=v, outliers=vspec)
    assert np.array_equal(c.points_rows.cpu().numpy(), w0.first[h0.rows.cpu().numpy()]) and torch.equal(c.points, h0.points)


def test_bad_arguments_raise_before_any_launch():
    from roreg_amd import cluster, hip, outliers
    pts = CC.box_case(65)
    grid = hip.IcpGrid(_cuda(pts), 0.1)
    for eps, mp in ((0.0, 1), (-0.1, 1), (float('nan'), 1), (float('inf'), 1), ('0.1', 1), (0.1, 0), (0.1, -2), (0.1, 2.5), (0.1, True), (0.1, None)):
        with pytest.raises(ValueError):
            hip.grid_dbscan(grid, eps, mp)
        with pytest.raises(ValueError):
            cluster.dbscan(pts, eps, mp)
        with pytest.raises(ValueError):
            outliers.cluster(pts, eps, min_size=3, min_points=mp)
    with pytest.raises(ValueError):
        hip.grid_dbscan(None, 0.1, 1)
    with pytest.raises(ValueError):
        outliers.cluster(pts, 0.1)
    with pytest.raises(ValueError):
        outliers.cluster(pts, 0.1, min_size=3, largest=True)
    with pytest.raises(hip.HipError):
        cluster.device_dbscan(torch.from_numpy(pts), 0.1, 1)                                 # a host tensor: no fall-back
