"""The grid k-nearest-neighbour kernel (csrc/grid_knn.hip, "v6q"), roreg_amd/neighbors.py and roreg_amd/outliers.py on the device against
tests/_grid_knn_oracle.py, on the families of tests/_grid_knn_cases.py (tests/test_grid_knn_oracle.py checks the families' own conditions on the
CPU), and the layers that take outliers=.  Every comparison is exact: integers as they are, floats as their bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

import _grid_knn_cases as KC
import _grid_knn_oracle as KO
import _icp_cases as C
import _icp_plane_cases as PC

pytestmark = pytest.mark.gpu


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _grid(p, d):
    from roreg_amd import hip
    return hip.IcpGrid(_cuda(np.asarray(p, np.float32).reshape(-1, 3)), d)


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.int64) if a.dtype == np.float64 else (a.view(np.int32) if a.dtype == np.float32 else a)


def _host(res):
    return KO.Knn(*(v.cpu().numpy() for v in res))


def _assert_same(got, want, what):
    assert got.idx.dtype == np.int32 and got.d2.dtype == np.float64 and got.count.dtype == np.int32 and got.mean.dtype == np.float64
    assert got.idx.shape == want.idx.shape and got.d2.shape == want.d2.shape
    bad = np.nonzero((got.idx != want.idx).any(1) | (_bits(got.d2) != _bits(want.d2)).any(1) | (got.count != want.count) | (_bits(got.mean) != _bits(want.mean)))[0]
    assert bad.size == 0, (f'{what}: {bad.size} of {want.count.shape[0]} rows differ, the first: row {bad[0]}, count {got.count[bad[0]]} against '
                           f'{want.count[bad[0]]}, idx {got.idx[bad[0]]} against {want.idx[bad[0]]}')


@pytest.mark.parametrize('case', KC.CASES, ids=KC.case_id)
def test_own_cloud_lists_equal_the_oracle_bits(case):
    """idx, d2, count and mean_dist of every row at every list length; the lattice from grids built for r, 2 r and r / 2, and everywhere a
    second run on a grid of its own: the same bytes."""
    from roreg_amd import hip
    pts, r = KC.case(*case)
    dists = tuple(d * r / PC.LAT_R for d in PC.LAT_GRID_DISTS) if case[0] == 'lattice' else (r,)
    grids = [_grid(pts, d) for d in dists + dists[:1]]
    for k in KC.case_ks(case):
        want = KC.reference(case[0], case[1], k)
        runs = [_host(hip.grid_knn(g, k, r, want_mean=True)) for g in grids]
        _assert_same(runs[0], want, f'k = {k}')
        for other in runs[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(other, runs[0]))
        three = hip.grid_knn(grids[0], k, r)
        assert len(three) == 3 and all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(three, runs[0][:3]))


@pytest.mark.parametrize('k', KC.KS)
def test_foreign_queries_and_own_rows_through_self_rows(k):
    """Queries inside the cloud, outside the grid's box on every side and far away (count 0, -1, +inf, mean +inf); nothing excluded with
    self_rows None or -1; a subset of the own rows through queries / self_rows equals those rows of the own-cloud call bit for bit."""
    from roreg_amd import hip
    pts, q, kind = KC.foreign_case()
    want = KC.foreign_reference(k)
    for d in (KC.FOREIGN_R, 3 * KC.FOREIGN_R):
        g = _grid(pts, d)
        got = _host(hip.grid_knn(g, k, KC.FOREIGN_R, queries=_cuda(q), want_mean=True))
        _assert_same(got, want, f'foreign, grid for {d}')
        minus = _host(hip.grid_knn(g, k, KC.FOREIGN_R, queries=_cuda(q), self_rows=torch.full((q.shape[0],), -1, dtype=torch.int32).cuda(), want_mean=True))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(minus, got))
    far = kind == 2
    assert (got.count[far] == 0).all() and (got.idx[far] == -1).all() and np.isposinf(got.d2[far]).all() and np.isposinf(got.mean[far]).all()
    own = _host(hip.grid_knn(g, k, KC.FOREIGN_R, want_mean=True))
    _assert_same(own, KC.reference('box', KC.FOREIGN_N, k), 'own cloud')
    sub = KC.subset_rows(pts.shape[0])
    again = _host(hip.grid_knn(g, k, KC.FOREIGN_R, queries=_cuda(pts[sub]), self_rows=_cuda(sub, np.int32), want_mean=True))
    assert all(a.tobytes() == np.ascontiguousarray(b[sub]).tobytes() for a, b in zip(again, own))
    # a wrong excluded row changes the answer (the row is excluded by its number, not by its distance)
    shifted = _host(hip.grid_knn(g, k, KC.FOREIGN_R, queries=_cuda(pts[sub]), self_rows=_cuda((sub + 1) % pts.shape[0], np.int32), want_mean=True))
    assert (shifted.idx[:, 0] == sub).all() and (shifted.d2[:, 0] == 0.0).all()


def test_device_refuses_what_the_host_checks_let_through():
    from roreg_amd import hip
    pts, r = KC.case('box', 65)
    g = _grid(pts, r)
    with pytest.raises(ValueError):
        hip.grid_knn(g, 8, r, queries=_cuda(np.float32([[0.0, np.nan, 0.0]])))
    with pytest.raises(hip.HipError):
        hip.grid_knn(g, 8, r, queries=torch.zeros((2, 3), dtype=torch.float32))              # a host tensor: no fall-back
    empty = hip.grid_knn(g, 8, r, queries=torch.zeros((0, 3), dtype=torch.float32).cuda(), want_mean=True)
    assert [tuple(v.shape) for v in empty] == [(0, 8), (0, 8), (0,), (0,)]


@pytest.mark.parametrize('seed', KC.OUT_SEEDS)
def test_exact_nearest_neighbours_and_the_statistical_filter(seed):
    """neighbors.knn(radius=None) equals the brute-force k nearest exactly, from its own starting radius (several rounds: the injected points'
    16th neighbour is up to a metre away) and from another; outliers.statistical: the score bit for bit, T within 1e-12 relative of numpy's,
    the mask on EVERY row (tests/test_grid_knn_oracle.py: no score within 1e-6 relative of T), points and rows consistent with the mask."""
    from roreg_amd import neighbors, outliers
    pts, n = KC.outlier_cloud(seed)
    near, ref = KC.outlier_nearest(seed), KC.outlier_reference(seed)
    info = {}
    res = neighbors.knn(pts, KC.OUT_NB, start_radius=KC.OUT_START_RADIUS, info=info)
    assert info['rounds'] >= 3, info
    for got, what in ((res, 'own start'), (neighbors.knn(pts, KC.OUT_NB, start_radius=0.37), 'start 0.37'), (neighbors.knn(pts, KC.OUT_NB, start_radius=50.0), 'start 50')):
        assert np.array_equal(got.idx.cpu().numpy(), near.idx) and np.array_equal(_bits(got.d2), _bits(near.d2)), what
        assert (got.count.cpu().numpy() == KC.OUT_NB).all()
    out = outliers.statistical(pts, nb_neighbors=KC.OUT_NB, std_ratio=KC.OUT_STD)
    assert out.score.dtype == torch.float64 and np.array_equal(_bits(out.score), _bits(ref.score))
    T = float(outliers.statistical_threshold(out.score, KC.OUT_STD))
    print(f'seed {seed}: {info["rounds"]} rounds at radii {[round(r, 4) for r in info["radii"]]}, T {T!r} against {ref.T!r}')
    assert abs(T - ref.T) <= 1e-12 * ref.T
    mask = out.mask.cpu().numpy()
    assert mask.dtype == bool and np.array_equal(mask, ref.mask)
    rows = out.rows.cpu().numpy()
    assert rows.dtype == np.int64 and np.array_equal(rows, np.nonzero(ref.mask)[0]) and np.array_equal(_bits(out.points), _bits(pts[ref.mask]))
    far = KC.outlier_far_rows(seed)
    assert (~mask[far]).sum() >= 0.95 * far.size and (~mask[:n]).sum() <= 0.01 * n


def test_exact_nearest_neighbours_of_small_and_foreign_inputs():
    """min(k, n - 1) neighbours in the cloud's own mode, min(k, n) for foreign queries (however far away they are), duplicates and all."""
    from roreg_amd import neighbors
    for n in (1, 2, 5, 65):
        pts = KC.case('box', n)[0]
        want = KO.knn(pts, 8, np.inf)
        got = neighbors.knn(pts, 8)
        assert np.array_equal(got.idx.cpu().numpy(), want.idx) and np.array_equal(_bits(got.d2), _bits(want.d2))
        assert (got.count.cpu().numpy() == min(8, n - 1)).all()
    same = np.tile(np.float32([[0.3, -1.2, 0.8]]), (40, 1))
    got, want = neighbors.knn(same, 8), KO.knn(same, 8, np.inf)
    assert np.array_equal(got.idx.cpu().numpy(), want.idx) and (got.d2.cpu().numpy() == 0.0).all()
    pts, q, kind = KC.foreign_case()
    want = KO.knn(pts, 20, np.inf, q)
    got = neighbors.knn(pts, 20, queries=q)
    assert np.array_equal(got.idx.cpu().numpy(), want.idx) and np.array_equal(_bits(got.d2), _bits(want.d2)) and (got.idx.cpu().numpy() >= 0).all()
    ball = neighbors.knn(pts, 20, radius=KC.FOREIGN_R)
    ref = KC.reference('box', KC.FOREIGN_N, 20)
    assert np.array_equal(ball.idx.cpu().numpy(), ref.idx) and np.array_equal(ball.count.cpu().numpy(), ref.count) and np.array_equal(_bits(ball.d2), _bits(ref.d2))


@pytest.mark.parametrize('name,arg', [('box', 257), ('box', 1025), ('terrain', None)])
def test_radius_filter_mask_is_exact(name, arg):
    """Keep iff at least min_neighbors other rows in the ball: thresholds below, at and far above the list length of the kernel."""
    from roreg_amd import outliers
    pts, r = KC.case(name, arg)
    count = KC.reference(name, arg, 1).count
    for mn in (1, 8, 33, int(np.median(count)), int(count.max()), int(count.max()) + 1):
        out = outliers.radius(pts, r, mn)
        want = count >= mn
        assert np.array_equal(out.mask.cpu().numpy(), want) and np.array_equal(out.score.cpu().numpy(), count.astype(np.float64))
        assert np.array_equal(out.rows.cpu().numpy(), np.nonzero(want)[0]) and np.array_equal(_bits(out.points), _bits(pts[want]))
    assert int(np.median(count)) > 20 and int(count.max()) > 32


def test_empty_and_one_point_clouds():
    from roreg_amd import neighbors, outliers
    for n in (0, 1):
        pts = np.zeros((n, 3), np.float32) + 0.5
        s = outliers.statistical(pts)
        assert tuple(s.points.shape) == (n, 3) and s.mask.cpu().numpy().all() and np.array_equal(s.rows.cpu().numpy(), np.arange(n)) and np.isposinf(s.score.cpu().numpy()).all()
        r = outliers.radius(pts, 0.1, 1)
        assert tuple(r.points.shape) == (0, 3) and not r.mask.cpu().numpy().any() and (r.score.cpu().numpy() == 0).all()
        res = neighbors.knn(pts, 4)
        assert tuple(res.idx.shape) == (n, 4) and (res.idx.cpu().numpy() == -1).all() and (res.count.cpu().numpy() == 0).all()
        assert tuple(neighbors.knn(pts, 4, radius=0.1).idx.shape) == (n, 4)


def _same_result(a, b):
    return (np.array_equal(_bits(np.float64(a.T)), _bits(np.float64(b.T))) and a.iters == b.iters and a.inliers == b.inliers and a.status == b.status
            and np.float64(a.rmse).tobytes() == np.float64(b.rmse).tobytes())


def test_refine_and_describe_with_outliers_equal_filtering_first():
    """icp.refine(outliers=) and fpfh.describe(outliers=) equal the same calls on the clouds filtered beforehand, bit for bit, alone and behind
    voxel=; estimate_normals returns the kept points' original rows."""
    from roreg_amd import fpfh, icp, outliers, synth, voxel
    spec = dict(kind='statistical', nb_neighbors=KC.OUT_NB, std_ratio=KC.OUT_STD)
    p0, n0 = KC.outlier_cloud(0)
    Tg = synth.dense_gt(3.0, (0.2, -0.4, 1.0), (0.02, -0.01, 0.015)).astype(np.float64)
    p1 = ((p0[::2].astype(np.float64) - Tg[:3, 3]) @ Tg[:3, :3]).astype(np.float32)
    f0, f1 = (outliers.statistical(p, **{k: v for k, v in spec.items() if k != 'kind'}) for p in (p0, p1))
    assert 0 < int(f0.points.shape[0]) < p0.shape[0]
    for method in ('point', 'plane'):
        a = icp.refine(p0, p1, np.eye(4), max_dist=0.1, max_iter=8, method=method, outliers=spec)
        b = icp.refine(f0.points, f1.points, np.eye(4), max_dist=0.1, max_iter=8, method=method)
        plain = icp.refine(p0, p1, np.eye(4), max_dist=0.1, max_iter=8, method=method)
        assert _same_result(a, b) and a.iters > 1 and not _same_result(a, plain)
    rspec = dict(kind='radius', radius=0.12, min_neighbors=6)
    v = 0.08
    w0, w1 = voxel.downsample(p0, v), voxel.downsample(p1, v)
    g0, g1 = outliers.radius(w0.points, 0.12, 6), outliers.radius(w1.points, 0.12, 6)
    assert 0 < int(g0.points.shape[0]) < w0.points.shape[0]
    a = icp.refine(p0, p1, np.eye(4), max_dist=0.1, max_iter=8, voxel=v, outliers=rspec)
    b = icp.refine(g0.points, g1.points, np.eye(4), max_dist=0.1, max_iter=8)
    assert _same_result(a, b) and a.iters > 1
    d = fpfh.describe(p0, KC.TERRAIN_R, outliers=spec)
    e = fpfh.describe(f0.points, KC.TERRAIN_R)
    assert all(torch.equal(x, y) for x, y in zip(d, e)) and torch.equal(d.points, f0.points) and int(d.valid.sum()) > 1000
    nrm = icp.estimate_normals(p0, 0.1, outliers=spec)
    ref = icp.estimate_normals(f0.points, 0.1)
    assert len(nrm) == 4 and all(np.array_equal(x, y) for x, y in zip(nrm[:3], ref)) and np.array_equal(nrm[3], f0.rows.cpu().numpy())
    nrm = icp.estimate_normals(p0, 0.2, voxel=v, outliers=rspec)
    assert np.array_equal(nrm[3], w0.first[g0.rows.cpu().numpy()]) and nrm[0].shape[0] == int(g0.points.shape[0])
    both = outliers.radius(p0, 0.12, 6, voxel=v)
    assert torch.equal(both.points, g0.points) and np.array_equal(both.rows.cpu().numpy(), w0.first[g0.rows.cpu().numpy()])


def test_attach_points_composes_the_rows_with_the_voxels():
    from roreg_amd import outliers, voxel
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    eng = RegistrationEngine(default_config(), None, None)
    p0, _ = KC.outlier_cloud(1)
    spec = dict(kind='statistical', nb_neighbors=KC.OUT_NB, std_ratio=KC.OUT_STD)
    want = KC.outlier_reference(1)
    c = eng.attach_points(CloudState(before=None), p0, outliers=spec)
    assert c.points_rows.dtype == torch.int64 and np.array_equal(c.points_rows.cpu().numpy(), np.nonzero(want.mask)[0]) and np.array_equal(_bits(c.points), _bits(p0[want.mask]))
    v = 0.08
    w = voxel.downsample(p0, v)
    f = outliers.statistical(w.points, nb_neighbors=8, std_ratio=1.5)
    c = eng.attach_points(CloudState(before=None), p0, voxel=v, outliers=dict(kind='statistical', nb_neighbors=8, std_ratio=1.5))
    kept = f.rows.cpu().numpy()
    assert 0 < kept.shape[0] < w.points.shape[0]
    assert np.array_equal(c.points_rows.cpu().numpy(), w.first[kept]) and torch.equal(c.points, f.points)
    plain = eng.attach_points(CloudState(before=None), p0, voxel=v)
    assert plain.points_rows.dtype == torch.int32 and np.array_equal(plain.points_rows.cpu().numpy(), w.first)       # without a filter: what it was
    # run_scene's icp dict: the filter goes to attach_points, the rest to the iteration
    from roreg_amd.engine import split_icp_outliers, split_icp_voxel
    kw, vv, mode = split_icp_voxel(dict(max_dist=0.1, voxel=v, outliers=spec))
    kw, got = split_icp_outliers(kw)
    assert kw == dict(max_dist=0.1) and vv == v and got == spec


def test_without_outliers_refine_stays_on_the_recorded_bits():
    """outliers=None through icp.refine: the walls' runs of both methods are the bits tests/golden/icp_parent_bits.npz holds."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import record_icp_bits as rec
    from roreg_amd import icp
    golden = np.load(rec.FIXTURE)
    walls = [C.wall_pair(seed) for seed in C.WALL_SEEDS]
    for method in ('point', 'plane'):
        res = icp.refine([(q, p, T0) for q, p, _, T0 in walls], max_dist=C.WALL_DIST, max_iter=C.WALL_ITER, method=method, normal_radius=PC.RANK_RADIUS, outliers=None)
        assert np.array_equal(np.stack([r.T for r in res]).view(np.int64), golden[f'wall/{method}/T'])
        assert np.array_equal(np.array([r.iters for r in res], np.int32), golden[f'wall/{method}/iters'])
        assert np.array_equal(np.array([r.inliers for r in res], np.int32), golden[f'wall/{method}/inliers'])
        assert np.array_equal(np.array([r.rmse for r in res]).view(np.int64), golden[f'wall/{method}/rmse'])


def test_run_scene_with_outliers_in_the_icp_dict(tmp_path):
    """run_scene(..., icp={'outliers': {...}, ...}) equals the same call on points filtered beforehand, alone and behind 'voxel'; the caller's
    dict is left as it was and every cloud's points_rows are the kept rows."""
    from types import SimpleNamespace as NS
    from conftest import load_golden
    from roreg_amd import outliers, synth, voxel
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.group import tables
    from roreg_amd.network import name2network
    from roreg_amd.parses.parses_test import default_config
    z = load_golden('pipeline_mutual_yohoo')
    keynum = int(z['keynum'])
    cfg = default_config(output_cache_fn=f'{tmp_path}/cache', model_fn=f'{tmp_path}/ckpt', base_dir=str(tmp_path), SO3_related_files=None, keynum=keynum,
                         bs_GF=50, bs_ET=40, ET='yohoo')
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
    rng = np.random.default_rng(37)
    world = synth.make_dense_pair(37, 24000, noise=0.0)[0].astype(np.float64) + np.array([2.0, 1.5, 0.0])
    dense = {}
    for c, (g, t) in enumerate(ds.poses):           # cloud c sees world points x_w at R_g^T (x_w - t_c), and 200 stray points around them
        x = world[rng.permutation(world.shape[0])[:6000]] + rng.normal(0, 0.002, (6000, 3))
        x = np.concatenate([x, rng.uniform(x.min(0) - 0.3, x.max(0) + 0.3, (200, 3))])
        dense[c] = np.ascontiguousarray((x - t) @ tables().R[g], np.float32)
    spec, v = dict(kind='statistical', nb_neighbors=12, std_ratio=1.0), 0.04
    kw = {k: w for k, w in spec.items() if k != 'kind'}
    kept = {c: outliers.statistical(p, **kw) for c, p in dense.items()}
    kept_v = {c: outliers.statistical(voxel.downsample(p, v).points, **kw) for c, p in dense.items()}
    assert all(0 < int(r.points.shape[0]) <= dense[c].shape[0] - 100 for c, r in kept.items())
    keys = [ds.get_kps(i) for i in ds.pc_ids]
    runs = {}
    for kind, points, icp in (('filter', dense, dict(max_dist=0.1, max_iter=20, outliers=spec)),
                              ('before', {c: r.points.cpu().numpy() for c, r in kept.items()}, dict(max_dist=0.1, max_iter=20)),
                              ('voxel+filter', dense, dict(max_dist=0.1, max_iter=20, voxel=v, outliers=spec)),
                              ('voxel before', {c: r.points.cpu().numpy() for c, r in kept_v.items()}, dict(max_dist=0.1, max_iter=20)),
                              ('none', dense, dict(max_dist=0.1, max_iter=20, outliers=None)), ('full', dense, dict(max_dist=0.1, max_iter=20))):
        eng = RegistrationEngine(NS(**vars(cfg)), gf, et)
        np.random.seed(99)
        ready = {}
        runs[kind] = eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=keynum, max_iter=1000, points=points, icp=icp, ready=ready)
        if kind == 'filter':
            assert all(np.array_equal(c.points_rows.cpu().numpy(), kept[i].rows.cpu().numpy()) for i, c in ready.items())
        assert ('outliers' in icp) == (kind in ('filter', 'voxel+filter', 'none'))          # the caller's dict is left as it was
    bits = lambda w: np.ascontiguousarray(np.float64(w)).view(np.uint8)
    for x, y in (('filter', 'before'), ('voxel+filter', 'voxel before'), ('none', 'full')):
        for a, b in zip(runs[x], runs[y]):
            assert np.array_equal(bits(a.trans), bits(b.trans)) and np.array_equal(bits(a.trans_icp), bits(b.trans_icp)), (x, y)
            assert (a.icp_iters, a.icp_inliers, a.icp_status) == (b.icp_iters, b.icp_inliers, b.icp_status) and np.array_equal(bits(a.icp_rmse), bits(b.icp_rmse))
    assert any(a.icp_iters >= 1 for a in runs['filter'])
    assert any(a.icp_inliers != b.icp_inliers for a, b in zip(runs['filter'], runs['full']))
