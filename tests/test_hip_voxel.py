"""Voxel-grid downsampling on the device (roreg_amd/csrc/voxel.hip) against its numpy restatement (tests/_voxel_oracle.py): every output equal,
bit for bit, on the families of tests/_voxel_cases.py (whose conditions tests/test_voxel_oracle.py asserts on the CPU)."""
import numpy as np
import pytest
import torch

import _icp_oracle as IO
import _icp_plane_cases as PC
import _voxel_cases as C
import _voxel_oracle as O

pytestmark = pytest.mark.gpu

FIELDS = ('points', 'coords', 'first', 'counts', 'inverse', 'centroid')


def device(p, v, mode='centroid'):
    from roreg_amd import voxel
    return voxel.downsample(p, v, mode)


def assert_equal(got, want, what=''):
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype.kind == 'f':                     # bit for bit: -0.0 and 0.0 differ
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (what, f, int((g != w).sum()))
        else:
            assert np.array_equal(g, w), (what, f, int((g != w).sum()))


def check(p, v, what=''):
    want = O.downsample(p, v)
    got = device(p, v)
    assert_equal(got, want, what)
    first = device(p, v, 'first')
    assert np.array_equal(first.points.view(np.uint8), np.ascontiguousarray(p[want.first]).view(np.uint8)), what
    assert np.array_equal(first.first, want.first)
    return got


@pytest.mark.parametrize('v', C.LATTICE_VOXELS)
def test_lattice_of_voxel_boundaries_and_their_float32_neighbours(v):
    from roreg_amd import hip
    p = C.lattice(v)
    got = check(p, v, f'lattice {v}')
    assert got.coords.min() == -C.KEY_LIM and got.coords.max() == C.KEY_LIM - 1
    bad = np.concatenate((p, np.array([[0.5 * v, C.beyond_value(v), -0.5 * v]], np.float32)))
    with pytest.raises(hip.HipError):
        device(bad, v)
    assert_equal(device(p, v), O.downsample(p, v), 'after the out-of-range row')


@pytest.mark.parametrize('n', C.SIZES)
def test_sizes_around_a_wave_a_workgroup_and_a_scan_block(n):
    got = check(C.cube(n), C.SIZES_VOXEL, f'n = {n}')
    assert got.inverse.shape == (n,) and (n == 0) == (got.first.shape[0] == 0)


def test_one_point_per_voxel_and_all_points_in_one_voxel():
    p, v = C.all_distinct()
    assert check(p, v, 'all distinct').first.shape[0] == p.shape[0]
    p, v = C.one_voxel()
    got = check(p, v, 'one voxel')
    assert got.first.shape[0] == 1 and got.counts[0] == 3000


@pytest.mark.parametrize('name', C.STRUCTURED)
def test_structured_keys(name):
    check(C.structured(name), 0.05, name)


@pytest.mark.parametrize('v', C.ROOM_VOXELS)
def test_room_scan_is_exact_repeatable_and_independent_of_the_row_order(v):
    p = C.room()
    got = check(p, v, f'room {v}')
    assert (got.first.shape[0], int(got.counts.max())) == C.ROOM_EXPECT[v]
    assert_equal(device(p, v), got, 'second call')
    perm = np.random.default_rng(5).permutation(p.shape[0])
    other = device(np.ascontiguousarray(p[perm]), v)
    canon = lambda r: np.unique(np.concatenate((r.coords, r.counts[:, None]), 1), axis=0)
    assert np.array_equal(canon(other), canon(got))
    assert_equal(other, O.downsample(p[perm], v), 'permuted')


def test_the_centroid_is_the_ascending_sequential_sum():
    p, v, pos = C.order_cloud()
    got = check(p, v, 'order')
    x = C.order_rows().astype(np.float64)
    asc = x[0]
    for a in x[1:]:
        asc = asc + a
    vox = got.inverse[pos[:, 0]]
    assert (got.centroid[vox, 0] == asc / 7.0).all() and (got.centroid[vox, 2] == asc / 7.0).all()


def test_a_far_outlier_is_one_more_key():
    p, v = C.outlier_cloud()
    got = check(p, v, 'outlier')
    assert got.coords.max() == 800000


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf])
def test_a_non_finite_row_raises_and_the_next_call_is_clean(bad):
    from roreg_amd import hip
    p = C.cube(1000).copy()
    q = p.copy()
    q[517, 1] = bad
    with pytest.raises(hip.HipError):
        device(q, 0.1)
    assert_equal(device(p, 0.1), O.downsample(p, 0.1), 'after the non-finite row')


def test_flagged_rows_take_no_voxel():
    """The C entry itself on a cloud with a NaN row and an out-of-range row: flags 1 | 2, inverse -1 on those rows, and the other rows
    numbered as the oracle numbers the cloud without them."""
    from roreg_amd import hip
    from roreg_amd.hip import _ptr, _stream, lib
    p = C.cube(300).copy()
    p[7, 0] = np.nan
    p[100, 2] = 3e5                                 # key 3e6 at voxel 0.1
    n = p.shape[0]
    d = torch.from_numpy(p).cuda()
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device='cuda')
    inverse, first, counts, coords, info = i32(n), i32(n), i32(n), i32(n, 3), i32(2)
    centroid = torch.empty((n, 3), dtype=torch.float64, device='cuda')
    ws_n = lib().roreg_voxel_workspace(n)
    ws = torch.empty(ws_n, dtype=torch.uint8, device='cuda')
    rc = lib().roreg_voxel_downsample(_ptr(d), n, 0.1, _ptr(inverse), _ptr(first), _ptr(counts), _ptr(coords), _ptr(centroid), _ptr(info), _ptr(ws), ws_n, _stream())
    assert rc == 0
    m, flags = info.cpu().numpy()
    keep = np.ones(n, bool); keep[[7, 100]] = False
    want = O.downsample(p[keep], 0.1)
    rows = np.flatnonzero(keep)
    assert flags == 3 and m == want.first.shape[0]
    inv = inverse.cpu().numpy()
    assert inv[7] == -1 and inv[100] == -1 and np.array_equal(inv[keep], want.inverse)
    assert np.array_equal(first.cpu().numpy()[:m], rows[want.first]) and np.array_equal(counts.cpu().numpy()[:m], want.counts)
    assert np.array_equal(coords.cpu().numpy()[:m], want.coords) and np.array_equal(centroid.cpu().numpy()[:m], want.centroid)
    assert hip.VOXEL_FLAGS[0] and rc == 0


# ---- consumers -------------------------------------------------------------------------------------------------------------------------
CONS_VOXEL = 0.05


def same(a, b):
    return (np.array_equal(a.T.view(np.uint8), b.T.view(np.uint8)) and (a.iters, a.inliers, a.status) == (b.iters, b.inliers, b.status)
            and np.array_equal(np.array([a.rmse], np.float64).view(np.uint8), np.array([b.rmse], np.float64).view(np.uint8)))


@pytest.mark.parametrize('method', ['point', 'plane'])
@pytest.mark.parametrize('mode', ['centroid', 'first'])
def test_refine_with_voxel_equals_refine_on_the_oracles_downsampled_clouds(method, mode):
    from roreg_amd import icp
    p0, p1, _ = PC.conv_pair()
    assert p0.shape[0] == 20000
    T0 = PC.conv_starts()[0]
    P0, P1 = O.downsample(p0, CONS_VOXEL, mode).points, O.downsample(p1, CONS_VOXEL, mode).points
    assert 1000 < P0.shape[0] < p0.shape[0]
    got = icp.refine(p0, p1, T0, PC.CONV_DIST, method=method, voxel=CONS_VOXEL, voxel_mode=mode)
    want = icp.refine(P0, P1, T0, PC.CONV_DIST, method=method)
    assert same(got, want), (got, want)
    assert got.iters > 1 and got.inliers > 1000
    full = icp.refine(p0, p1, T0, PC.CONV_DIST, method=method)
    assert same(icp.refine(p0, p1, T0, PC.CONV_DIST, method=method, voxel=None), full)
    assert not same(got, full)


def test_estimate_normals_with_voxel_returns_the_downsampled_clouds_normals_and_rows():
    from roreg_amd import icp
    p0 = PC.conv_pair()[0]
    want = O.downsample(p0, CONS_VOXEL)
    nrm, valid, cnt, rows = icp.estimate_normals(p0, 0.2, voxel=CONS_VOXEL)
    ref = icp.estimate_normals(want.points, 0.2)
    assert len(ref) == 3 and np.array_equal(rows, want.first)
    assert np.array_equal(nrm.view(np.uint8), ref[0].view(np.uint8)) and np.array_equal(valid, ref[1]) and np.array_equal(cnt, ref[2])


def test_attach_points_and_run_scene_with_voxel_equal_the_same_calls_on_downsampled_points():
    from roreg_amd import hip
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    eng = RegistrationEngine(default_config(), None, None)
    p0, p1, _ = PC.conv_pair()
    w0, w1 = O.downsample(p0, CONS_VOXEL), O.downsample(p1, CONS_VOXEL)
    c0 = eng.attach_points(CloudState(before=None), p0, voxel=CONS_VOXEL)
    assert np.array_equal(c0.points.cpu().numpy().view(np.uint8), w0.points.view(np.uint8)) and np.array_equal(c0.points_rows.cpu().numpy(), w0.first)
    plain = eng.attach_points(CloudState(before=None), p0)
    assert plain.points_rows is None and plain.points.shape[0] == p0.shape[0]
    c1 = eng.attach_points(CloudState(before=None), p1, voxel=CONS_VOXEL, voxel_mode='first')
    assert np.array_equal(c1.points.cpu().numpy(), p1[w1.first])
    T0 = hip.upload(PC.conv_starts()[0])
    a = eng.icp_many([(c0, eng.attach_points(CloudState(before=None), p1, voxel=CONS_VOXEL), T0)], PC.CONV_DIST)
    b = eng.icp_many([(eng.attach_points(CloudState(before=None), w0.points), eng.attach_points(CloudState(before=None), w1.points), T0)], PC.CONV_DIST)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))


def test_run_scene_with_voxel_in_the_icp_dict(tmp_path):
    """run_scene(..., icp={'voxel': v, ...}) equals the same call on points downsampled beforehand; voxel None is the call without the key."""
    from types import SimpleNamespace as NS
    from conftest import load_golden
    from roreg_amd import synth
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
    rng = np.random.default_rng(31)
    world = synth.make_dense_pair(31, 24000, noise=0.0)[0].astype(np.float64) + np.array([2.0, 1.5, 0.0])
    dense = {}
    for c, (g, t) in enumerate(ds.poses):           # cloud c sees world points x_w at R_g^T (x_w - t_c)
        x = world[rng.permutation(world.shape[0])[:8000]] + rng.normal(0, 0.002, (8000, 3))
        dense[c] = np.ascontiguousarray((x - t) @ tables().R[g], np.float32)
    down = {c: O.downsample(p, CONS_VOXEL).points for c, p in dense.items()}
    assert all(down[c].shape[0] < 0.9 * dense[c].shape[0] for c in dense)
    keys = [ds.get_kps(i) for i in ds.pc_ids]
    runs = {}
    for kind, points, icp in (('voxel', dense, dict(max_dist=0.1, max_iter=20, voxel=CONS_VOXEL)), ('before', down, dict(max_dist=0.1, max_iter=20)),
                              ('none', dense, dict(max_dist=0.1, max_iter=20, voxel=None)), ('full', dense, dict(max_dist=0.1, max_iter=20))):
        eng = RegistrationEngine(NS(**vars(cfg)), gf, et)
        np.random.seed(99)
        ready = {}
        runs[kind] = eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=keynum, max_iter=1000, points=points, icp=icp, ready=ready)
        if kind == 'voxel':
            assert all(np.array_equal(c.points_rows.cpu().numpy(), O.downsample(dense[i], CONS_VOXEL).first) for i, c in ready.items())
        assert ('voxel' in icp) == (kind in ('voxel', 'none'))          # the caller's dict is left as it was
    bits = lambda v: np.ascontiguousarray(np.float64(v)).view(np.uint8)
    for x, y in (('voxel', 'before'), ('none', 'full')):
        for a, b in zip(runs[x], runs[y]):
            assert np.array_equal(bits(a.trans), bits(b.trans)) and np.array_equal(bits(a.trans_icp), bits(b.trans_icp)), (x, y)
            assert (a.icp_iters, a.icp_inliers, a.icp_status) == (b.icp_iters, b.icp_inliers, b.icp_status) and np.array_equal(bits(a.icp_rmse), bits(b.icp_rmse))
    assert any(a.icp_iters >= 1 for a in runs['voxel'])
    assert any(a.icp_inliers != b.icp_inliers for a, b in zip(runs['voxel'], runs['full']))
