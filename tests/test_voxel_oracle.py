"""CPU half of the voxel-grid downsampling tests: the interface exists (header, prototypes, exported symbols, Python entry points and their
argument checks), the numpy oracle equals a plain loop, and every family of tests/_voxel_cases.py reaches the branch the GPU tests
(tests/test_hip_voxel.py) rely on it to reach."""
import inspect
import os
import re

import numpy as np
import pytest

import _voxel_cases as C
import _voxel_oracle as O
from conftest import ROOT

V6E = ('roreg_voxel_workspace', 'roreg_voxel_downsample')


def test_v6e_names_are_declared_prototyped_and_exported():
    from roreg_amd import _abi, hip
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read(), flags=re.S)
    L = hip.lib()
    for name in V6E:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in roreg_hip.h'
        assert name in _abi.PROTOTYPES
        assert hasattr(L, name)
    assert _abi.ABI_VERSION == 6 and L.roreg_abi_version() == 6
    assert len(_abi.PROTOTYPES['roreg_voxel_downsample'][1]) == 12
    assert L.roreg_voxel_workspace(1000) > 0
    assert L.roreg_voxel_workspace(0) > 0                      # the table's 64 slots
    assert L.roreg_voxel_workspace(-1) == 0
    assert L.roreg_voxel_workspace(2000) > L.roreg_voxel_workspace(1000)
    assert hip.voxel_downsample is not None and hip.VoxelDev._fields == ('coords', 'first', 'counts', 'inverse', 'centroid')


def test_python_entry_points_and_keyword_arguments_exist():
    from roreg_amd import icp, voxel
    from roreg_amd.engine import CloudState, RegistrationEngine
    assert voxel.VoxelCloud._fields == ('points', 'coords', 'first', 'counts', 'inverse', 'centroid')
    sig = inspect.signature(voxel.downsample)
    assert sig.parameters['mode'].default == 'centroid' and sig.parameters['device'].default == 'cuda'
    for fn, names in ((icp.refine, ('voxel', 'voxel_mode')), (icp.estimate_normals, ('voxel',)), (RegistrationEngine.attach_points, ('voxel', 'voxel_mode'))):
        p = inspect.signature(fn).parameters
        for name in names:
            assert name in p, (fn.__name__, name)
        assert p['voxel'].default is None
    assert 'points_rows' in CloudState.__dataclass_fields__


@pytest.mark.parametrize('voxel', [0, -0.1, float('nan'), float('inf'), 'x', None])
def test_a_bad_voxel_raises_before_any_device_call(voxel, monkeypatch):
    from roreg_amd import hip, icp, voxel as V

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('voxel_downsample', 'IcpGrid', 'icp_batch', 'icp_normals', 'upload'):
        monkeypatch.setattr(hip, name, no_device)
    monkeypatch.setattr(icp, 'device_points', no_device)
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        V.downsample(p, voxel)
    if voxel is not None:                                   # None means 'no downsampling' to the consumers
        with pytest.raises(ValueError):
            icp.refine(p, p, np.eye(4), max_dist=0.1, voxel=voxel)
        with pytest.raises(ValueError):
            icp.estimate_normals(p, 0.1, voxel=voxel)


def test_a_bad_mode_raises_before_any_device_call(monkeypatch):
    from roreg_amd import hip, icp, voxel as V

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    for name in ('voxel_downsample', 'IcpGrid', 'icp_batch'):
        monkeypatch.setattr(hip, name, no_device)
    monkeypatch.setattr(icp, 'device_points', no_device)
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        V.downsample(p, 0.1, mode='mean')
    with pytest.raises(ValueError):
        icp.refine(p, p, np.eye(4), max_dist=0.1, voxel=0.1, voxel_mode='mean')


@pytest.mark.parametrize('method', ['point', 'plane'])
def test_refine_without_voxel_takes_the_existing_path_and_with_voxel_downsamples_each_array_once(method, monkeypatch):
    """On the call structure, no device: the uploaded tensor reaches IcpGrid as it is when voxel is None; with voxel= every distinct array goes
    through device_downsample exactly once, where it is uploaded, and the grids are built on what it returned."""
    from roreg_amd import hip, icp, voxel as V
    calls = []
    monkeypatch.setattr(icp, 'device_points', lambda p, device='cuda': ('dev', id(p)))
    monkeypatch.setattr(icp, 'device_transform', lambda T, device='cuda': 'T')
    monkeypatch.setattr(icp, 'results_to_host', lambda *a: ['r%d' % i for i in range(a[0])])
    monkeypatch.setattr(hip, 'IcpGrid', lambda pts, d: calls.append(('grid', pts)) or ('grid', pts))
    monkeypatch.setattr(hip, 'icp_normals', lambda g, r, k: ('normals', g))
    monkeypatch.setattr(hip, 'icp_batch', lambda pairs, *a: (len(pairs),) * 5)
    monkeypatch.setattr(hip, 'icp_plane_batch', lambda pairs, *a: (len(pairs),) * 5)
    monkeypatch.setattr(V, 'device_downsample', lambda pts, v, mode='centroid': calls.append(('voxel', pts, v, mode)) or (('down', pts), None))
    a, b, c = (np.zeros((3, 3)) for _ in range(3))
    items = [(a, b, np.eye(4)), (a, c, np.eye(4)), (b, a, np.eye(4))]
    assert icp.refine(items, max_dist=0.1, method=method) == ['r0', 'r1', 'r2']
    assert icp.refine(items, max_dist=0.1, method=method, voxel=None) == ['r0', 'r1', 'r2']
    assert all(k[0] == 'grid' and k[1][0] == 'dev' for k in calls) and len(calls) == 6
    del calls[:]
    icp.refine(items, max_dist=0.1, method=method, voxel=0.05, voxel_mode='first')
    vox = [k for k in calls if k[0] == 'voxel']
    assert sorted(k[1][1] for k in vox) == sorted(id(x) for x in (a, b, c)) and all(k[2:] == (0.05, 'first') for k in vox)
    assert sorted(k[1] for k in calls if k[0] == 'grid') == sorted(('down', k[1]) for k in vox)


def test_run_scene_takes_the_voxel_out_of_the_icp_arguments():
    from roreg_amd.engine import split_icp_voxel
    assert split_icp_voxel(None) == ({}, None, 'centroid')
    assert split_icp_voxel({'max_dist': 0.1}) == ({'max_dist': 0.1}, None, 'centroid')
    icp = {'max_dist': 0.1, 'voxel': 0.05, 'voxel_mode': 'first'}
    assert split_icp_voxel(icp) == ({'max_dist': 0.1}, 0.05, 'first') and 'voxel' in icp
    with pytest.raises(ValueError):
        split_icp_voxel({'voxel': -1.0})


def test_run_distributed_has_the_voxel_flags():
    src = open(os.path.join(ROOT, 'roreg_amd', 'run_distributed.py')).read()
    assert "'--icp_voxel'" in src and "'--icp_voxel_mode'" in src


# ---- the oracle --------------------------------------------------------------------------------------------------------------------------
def equal(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_the_oracle_equals_a_plain_loop_on_2000_random_points():
    rng = np.random.default_rng(0)
    p = (rng.random((2000, 3)) * 2.0 - 1.0).astype(np.float32)
    for v in (0.1, 0.3):
        a, b = O.downsample(p, v), O.downsample_loop(p, v)
        assert equal(a, b)
        assert a.counts.max() >= 4 and a.counts.sum() == 2000
        assert np.all(np.diff(a.first) > 0) and np.array_equal(a.coords[a.inverse], O.keys(p, v))
        assert np.array_equal(O.downsample(p, v, 'first').points, p[a.first])


def test_np_add_at_adds_in_index_order():
    x = C.order_rows().astype(np.float64)
    s = np.zeros(1)
    np.add.at(s, np.zeros(7, np.int64), x)
    asc = 0.0
    for v in x:
        asc = asc + v
    assert s[0] == asc


@pytest.mark.parametrize('v', C.LATTICE_VOXELS)
def test_lattice_family(v):
    vals = C.lattice_values(v)
    assert vals.shape == (24000,)
    moved = int((np.floor(vals.astype(np.float64) / v) != np.floor(vals / np.float32(v))).sum())
    if v != 0.25:                                           # a dyadic voxel divides exactly in either format
        assert moved >= 1000, moved
    else:
        assert moved == 0
    p = C.lattice(v)
    r = O.downsample(p, v)
    assert r.coords.min() == -C.KEY_LIM and r.coords.max() == C.KEY_LIM - 1
    assert r.counts.max() >= 3 and r.counts.min() == 1
    zero = p[(p == 0).any(1)]
    assert np.signbit(zero).any() and (O.keys(zero, v)[zero == 0] == 0).all()                # -0.0 is there and falls in voxel 0
    with pytest.raises(O.BadInput):
        O.keys(np.array([[C.beyond_value(v), 0, 0]], np.float32), v)
    assert np.floor(np.float64(C.beyond_value(v)) / v) == C.KEY_LIM


def test_size_families():
    for n in C.SIZES:
        r = O.downsample(C.cube(n), C.SIZES_VOXEL)
        assert r.inverse.shape == (n,) and r.counts.sum() == n
    p, v = C.all_distinct()
    assert O.downsample(p, v).first.shape[0] == p.shape[0] == 17 ** 3
    p, v = C.one_voxel()
    assert O.downsample(p, v).first.shape[0] == 1 and p.shape[0] == 3000


@pytest.mark.parametrize('name', C.STRUCTURED)
def test_structured_families(name):
    p = C.structured(name)
    r = O.downsample(p, 0.05)
    assert r.first.shape[0] == (256 if name == 'top_bits' else 4096)
    assert r.counts.min() == 1 and r.counts.max() == 3
    moving = [a for a in range(3) if np.unique(r.coords[:, a]).shape[0] > 1]
    assert len(moving) == (2 if name == 'plane' else 1)
    if name == 'top_bits':
        assert np.all(r.coords[:, 1] % 4096 == 0)


@pytest.mark.parametrize('v', C.ROOM_VOXELS)
def test_room_family(v):
    p = C.room()
    r = O.downsample(p, v)
    assert p.shape == (C.ROOM_N, 3) and (r.first.shape[0], int(r.counts.max())) == C.ROOM_EXPECT[v]
    assert r.coords.min() < 0 < r.coords.max()


def test_order_family():
    x = C.order_rows().astype(np.float64)
    asc, desc = x[0], x[-1]
    for a in x[1:]:
        asc = asc + a
    for a in x[-2::-1]:
        desc = desc + a
    assert asc != desc and asc != C.tree_sum(x)
    p, v, pos = C.order_cloud()
    r = O.downsample(p, v)
    vox = r.inverse[pos[:, 0]]
    assert np.unique(vox).shape[0] == 200 and (r.counts[vox] == 7).all()
    assert (r.inverse[pos] == vox[:, None]).all()
    assert (r.centroid[vox, 0] == asc / 7.0).all() and (r.centroid[vox, 0] != desc / 7.0).all()


def test_outlier_family():
    p, v = C.outlier_cloud()
    r = O.downsample(p, v)
    assert r.coords.max() == 800000 and r.coords.min() == -800000 and p.shape[0] == 5001
