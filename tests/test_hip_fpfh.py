"""The FPFH kernels (csrc/fpfh.hip, "v6n") and roreg_amd/fpfh.py on the device against tests/_fpfh_oracle.py, on the families of
tests/_fpfh_cases.py (tests/test_fpfh_oracle.py checks the families' own conditions on the CPU)."""
import numpy as np
import pytest
import torch

import _fpfh_cases as K
import _fpfh_oracle as FO
import _icp_plane_cases as PC

pytestmark = pytest.mark.gpu


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _grid(p, d):
    from roreg_amd import hip
    return hip.IcpGrid(_cuda(np.asarray(p, np.float32).reshape(-1, 3), np.float32), d)


def test_orientation_equals_the_oracle_bits():
    """5,000 axis-aligned points, normals and viewpoint: zero rows stay zero, a dot product of exactly 0 keeps its sign, column 3 is copied."""
    from roreg_amd import hip
    pts, nrm = K.orient_case()
    want = FO.orient(pts, nrm, K.ORIENT_VIEWPOINT)
    dots = FO.dot(nrm[:, :3], np.float64(K.ORIENT_VIEWPOINT)[None] - pts.astype(np.float64))
    valid = FO.valid_normals(nrm)
    assert (~valid).sum() > 500 and (valid & (dots == 0.0)).sum() > 300 and (dots < 0).sum() > 1000 and (dots > 0).sum() > 1000
    for d in (1.0, 3.0):
        got = hip.fpfh_orient(_grid(pts, d), _cuda(nrm, np.float64), K.ORIENT_VIEWPOINT).cpu().numpy()
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    assert not got[~valid, :3].any() and np.array_equal(got[valid & (dots == 0.0)], nrm[valid & (dots == 0.0)])


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_spfh_counts_equal_the_oracle_at_every_row(case):
    from roreg_amd import hip
    pts, nrm, r = K.case(*case)
    want_counts, want_m = K.reference(*case)[:2]
    dists = tuple(d * r / PC.LAT_R for d in PC.LAT_GRID_DISTS) if case[0] == 'lattice' else (r,)
    tables = []
    for d in dists + dists[:1]:                                   # (the last: a second run on a grid of its own)
        counts, m = hip.fpfh_spfh(_grid(pts, d), _cuda(nrm, np.float64), r)
        tables.append((counts.cpu().numpy(), m.cpu().numpy()))
    counts, m = tables[0]
    assert counts.dtype == np.int32 and counts.shape == (pts.shape[0], 33) and m.shape == (pts.shape[0],)
    bad = np.nonzero((counts != want_counts).any(1) | (m != want_m))[0]
    assert bad.size == 0, f'{bad.size} of {pts.shape[0]} rows differ, the first: row {bad[0]}, m {m[bad[0]]} against {want_m[bad[0]]}'
    for c2, m2 in tables[1:]:
        assert c2.tobytes() == counts.tobytes() and m2.tobytes() == m.tobytes()


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_fpfh_pass_within_one_float32_step_of_the_oracle(case):
    """Fed the oracle's counts.  The float64 sums of at most a few thousand non-negative terms differ between summation orders by far less
    than 2^-24 relative, so the float32 rounding of a feature can differ from the oracle's by one step at most."""
    from roreg_amd import hip
    pts, _, r = K.case(*case)
    counts, m, want, want_valid, _ = K.reference(*case)
    got, valid = hip.fpfh_features(_grid(pts, r), _cuda(counts, np.int32), _cuda(m, np.int32), r)
    got, valid = got.cpu().numpy(), valid.cpu().numpy().astype(bool)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(valid, want_valid) and not got[~valid].any()
    lo, hi = FO.neighbours_f32(want)
    differs = got != want
    print(f'{case}: {int(differs.sum())} of {got.size} features differ from the oracle\'s float32 ({differs.mean():.2e})')
    assert ((got == want) | (got == lo) | (got == hi)).all()
    assert np.isfinite(got).all() and (got >= 0).all()


def test_describe_is_the_composition_of_its_parts():
    from roreg_amd import fpfh, hip, icp, voxel
    p = K.terrain_pair(1)[0]
    radius, v = 0.25, 0.05
    d = fpfh.describe(p, radius, voxel=v)
    vc = voxel.downsample(p, v)
    normals, ok, cnt = icp.estimate_normals(vc.points, radius / 2.5)
    grid = _grid(vc.points, radius)
    c = torch.from_numpy(vc.points).cuda().double().mean(0).cpu().numpy()
    oriented = hip.fpfh_orient(grid, _cuda(np.concatenate([normals, cnt[:, None].astype(np.float64)], 1), np.float64), c)
    counts, m = hip.fpfh_spfh(grid, oriented, radius)
    feats, valid = hip.fpfh_features(grid, counts, m, radius)
    assert torch.equal(d.points.cpu(), torch.from_numpy(vc.points)) and torch.equal(d.normals.view(torch.int64), oriented.view(torch.int64))
    assert torch.equal(d.features.view(torch.int32), feats.view(torch.int32)) and torch.equal(d.valid, valid)
    assert 4000 < d.points.shape[0] < 8000 and int(d.valid.sum()) > 0.95 * d.points.shape[0]
    # an explicit viewpoint and normal radius reach the kernels too
    d2 = fpfh.describe(p, radius, normal_radius=0.15, voxel=v, viewpoint=(0.0, 0.0, 10.0))
    towards = ((torch.tensor([0.0, 0.0, 10.0], dtype=torch.float64, device='cuda') - d2.points.double()) * d2.normals[:, :3]).sum(1)
    assert not torch.equal(d2.features, d.features) and (towards >= -1e-12).all() and (towards > 0).sum() > 4000


@pytest.mark.parametrize('n', (0, 1))
def test_describe_of_an_empty_and_of_a_one_point_cloud(n):
    from roreg_amd import fpfh
    d = fpfh.describe(np.zeros((n, 3), np.float32) + 0.5, 0.25)
    assert tuple(d.points.shape) == (n, 3) and tuple(d.normals.shape) == (n, 4) and tuple(d.features.shape) == (n, 33) and tuple(d.valid.shape) == (n,)
    assert not d.valid.any() and not d.features.any()
    assert tuple(fpfh.match(d, d).shape) == (0, 2)


@pytest.mark.parametrize('seed', K.TERRAIN_SEEDS)
def test_register_lands_on_the_terrain_pose(seed):
    """fpfh.register at voxel 0.05 within 2 degrees and 5 cm of the ground truth (the bar of the oracle chain in tests/test_fpfh_oracle.py, for
    the same reason); point-to-plane ICP on the downsampled clouds makes neither error larger."""
    from roreg_amd import fpfh
    p0, p1, Tg = K.terrain_pair(seed)
    res = fpfh.register(p0, p1, voxel=K.TERRAIN_VOXEL, icp=dict(method='plane', max_dist=0.1))
    deg, dt = K.pose_error(res.trans, Tg)
    deg_icp, dt_icp = K.pose_error(res.trans_icp, Tg)
    print(f'terrain seed {seed}: {res.matches.shape[0]} matches, estimator {deg:.3f} degrees / {dt * 100:.2f} cm, after ICP ({res.icp.status}, '
          f'{res.icp.iters} iterations) {deg_icp:.3f} degrees / {dt_icp * 100:.2f} cm')
    assert deg <= K.TERRAIN_DEG and dt <= K.TERRAIN_T
    assert deg_icp <= deg and dt_icp <= dt


def test_register_scene_equals_the_pairs_one_by_one():
    from roreg_amd import fpfh, synth
    p0, p1, _ = K.terrain_pair(0)
    T2 = synth.dense_gt(-25.0, (0.0, 1.0, 1.0), (-0.2, 0.4, 0.1))
    p2 = ((p0[::2].astype(np.float64) - T2[:3, 3]) @ T2[:3, :3]).astype(np.float32)          # a third view: every other point of view 0, moved
    clouds, pairs = [p0, p1, p2], [(0, 1), (2, 1)]
    scene = fpfh.register_scene(clouds, pairs, voxel=K.TERRAIN_VOXEL)
    for (i, j), got in zip(pairs, scene):
        one = fpfh.register(clouds[i], clouds[j], voxel=K.TERRAIN_VOXEL)
        assert np.array_equal(got.matches, one.matches) and got.matches.shape[0] > 500
        assert np.array_equal(got.trans.view(np.int64), one.trans.view(np.int64)) and np.isfinite(got.trans).all()
        assert got.trans_icp is None and one.trans_icp is None
