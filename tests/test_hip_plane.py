"""The plane segmentation kernels (csrc/plane.hip, "v6t") and roreg_amd/segment.py on the device against tests/_plane_oracle.py, on the families of
tests/_plane_cases.py (tests/test_plane_oracle.py checks the families' own conditions on the CPU).  labels, n_planes, counts, triples and the raw
planes are compared by their bytes; the least-squares fit, which decides nothing, against numpy's eigh within the bound of
tests/test_hip_icp_plane.py."""
import numpy as np
import pytest
import torch

import _cluster_oracle as CO
import _plane_cases as K
import _plane_oracle as PO
import _voxel_oracle as VO

pytestmark = pytest.mark.gpu

GAP_MIN = 1e-3           # planes whose covariance has (lambda_mid - lambda_min) / lambda_max below this are left out of the fit comparison


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _run(case):
    from roreg_amd import hip
    pts, dist, H, planes, min_inliers, seed = K.case(*case)
    return [v.cpu().numpy() for v in hip.plane_segment(_cuda(pts.reshape(-1, 3)), dist, H, planes, min_inliers, seed)]


def _assert_equals_oracle(got, want, what):
    labels, n_planes, counts, triples, raw, fit, rms = got
    assert labels.dtype == np.int32 and n_planes.dtype == np.int32 and counts.dtype == np.int32 and triples.dtype == np.int32 and raw.dtype == np.float64
    assert fit.dtype == np.float64 and rms.dtype == np.float64
    assert labels.shape == want.labels.shape and n_planes.shape == (1,) and counts.shape == want.counts.shape and triples.shape == want.triples.shape
    assert raw.shape == want.raw.shape and fit.shape == want.fit.shape and rms.shape == want.rms.shape
    assert int(n_planes[0]) == want.n_planes, f'{what}: {int(n_planes[0])} planes against {want.n_planes}'
    assert np.array_equal(counts, want.counts), f'{what}: counts {counts.tolist()} against {want.counts.tolist()}'
    assert np.array_equal(triples, want.triples), f'{what}: triples {triples.tolist()} against {want.triples.tolist()}'
    assert raw.tobytes() == want.raw.tobytes(), f'{what}: raw planes differ'
    bad = np.flatnonzero(labels != want.labels)
    assert bad.size == 0, f'{what}: {bad.size} of {labels.shape[0]} labels differ, the first: row {bad[0]}, {labels[bad[0]]} against {want.labels[bad[0]]}'


def _angle(a, b):
    return float(np.arctan2(np.sqrt((np.cross(a, b) ** 2).sum()), (a * b).sum()))


def _check_fit(pts, got, want, what):
    """-> (planes compared, planes left out by the gap rule, the worst fraction of the angle bound).  The angle within 1e-12 lambda_max /
    (lambda_mid - lambda_min) (tests/test_hip_icp_plane.py _normal_bound); every inlier's distance to the two planes within that angle times the
    inliers' radius plus 1e-12 of the cloud's extent.  rms: 1e-9 relative; where the oracle's rms is itself below 1e-12 of the extent (an exact
    plane: both values are rounding residue of the distances, which the line above allows to differ by that much) within that floor instead."""
    labels, fit, rms = got[0], got[5], got[6]
    X = PO.widen(pts)
    finite = X[np.isfinite(X).all(1)]
    extent = float((finite.max(0) - finite.min(0)).max()) if finite.shape[0] else 0.0
    floor = 1e-12 * extent
    done = left = 0
    worst = 0.0
    assert (fit[want.n_planes:] == 0).all() and (rms[want.n_planes:] == 0).all()
    for r in range(want.n_planes):
        assert abs(np.sqrt((fit[r, :3] ** 2).sum()) - 1.0) <= 1e-15 and (fit[r, :3] * want.raw[r, :3]).sum() >= 0.0
        if PO.gap_ratio(want.lam[r])[0] < GAP_MIN:
            left += 1
            continue
        done += 1
        bound = 1e-12 * want.lam[r, 2] / (want.lam[r, 1] - want.lam[r, 0])
        ang = _angle(fit[r, :3], want.fit[r, :3])
        worst = max(worst, ang / bound)
        Y = X[labels == r]
        c0 = Y.mean(0)
        radius = float(np.sqrt(((Y - c0) ** 2).sum(1)).max())
        d_dev = (Y - c0) @ fit[r, :3] + ((fit[r, :3] * c0).sum() + fit[r, 3])
        d_ref = (Y - c0) @ want.fit[r, :3] + ((want.fit[r, :3] * c0).sum() + want.fit[r, 3])
        dd = float(np.abs(d_dev - d_ref).max())
        tol = 1e-9 * want.rms[r] if want.rms[r] > floor else floor
        print(f'{what} plane {r}: {Y.shape[0]} rows, gap ratio {PO.gap_ratio(want.lam[r])[0]:.3g}, angle {ang:.3e} (bound {bound:.3e}), distances differ by at most '
              f'{dd:.3e} (allowed {bound * radius + floor:.3e}), rms {float(rms[r])!r} against {float(want.rms[r])!r} (allowed {tol:.3e})')
        assert ang <= bound, (what, r)
        assert dd <= bound * radius + floor, (what, r)
        assert abs(rms[r] - want.rms[r]) <= tol, (what, r)
    return done, left, worst


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_segmentation_equals_the_oracle(case):
    """hip.plane_segment on every case: the oracle's bytes, the same bytes on a second run (fit and rms too: fixed slots), the fit within its bound"""
    got = _run(case)
    want = K.reference(*case)
    _assert_equals_oracle(got, want, K.case_id(case))
    again = _run(case)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    done, left, _ = _check_fit(K.case(*case)[0], got, want, K.case_id(case))
    if case[0] in ('room', 'objects') or case == ('early', 'room'):
        assert left == 0 and done == want.n_planes >= 5               # none of the room's planes falls under the gap rule


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_score_of_round_zeros_triples_equals_the_oracle(case):
    """hip.plane_score on the triples round 0 drew (rows as drawn, -1 where two draws were equal): the oracle's counts of that round"""
    from roreg_amd import hip
    pts = K.case(*case)[0]
    want = K.reference(*case)
    counts = hip.plane_score(_cuda(pts.reshape(-1, 3)), _cuda(want.hyp_triples, np.int32), K.case(*case)[1])
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want.hyp_counts)


@pytest.mark.parametrize('name', K.SCORE_CASES)
def test_score_edges(name):
    """a repeated row, a row of -1, a row of n, a dead row, no triples, an empty cloud; the lattice's axis plane at dist = 1 and one step below"""
    from roreg_amd import hip
    pts, triples, dist = K.score_case(name)
    a = hip.plane_score(_cuda(pts), _cuda(triples, np.int32), dist)
    b = hip.plane_score(_cuda(pts), _cuda(triples, np.int32), dist)
    assert np.array_equal(a.cpu().numpy(), K.score_reference(name)) and torch.equal(a, b)


def test_caps_and_bad_arguments_raise_value_error():
    from roreg_amd import hip, segment
    pts = _cuda(K.slab_cloud(65))
    for kw in (dict(n_hyp=hip.PLANE_MAX_HYP + 1), dict(max_planes=hip.PLANE_MAX_PLANES + 1), dict(n_hyp=0), dict(max_planes=-1), dict(min_inliers=2), dict(seed=-1),
               dict(seed=2 ** 64), dict(dist=0.0), dict(dist=float('nan'))):
        args = dict(dist=0.02, n_hyp=16, max_planes=1, min_inliers=3, seed=0)
        args.update(kw)
        with pytest.raises(ValueError):
            hip.plane_segment(pts, **args)
        with pytest.raises(ValueError):
            segment.device_planes(pts, **args)
    for bad in (pts.double(), pts[:, :2].contiguous(), pts.reshape(-1), pts.cpu(), pts.t(), pts.cpu().numpy()):
        with pytest.raises(ValueError):
            hip.plane_segment(bad, 0.02)
        with pytest.raises(ValueError):
            hip.plane_score(bad, torch.zeros((1, 3), dtype=torch.int32).cuda(), 0.02)
    for bad in (torch.zeros((1, 3), dtype=torch.int64).cuda(), torch.zeros((1, 2), dtype=torch.int32).cuda(), torch.zeros((1, 3), dtype=torch.int32),
                torch.zeros((hip.PLANE_MAX_HYP + 1, 3), dtype=torch.int32).cuda()):
        with pytest.raises(ValueError):
            hip.plane_score(pts, bad, 0.02)
    with pytest.raises(ValueError):
        hip.plane_score(pts, torch.zeros((1, 3), dtype=torch.int32).cuda(), -1.0)
    assert int(hip.plane_segment(pts, 0.02, seed=2 ** 64 - 1)[1]) == 1                     # the whole range of seeds


def test_planes_of_a_host_cloud_and_of_its_voxels():
    """segment.planes / plane / device_planes: the oracle's result cut to the planes found, unit normals; voxel= equals voxel.device_downsample
    followed by device_planes, and the oracle on the voxel oracle's centroids"""
    from roreg_amd import segment, voxel
    case = K.ROOM_CASES[0]
    pts, dist, H, planes, min_inliers, seed = K.case(*case)
    want = K.reference(*case)
    res = segment.planes(pts, dist, planes, min_inliers, H, seed)
    k = want.n_planes
    assert res.n_planes == k and all(int(v.shape[0]) == k for v in (res.planes, res.fit, res.counts, res.triples, res.rms))
    assert np.array_equal(res.labels.cpu().numpy(), want.labels) and np.array_equal(res.counts.cpu().numpy(), want.counts[:k])
    assert np.array_equal(res.triples.cpu().numpy(), want.triples[:k])
    assert np.abs(res.planes.cpu().numpy() - PO.unit(want.raw[:k])).max() <= 1e-15 and res.planes.dtype == torch.float64
    one = segment.plane(pts, dist, min_inliers, H, seed)
    assert one.n_planes == 1 and torch.equal(one.triples, res.triples[:1]) and np.array_equal(one.labels.cpu().numpy(), np.where(want.labels == 0, 0, -1))
    dev = segment.device_planes(_cuda(pts), dist, planes, min_inliers, H, seed)
    assert dev.n_planes.shape == (1,) and int(dev.n_planes) == k and dev.planes.shape == (planes, 4) and torch.equal(dev.planes[:k], res.planes)
    assert (dev.planes[k:] == 0).all() and torch.equal(dev.labels, res.labels)
    vs = 0.05
    v = segment.planes(pts, dist, planes, 30, H, seed, voxel=vs)
    down = voxel.device_downsample(_cuda(pts), vs)[0]
    by_hand = segment.device_planes(down, dist, planes, 30, H, seed)
    kv = int(by_hand.n_planes)
    assert v.n_planes == kv >= 3 and torch.equal(v.labels, by_hand.labels) and torch.equal(v.triples, by_hand.triples[:kv]) and torch.equal(v.planes, by_hand.planes[:kv])
    cen = np.ascontiguousarray(VO.downsample(pts, vs).points, np.float32)
    ref = PO.segment(cen, dist, H, planes, 30, seed)
    assert np.array_equal(down.cpu().numpy(), cen) and np.array_equal(v.labels.cpu().numpy(), ref.labels) and np.array_equal(v.counts.cpu().numpy(), ref.counts[:kv])
    spec = dict(kind='radius', radius=0.1, min_neighbors=3)
    from roreg_amd import outliers
    kept = outliers.radius(pts, 0.1, 3).points
    f = segment.planes(pts, dist, 2, min_inliers, H, seed, outliers=spec)
    assert np.array_equal(f.labels.cpu().numpy(), PO.segment(kept.cpu().numpy(), dist, H, 2, min_inliers, seed).labels)
    empty = segment.planes(np.zeros((0, 3), np.float32), dist, 3)
    assert empty.n_planes == 0 and empty.labels.shape == (0,) and empty.planes.shape == (0, 4)


@pytest.mark.parametrize('seed', K.OBJ_SEEDS)
def test_off_planes_then_dbscan_gives_the_oracles_objects(seed):
    """off_planes / on_planes split the view as the oracle's labels do, score is the row's plane's count; cluster.dbscan on what is off the planes
    gives the cluster oracle's labels on the oracle's rest, the three furniture boxes, bit for bit"""
    from roreg_amd import cluster, segment
    pts, dist, H, planes, min_inliers, sd = K.case('objects', seed)
    want = K.reference('objects', seed)
    off = segment.off_planes(pts, dist, planes, min_inliers, H, sd)
    on = segment.on_planes(pts, dist, planes, min_inliers, H, sd)
    rest = np.flatnonzero(want.labels < 0)
    assert np.array_equal(off.rows.cpu().numpy(), rest) and np.array_equal(off.points.cpu().numpy(), pts[rest]) and off.rows.dtype == torch.int64
    assert np.array_equal(off.mask.cpu().numpy(), want.labels < 0) and torch.equal(on.mask, ~off.mask) and np.array_equal(on.rows.cpu().numpy(), np.flatnonzero(want.labels >= 0))
    score = np.where(want.labels >= 0, want.counts[np.maximum(want.labels, 0)], 0).astype(np.float64)
    assert off.score.dtype == torch.float64 and np.array_equal(off.score.cpu().numpy(), score) and torch.equal(on.score, off.score)
    parts = cluster.dbscan(off.points, K.OBJ_EPS, K.OBJ_MIN_POINTS)
    ref = CO.dbscan(pts[rest], K.OBJ_EPS, K.OBJ_MIN_POINTS)
    assert parts.n_clusters == CO.n_clusters(ref) and np.array_equal(parts.labels.cpu().numpy(), ref.labels) and np.array_equal(parts.sizes.cpu().numpy(), ref.sizes[:parts.n_clusters])
    top = np.sort(ref.sizes)[::-1][:3]
    assert top.sum() >= 0.9 * rest.shape[0]


def test_smoke_leg():
    import __graft_entry__ as entry
    assert 'plane' in entry._smoke_planes()
