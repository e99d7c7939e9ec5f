"""Registration of raw scans with no checkpoint: FPFH descriptors (Rusu et al., 2009) on the device (csrc/fpfh.hip; no
reference counterpart: the reference's descriptors are learned), matched by mutual nearest neighbours and handed to the spatial-compatibility
estimator (roreg_amd/sc2.py) and, optionally, to dense ICP (roreg_amd/icp.py).

    from roreg_amd import fpfh
    d = fpfh.describe(points, radius=0.25, voxel=0.05)             # -> FpfhCloud: points, normals, features [n,33], valid (device tensors)
    m = fpfh.match(d0, d1)                                         # -> int64 [M,2] device tensor: rows of d0.points, rows of d1.points
    m = fpfh.match(d0, d1, method='mfma')                          # the same bytes from the matrix cores ('scan': the literal search; 'auto': by size)
    res = fpfh.register(points0, points1, voxel=0.05)              # -> FpfhRegistration; res.trans [4,4]: points0 ~ points1 R^T + t
    res = fpfh.register(points0, points1, voxel=0.05, icp=dict(method='plane', max_dist=0.1))      # ... then refined: res.trans_icp
    out = fpfh.register_scene(clouds, [(0, 1), (1, 2)], voxel=0.05)    # every cloud described once, all pairs estimated in the same launches
    res = fpfh.register(points0, points1, voxel=0.05, keypoints=5000)  # only 5000 farthest-point samples per cloud (roreg_amd/sample.py) are matched

Coordinates are rounded to float32 once, at upload; the descriptor's arithmetic is float64.  A scene that looks the same from two poses under
local geometry (a box room turned by 180 degrees) is registered to either: the descriptor cannot tell them apart."""
from collections import namedtuple

import torch

from . import hip
from . import icp as dense_icp
from . import outliers as outlier_filter
from . import sample
from . import sc2
from . import voxel as voxel_grid

FpfhCloud = namedtuple('FpfhCloud', 'points normals features valid')
FpfhCloud.__doc__ = ('device tensors: points float32 [n,3] (the cloud, downsampled where voxel= asked for it), normals float64 [n,4] = the oriented unit '
                     'normal (zero where the neighbourhood gives none) and the size of its neighbourhood, features float32 [n,33], valid uint8 [n] '
                     '(a row with no valid normal or no neighbour with one is invalid and zero)')
FpfhRegistration = namedtuple('FpfhRegistration', 'trans matches sc2 trans_icp icp')
FpfhRegistration.__doc__ = ('trans [4,4] float64 (the estimator\'s: points0 ~ points1 R^T + t); matches int64 [M,2] on the host (rows of the downsampled '
                            'clouds); sc2: the Sc2Result; trans_icp, icp: the refined transform and the IcpResult, None unless icp= was given')
NORMAL_RADIUS_RATIO = 2.5


def describe(points, radius, normal_radius=None, voxel=None, viewpoint=None, min_neighbors=6, device='cuda', outliers=None):
    """A cloud [n,3] (host array or tensor) -> FpfhCloud.  normal_radius: the ball the normals are estimated from (default radius / 2.5);
    viewpoint: the point every normal is turned towards (default: the cloud's centroid, which moves with the cloud under a rigid motion, so
    two scans orient a shared surface alike when it lies on the same side of both centroids; reading it back is the one synchronisation).
    One grid, built for `radius`, serves the normals and both passes.  outliers=dict(kind='statistical' | 'radius' | 'cluster', ...) (roreg_amd.outliers):
    the cloud is filtered after voxel=, before the grid is built; FpfhCloud.points are the kept points."""
    radius = float(radius)
    outliers = outlier_filter.check_args(outliers, 'fpfh.describe')
    normal_radius = radius / NORMAL_RADIUS_RATIO if normal_radius is None else float(normal_radius)
    pts = dense_icp.device_points(points, device)
    if voxel is not None:
        pts = voxel_grid.device_downsample(pts, voxel)[0]
    pts = outlier_filter.device_apply(pts, outliers)[0]
    if int(pts.shape[0]) == 0:
        return FpfhCloud(pts, torch.zeros((0, 4), dtype=torch.float64, device=pts.device), torch.zeros((0, hip.FPFH_WIDTH), dtype=torch.float32, device=pts.device),
                         torch.zeros(0, dtype=torch.uint8, device=pts.device))
    grid = hip.IcpGrid(pts, radius)
    table = hip.icp_normals(grid, normal_radius, min_neighbors)
    if viewpoint is None:
        viewpoint = pts.double().mean(0).cpu().numpy()
    oriented = hip.fpfh_orient(grid, table, viewpoint)
    counts, m = hip.fpfh_spfh(grid, oriented, radius)
    features, valid = hip.fpfh_features(grid, counts, m, radius)
    return FpfhCloud(pts, oriented, features, valid)


# method='auto': the matrix-core matcher (hip.fpfh_match) where the two sides' lengths multiply to at least this, the literal scan below it.  Both
# give the same bytes.  tools/time_fpfh.py --match found no crossover (profiles/fpfh_match_timing.txt): the matcher was the faster at every side
# length measured, 64 x 64 (0.23 ms against 0.46 ms) to 130,581 x 92,916; below 64 x 64 nothing was measured and the scan stays.
MATCH_MFMA_MIN_PRODUCT = 64 * 64


def _valid_rows(desc, rows=None):
    """the valid rows of desc in increasing order; rows (an integer device tensor, any order; entries that are no row of the cloud, such as
    the -1 behind a sample's count, are dropped): those of them that are valid"""
    if rows is None:
        return desc.valid.nonzero().reshape(-1).contiguous()
    n = int(desc.valid.shape[0])
    rows = rows.reshape(-1).long()
    given = torch.zeros(n, dtype=torch.bool, device=desc.valid.device)
    given[rows[(rows >= 0) & (rows < n)]] = True
    return (given & desc.valid.bool()).nonzero().reshape(-1).contiguous()


def _cut(m, rows0, dist, n0, max_matches):
    """at most max_matches rows of m, those of the least descriptor distance (ties to the lower row), in increasing row of side 0"""
    if max_matches is not None and int(m.shape[0]) > int(max_matches):
        d = torch.full((n0,), float('inf'), dtype=torch.float32, device=dist.device)
        d[rows0] = dist
        keep = torch.sort(d[m[:, 0]], stable=True)[1][:int(max_matches)]
        m = m[torch.sort(keep)[0]]
    return m.contiguous()


def match(desc0, desc1, max_matches=None, method='auto', rows0=None, rows1=None):
    """Mutual nearest neighbours of the valid rows of two FpfhClouds -> int64 [M,2] device tensor (row of desc0.points, row of desc1.points),
    in increasing row of desc0.  max_matches: keep at most that many, those of the least descriptor distance (ties to the lower row).
    rows0 / rows1: int64 device tensors of rows in any order (keypoints; a sample's rows); only those of them that are valid take part, on
    that side, and the search on the other side sees only them.
    method: 'scan' = two literal searches (hip.nn_search) and hip.mutual_matches; 'mfma' = hip.fpfh_match, the same bytes from the matrix
    cores; 'auto' = by size."""
    if method not in ('auto', 'mfma', 'scan'):
        raise ValueError(f"fpfh.match: method must be 'auto', 'mfma' or 'scan', got {method!r}")
    rows0, rows1 = _valid_rows(desc0, rows0), _valid_rows(desc1, rows1)
    if int(rows0.shape[0]) == 0 or int(rows1.shape[0]) == 0:
        return torch.zeros((0, 2), dtype=torch.int64, device=desc0.points.device)
    if method == 'auto':
        method = 'mfma' if int(rows0.shape[0]) * int(rows1.shape[0]) >= MATCH_MFMA_MIN_PRODUCT else 'scan'
    if method == 'mfma':
        out, count, _, dist, _ = hip.fpfh_match(desc0.features, desc1.features, rows0, rows1)
    else:
        nn01, dist = hip.nn_search(desc0.features, desc1.features, src_rows=rows0, tgt_rows=rows1, want_dist=True)
        nn10 = hip.nn_search(desc1.features, desc0.features, src_rows=rows1, tgt_rows=rows0)
        out, count = hip.mutual_matches(nn01, nn10, sample0=rows0, sample1=rows1)
    return _cut(out[:int(count.item())], rows0, dist, int(desc0.points.shape[0]), max_matches)


def match_pairs(descs, pairs, max_matches=None, rows=None):
    """match(descs[i], descs[j], max_matches, rows0=rows[i], rows1=rows[j]) of every (i, j), all pairs in one hip.fpfh_match_batch call ->
    [int64 [M,2] device tensors].  rows: None, or per cloud None / the rows of it that take part."""
    rows = {k: _valid_rows(descs[k], None if rows is None else rows[k]) for k in sorted({k for p in pairs for k in p})}
    res = hip.fpfh_match_batch([(descs[i].features, descs[j].features, rows[i], rows[j]) for i, j in pairs])
    counts = [int(c) for c in torch.cat([r[1] for r in res]).cpu()] if pairs else []
    return [_cut(r[0][:c], rows[i], r[3], int(descs[i].points.shape[0]), max_matches) for (i, j), r, c in zip(pairs, res, counts)]


def _args(voxel, radius, ird):
    v = voxel_grid.check_args(voxel, what='fpfh.register')
    return v, 5.0 * v if radius is None else float(radius), 2.0 * v if ird is None else float(ird)


def _keypoint_args(keypoints, what):
    """keypoints= of register / register_scene -> None, or dict(k, start, min_dist); ValueError otherwise (no device call)."""
    if keypoints is None:
        return None
    kw = dict(keypoints) if isinstance(keypoints, dict) else dict(k=keypoints)
    extra = set(kw) - {'k', 'start', 'min_dist'}
    if extra:
        raise ValueError(f'{what}: keypoints takes no {sorted(extra)}')
    kw = dict(k=kw.get('k'), start=kw.get('start', 0), min_dist=kw.get('min_dist'))
    sample.check_args(kw['k'], kw['start'], kw['min_dist'], what)
    return kw


def _keypoint_rows(descs, kp):
    """the farthest-point sample of every described cloud, all in one launch -> [int32 rows, -1 behind the sample's count] (or Nones)"""
    if kp is None:
        return [None] * len(descs)
    return [r[0] for r in sample.device_farthest([d.points for d in descs], kp['k'], kp['start'], kp['min_dist'])]


def _result(m, res, refined):
    return FpfhRegistration(res.T, m.cpu().numpy(), res, None if refined is None else refined.T, refined)


def register(points0, points1, voxel, radius=None, ird=None, icp=None, match_method='auto', outliers=None, keypoints=None, **sc2_kw):
    """Two raw clouds -> FpfhRegistration: both downsampled at `voxel` and described (radius: default 5 voxel), matched, and the pose estimated
    from the matched points by sc2.register (ird: its inlier distance, default 2 voxel; sc2_kw: its other arguments).  icp=dict(...): the
    arguments of icp.refine (max_dist at least), which then refines the estimate on the downsampled clouds.  match_method: match's method.  outliers: describe's, for both clouds
    (the refinement then runs on the kept points).  keypoints=K or dict(k=K, min_dist=r, start=s): every row is still described (a
    descriptor needs its neighbours' histograms), but only a farthest-point sample of each described cloud (sample.device_farthest) is
    matched: K rows that cover the cloud evenly, and a matcher that costs K^2 instead of n0 n1."""
    voxel, radius, ird = _args(voxel, radius, ird)
    kp = _keypoint_args(keypoints, 'fpfh.register')
    d0, d1 = describe(points0, radius, voxel=voxel, outliers=outliers), describe(points1, radius, voxel=voxel, outliers=outliers)
    r0, r1 = _keypoint_rows([d0, d1], kp)
    m = match(d0, d1, hip.SC2_MAX_M, method=match_method, rows0=r0, rows1=r1)
    res = sc2.register(d0.points, d1.points, m, None, ird=ird, **sc2_kw)
    refined = None if icp is None else dense_icp.refine(d0.points, d1.points, res.T, **icp)
    return _result(m, res, refined)


def register_scene(clouds, pairs, voxel, radius=None, ird=None, icp=None, match_method='auto', outliers=None, keypoints=None, **sc2_kw):
    """clouds: a list of raw clouds; pairs: [(i, j)] -> [FpfhRegistration], trans mapping cloud j into cloud i.  Every cloud is downsampled
    and described once; all pairs go through the matcher's batch form (match_pairs; match_method='scan': through match, pair by pair, the same
    bytes), through sc2.register's list form and through icp.refine's, in one call each.  outliers: describe's, for every cloud.  keypoints: register's; all clouds are sampled in one launch."""
    voxel, radius, ird = _args(voxel, radius, ird)
    kp = _keypoint_args(keypoints, 'fpfh.register_scene')
    descs = [describe(c, radius, voxel=voxel, outliers=outliers) for c in clouds]
    rows = _keypoint_rows(descs, kp)
    if match_method == 'scan':
        matches = [match(descs[i], descs[j], hip.SC2_MAX_M, method='scan', rows0=rows[i], rows1=rows[j]) for i, j in pairs]
    else:
        matches = match_pairs(descs, [tuple(p) for p in pairs], hip.SC2_MAX_M, rows)
    if not pairs:
        return []
    results = sc2.register([(descs[i].points, descs[j].points, m, None) for (i, j), m in zip(pairs, matches)], ird=ird, **sc2_kw)
    refined = [None] * len(pairs)
    if icp is not None:
        refined = dense_icp.refine([(descs[i].points, descs[j].points, r.T) for (i, j), r in zip(pairs, results)], **icp)
    return [_result(m, r, f) for m, r, f in zip(matches, results, refined)]
