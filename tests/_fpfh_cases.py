"""Seeded input families of the FPFH tests (tests/test_fpfh_oracle.py checks each family's conditions on the CPU with the oracle alone,
tests/test_hip_fpfh.py runs the same families on the device) and the oracle's result for each, computed once per process.

  terrain   -- two partial views of a height field (a sum of Gaussian bumps: no symmetry, curvature everywhere), the end-to-end family;
  box       -- n seeded points in a box with seeded unit normals, fed directly (independent of the normal estimation), mean m about 30;
  lattice   -- tests/_icp_plane_cases.py lattice_case with seeded normals: neighbours at exactly d2 == r^2 across a cell face and a corner;
  axis      -- isolated pairs built by hand that reach the bins' edges, an exact |a1| == |a2| tie and a pair with no frame;
  duplicate -- a box cloud with duplicated rows (d2 == 0: skipped both ways);
  third / none -- a box cloud with a third of its normals zero, and with all of them zero;
  cluster   -- 2,001 points inside one ball (every m = 2000);
  orient    -- 5,000 axis-aligned points, normals and viewpoint: zero rows and dot products of exactly 0.
No GPU imports."""
import functools

import numpy as np

import _fpfh_oracle as FO
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
import _voxel_oracle as VO
from roreg_amd import synth

# ---- terrain -------------------------------------------------------------------------------------------------------------------------------
TERRAIN_SEEDS = (0, 1, 2, 3)
TERRAIN_N, TERRAIN_VOXEL, TERRAIN_NORMAL_R, TERRAIN_R, TERRAIN_TAU = 40000, 0.05, 0.1, 0.25, 0.1
TERRAIN_DEG, TERRAIN_T = 2.0, 0.05          # the end-to-end bar: about 2.5 x the worst the oracle chain was seen to give (0.76 degrees, 2.8 cm)
# The radius at which the oracle chain counts a hypothesis' inliers when it picks the best one: one voxel.  The count has to resolve the bar it
# is held to: 2 degrees move a point 1 m from the centre of the overlap (which is 1.6 m x 3 m) by 3.5 cm, and the bar on the translation is
# 5 cm, so a radius of 2 voxels = 0.1 counts the same correspondences for a hypothesis at the truth and for one at the edge of the bar.  A
# correct correspondence joins the centroids of two independently sampled voxels, at most about one voxel apart: that is the radius.
TERRAIN_INLIER = TERRAIN_VOXEL


@functools.lru_cache(maxsize=None)
def terrain_pair(seed):
    """-> (points0 float32 [n,3], points1 float32 [n,3], T_gt) with points0 ~ points1 R^T + t on the shared surface.  A height field over
    [-2, 2] x [-1.5, 1.5]: 40 Gaussian bumps, amplitudes U(-0.5, 0.5), widths U(0.15, 0.45), centres uniform; view 0 is 40,000 uniform
    samples with x < 0.8, view 1 independent samples with x > -0.8; noise N(0, 2 mm) per coordinate; view 1 is given in its own frame."""
    rng = np.random.default_rng([int(seed), 0xf9f4])
    amp, wid = rng.uniform(-0.5, 0.5, 40), rng.uniform(0.15, 0.45, 40)
    cen = np.stack([rng.uniform(-2.0, 2.0, 40), rng.uniform(-1.5, 1.5, 40)], 1)

    def view(lo, hi):
        xy = np.stack([rng.uniform(lo, hi, TERRAIN_N), rng.uniform(-1.5, 1.5, TERRAIN_N)], 1)
        d2 = ((xy[:, None, :] - cen[None, :, :]) ** 2).sum(-1)
        z = (amp[None, :] * np.exp(-d2 / (2.0 * wid[None, :] ** 2))).sum(1)
        return np.concatenate([xy, z[:, None]], 1) + rng.normal(0.0, 0.002, (TERRAIN_N, 3))

    v0, v1 = view(-2.0, 0.8), view(-0.8, 2.0)
    T = synth.dense_gt()
    x1 = (v1 - T[:3, 3]) @ T[:3, :3]
    return np.ascontiguousarray(v0, np.float32), np.ascontiguousarray(x1, np.float32), T


@functools.lru_cache(maxsize=None)
def terrain_view(seed, which):
    """One view downsampled at TERRAIN_VOXEL by the voxel oracle, with the normal oracle's table and the cloud's centroid
    -> (points float32 [m,3], normal table f64 [m,4], viewpoint f64 [3])"""
    pts = np.ascontiguousarray(VO.downsample(terrain_pair(seed)[which], TERRAIN_VOXEL).points, np.float32)
    return pts, PO.normals(pts, TERRAIN_NORMAL_R, PC.MIN_NB).table, pts.astype(np.float64).mean(0)


@functools.lru_cache(maxsize=None)
def terrain_reference(seed, which):
    """-> (oriented table, counts, m, features float32, valid) of FO.describe"""
    pts, table, c = terrain_view(seed, which)
    return FO.describe(pts, table, c, TERRAIN_R)


def pose_error(T, Tg):
    """-> (rotation angle between them in degrees, distance of the translations)"""
    dR = T[:3, :3] @ Tg[:3, :3].T
    s = np.sqrt(((dR - dR.T) ** 2).sum() / 8.0)                 # sin of the angle, well conditioned where it is small
    c = (np.trace(dR) - 1.0) / 2.0
    return float(np.degrees(np.arctan2(s, c))), float(np.sqrt(((T[:3, 3] - Tg[:3, 3]) ** 2).sum()))


# ---- box -----------------------------------------------------------------------------------------------------------------------------------
BOX_N = (1, 2, 5, 63, 64, 65, 255, 256, 257, 1025)
BOX_R = 0.1


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(1))[:, None]


@functools.lru_cache(maxsize=None)
def box_case(n):
    """-> (points float32 [n,3], unit normals f64 [n,4] with a zero last column): the box's side gives an interior point 45 neighbours
    within BOX_R, the faces bring the mean to about 30 (small n: every other point)."""
    rng = np.random.default_rng([int(n), 0xb0c5])
    side = BOX_R * (4.18879 * n / 45.0) ** (1.0 / 3.0)
    pts = (rng.uniform(0.0, side, (n, 3)) + np.array([0.3, -0.7, 1.1])).astype(np.float32)
    return pts, np.concatenate([unit_normals(rng, n), np.zeros((n, 1))], 1)


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    """(points, oriented normal table, radius) of a named case -> (counts, m, features float32, valid, float64 features)"""
    pts, nrm, r = case(name, arg)
    counts, m = FO.spfh(pts, nrm, r)
    F, valid, F64 = FO.fpfh(pts, counts, m, r)
    return counts, m, F, valid, F64


# ---- lattice ---------------------------------------------------------------------------------------------------------------------------------
def lattice_case(base):
    pts = PC.lattice_case(base)[0]
    rng = np.random.default_rng([int(abs(base)), 0x1a77])
    return pts, np.concatenate([unit_normals(rng, pts.shape[0]), np.zeros((pts.shape[0], 1))], 1)


# ---- axis: isolated pairs, 8 apart along x ---------------------------------------------------------------------------------------------------
AXIS_R = 1.5
EX, EY, EZ = np.eye(3)
AXIS_PAIRS = (                                                   # (name, n_i, x_j - x_i, n_j)
    ('f2_plus_one_xy_zero_tie', EZ, EX, -EY),                    # a1 = a2 = 0 (tie: no swap); f2 = +1 (clamped to bin 10); x = y = 0 (bin 5)
    ('f2_minus_one', EZ, EX, EY),                                # f2 = -1 (bin 0)
    ('y_zero_x_negative', EZ, EX, -EZ),                          # y = 0, x = -1: the angle is pi (bin 10)
    ('tie_nonzero', EZ, EX + EZ, EX),                            # a1 = a2 = 1 / sqrt(2), the same operations: no swap
    ('no_frame', EX, EX, EY),                                    # dp parallel to na from either end: skipped both ways
    ('swap', EZ, EX, (EX + EZ) / np.sqrt(2.0)),                  # |a1| = 0 < |a2|: the frame moves to j
)


def axis_case():
    pts, nrm = [], []
    for p, (_, ni, dp, nj) in enumerate(AXIS_PAIRS):
        base = np.array([8.0 * p, 0.0, 0.0])
        pts += [base, base + dp]; nrm += [ni, nj]
    return np.float32(pts), np.concatenate([np.float64(nrm), np.zeros((len(nrm), 1))], 1)


# ---- duplicate, third, none, cluster -------------------------------------------------------------------------------------------------------
def duplicate_case():
    pts, nrm = (v.copy() for v in box_case(257))
    pts[10:40] = pts[200:230]                                    # thirty duplicated rows, each with its own normal
    return pts, nrm


def third_case():
    pts, nrm = (v.copy() for v in box_case(1025))
    nrm[::3] = 0.0
    return pts, nrm


def none_case():
    pts, nrm = box_case(257)
    return pts, np.zeros_like(nrm)


CLUSTER_N, CLUSTER_R = 2001, 0.1


def cluster_case():
    """2,001 points in a cube of side 0.05 (its diagonal is shorter than the radius): every point is every other point's neighbour"""
    rng = np.random.default_rng(0xc1a5)
    pts = (rng.uniform(0.0, 0.05, (CLUSTER_N, 3)) + np.array([-0.4, 0.2, 0.9])).astype(np.float32)
    return pts, np.concatenate([unit_normals(rng, CLUSTER_N), np.zeros((CLUSTER_N, 1))], 1)


def case(name, arg=None):
    """-> (points float32, oriented normal table f64 [n,4], radius)"""
    if name == 'box':
        return box_case(arg) + (BOX_R,)
    if name == 'lattice':
        return lattice_case(arg) + (PC.LAT_R,)
    if name == 'terrain':
        pts, _, _ = terrain_view(0, 0)
        return pts, terrain_reference(0, 0)[0], TERRAIN_R
    return dict(axis=axis_case, duplicate=duplicate_case, third=third_case, none=none_case, cluster=cluster_case)[name]() + (
        dict(axis=AXIS_R, cluster=CLUSTER_R).get(name, BOX_R),)


CASES = ([('box', n) for n in BOX_N] + [('terrain', None)] + [('lattice', b) for b in PC.LAT_BASES]
         + [('axis', None), ('duplicate', None), ('third', None), ('none', None), ('cluster', None)])


def case_id(c):
    return c[0] if c[1] is None else f'{c[0]}-{c[1]}'


# ---- orient --------------------------------------------------------------------------------------------------------------------------------
ORIENT_N, ORIENT_VIEWPOINT = 5000, (1.0, -2.0, 0.0)


@functools.lru_cache(maxsize=None)
def orient_case():
    """-> (points float32 [n,3] with integer coordinates in [-4, 4], normal table f64 [n,4]: +-axis or zero, column 3 a row count)"""
    rng = np.random.default_rng(0x0e17)
    pts = rng.integers(-4, 5, (ORIENT_N, 3)).astype(np.float32)
    kind = rng.integers(0, 7, ORIENT_N)                          # 0..5: +-e_a, 6: the zero row
    nrm = np.zeros((ORIENT_N, 4))
    rows = np.nonzero(kind < 6)[0]
    nrm[rows, kind[rows] // 2] = np.where(kind[rows] % 2 == 0, 1.0, -1.0)
    nrm[:, 3] = np.arange(ORIENT_N) % 17
    return pts, nrm
