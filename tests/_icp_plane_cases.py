"""Seeded input families of the point-to-plane ICP tests (tests/test_icp_plane_oracle.py checks each family's conditions on the CPU with the
oracle alone, tests/test_hip_icp_plane.py runs the same families on the device) and the oracle's result for each, computed once per process.

  dense     -- a 30,000-point room scan with sixty duplicated rows: the neighbourhood counts and the normals of a real surface mix;
  lattice   -- points on a dyadic lattice with neighbours at exactly d2 == r^2 across a cell face ((3, 0, 0) / 16) and across a cell corner
               ((1, 2, 2) / 16 and its permutations, 1 + 4 + 4 = 9), and the same neighbours one float32 step beyond;
  small     -- clouds of 1 .. 257 points, fifty copies of one point, exactly collinear points, exactly coplanar lattice points;
  tie       -- the one-iteration pair of tests/test_hip_icp.py (1000 duplicated target rows: exact ties for every query near them);
  conv      -- the convergence pair of tests/_icp_oracle.py: normal radius 0.2 (converges) and 0.1 from the first start (the two-set cycle);
  rank      -- targets on one, two and three exact axis-aligned planes (A of rank 3, 5, 6) and the noisy wall of tests/_icp_cases.py;
  chunk     -- source counts at the slot boundaries against a whole target.
No GPU imports."""
import functools

import numpy as np

import _icp_cases as C
import _icp_oracle as O
import _icp_plane_oracle as PO
from roreg_amd import synth

MIN_NB = 6

# ---- dense ---------------------------------------------------------------------------------------------------------------------------------
DENSE_R = 0.1


@functools.lru_cache(maxsize=None)
def dense_cloud():
    p0 = synth.make_dense_pair(8, 30000)[0]
    p0[200:260] = p0[7000:7060]                                 # duplicated rows: d2 == 0 neighbours, each counted
    return p0


@functools.lru_cache(maxsize=None)
def dense_reference():
    return PO.normals(dense_cloud(), DENSE_R, MIN_NB)


# ---- lattice -------------------------------------------------------------------------------------------------------------------------------
LAT_R = 0.1875                                                  # 3 / 16: (3, 0, 0) / 16 and (1, 2, 2) / 16 are both at exactly r
LAT_BASES = (0.0, -3.0, 1024.0)
LAT_GRID_DISTS = (LAT_R, 2 * LAT_R, LAT_R / 2)                  # the radius the grid is built for; the normals are always for LAT_R
KIND_CENTRE, KIND_FACE, KIND_FACE_BEYOND, KIND_CORNER, KIND_CORNER_BEYOND = 0, 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def lattice_case(base):
    """-> (points float32 [n,3], kind int [n], centre int [n]: the row of the point's lattice centre).  27 centres 1.5 apart; around each:
    6 face neighbours at exactly r, the same 6 one float32 step of the coordinate beyond, 24 corner neighbours at exactly r and the same
    24 with their longest offset one step beyond.  Every coordinate is a multiple of 1 / 16 or one float32 step off it: every d2 is exact."""
    b = np.float32(base)
    k = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing='ij'), -1).reshape(-1, 3)
    cen = (b + np.float32(1.5) * k.astype(np.float32)).astype(np.float32)
    pts, kind, owner = [c for c in cen], [KIND_CENTRE] * 27, list(range(27))
    for i, c in enumerate(cen):
        for ax in range(3):
            for sg in (-1.0, 1.0):
                x = c.copy(); x[ax] = np.float32(c[ax] + np.float32(sg * LAT_R))
                pts.append(x); kind.append(KIND_FACE); owner.append(i)
                y = x.copy(); y[ax] = np.nextafter(x[ax], np.float32(sg * np.inf))
                pts.append(y); kind.append(KIND_FACE_BEYOND); owner.append(i)
        for ax in range(3):                                     # the axis of the short offset
            for sx in (-1, 1):
                for sy in (-1, 1):
                    for sz in (-1, 1):
                        o = np.float32([2, 2, 2]) / np.float32(16); o[ax] = np.float32(1.0 / 16)
                        o = o * np.float32([sx, sy, sz])
                        x = (c + o).astype(np.float32)
                        pts.append(x); kind.append(KIND_CORNER); owner.append(i)
                        l = (ax + 1) % 3
                        y = x.copy(); y[l] = np.nextafter(x[l], np.float32(np.sign(o[l]) * np.inf))
                        pts.append(y); kind.append(KIND_CORNER_BEYOND); owner.append(i)
    return np.stack(pts).astype(np.float32), np.array(kind), np.array(owner)


@functools.lru_cache(maxsize=None)
def lattice_reference(base):
    return PO.normals_full(lattice_case(base)[0], LAT_R, MIN_NB)


# ---- small ---------------------------------------------------------------------------------------------------------------------------------
SMALL_R = 0.1
SMALL_N = (1, 5, 6, 63, 64, 65, 257)


@functools.lru_cache(maxsize=None)
def small_cloud(n):
    """n points of a noisy patch of a tilted plane, 0.25 m across (several cells at r = 0.1), thickness 2 mm."""
    rng = np.random.default_rng([int(n), 0x51a])
    x = np.concatenate([rng.uniform(0, 0.25, (n, 2)), rng.normal(0, 0.002, (n, 1))], 1)
    return (x @ synth.dense_gt(33.0, (2.0, -1.0, 0.5), (0, 0, 0))[:3, :3].T + np.array([0.3, -0.2, 0.7])).astype(np.float32)


def copies_cloud():
    return np.tile(np.float32([[0.3, -1.2, 0.8]]), (50, 1))


def collinear_cloud():
    """Fifty points k (1, 2, -1) / 256: exactly collinear (dyadic), 0.0096 apart."""
    return (np.arange(50, dtype=np.float32)[:, None] * np.float32([1, 2, -1]) / np.float32(256)).astype(np.float32)


def coplanar_clouds():
    """-> [(points float32, unit normal float64)]: a 12 x 12 lattice of spacing 1 / 32 in the plane z = 0.5, and one in the plane
    x + y - z = 0 (points (i, j, i + j) / 32: every offset dyadic, every product exact)."""
    i, j = (v.reshape(-1).astype(np.float32) for v in np.meshgrid(np.arange(12), np.arange(12), indexing='ij'))
    flat = np.stack([i / 32, j / 32, np.full_like(i, 0.5)], 1).astype(np.float32)
    tilt = np.stack([i / 32, j / 32, (i + j) / 32], 1).astype(np.float32)
    return [(flat, np.array([0.0, 0.0, 1.0])), (tilt, np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0))]


# ---- tie: one iteration from a given transform --------------------------------------------------------------------------------------------
TIE_DISTS = (0.05, 0.1)


@functools.lru_cache(maxsize=None)
def tie_pair():
    p0, p1, Tg = synth.make_dense_pair(5, 20000)
    p0[100:1100] = p0[5000:6000]
    return p0, p1, O.perturb(Tg, 1.0, 0.02, 5)


@functools.lru_cache(maxsize=None)
def tie_normals(d):
    return PO.normals(tie_pair()[0], 2 * d, MIN_NB)


@functools.lru_cache(maxsize=None)
def tie_reference(d):
    p0, p1, T0 = tie_pair()
    return PO.iterate(PO.widen(p0), PO.widen(p1), tie_normals(d).table, T0[:3, :3], T0[:3, 3], d)


# ---- conv ----------------------------------------------------------------------------------------------------------------------------------
CONV_DIST, CONV_RADIUS, CYCLE_RADIUS, CONV_ITER, CYCLE_ITER = 0.1, 0.2, 0.1, 50, 30


@functools.lru_cache(maxsize=None)
def conv_pair():
    return synth.make_dense_pair(O.CONV_SEED, O.CONV_N)


def conv_starts():
    Tg = conv_pair()[2]
    return [O.perturb(Tg, deg, shift, O.CONV_SEED) for deg, shift in O.CONV_STARTS]


@functools.lru_cache(maxsize=None)
def conv_normals(radius):
    return PO.normals(conv_pair()[0], radius, MIN_NB)


@functools.lru_cache(maxsize=None)
def conv_reference(start, radius, max_iter):
    """-> (PO.Result, trace)"""
    p0, p1, _ = conv_pair()
    trace = []
    return PO.icp(p0, p1, conv_normals(radius).table, conv_starts()[start], CONV_DIST, max_iter=max_iter, trace=trace), trace


@functools.lru_cache(maxsize=None)
def conv_point_reference(start):
    p0, p1, _ = conv_pair()
    return O.icp(p0, p1, conv_starts()[start], CONV_DIST, max_iter=CONV_ITER)


# ---- rank ----------------------------------------------------------------------------------------------------------------------------------
RANK_DIST, RANK_RADIUS, RANK_ITER = 0.1, 0.2, 20
RANK_PLANES = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def planes_pair(n_planes):
    """Targets on n exact axis-aligned planes: patches [0.4, 1.4]^2 of z = 0, x = 0 and y = 0, 0.4 from the edges where the planes meet, so
    that no ball of RANK_RADIUS holds points of two patches and every normal is an exact axis.  1500 points per patch, the source is every
    other target point moved by the inverse of T_gt plus 1 mm of noise -> (target f32, source f32, T_gt, T0)."""
    rng = np.random.default_rng([int(n_planes), 0x9a7e])
    patches = []
    for ax in (2, 0, 1)[:n_planes]:
        x = rng.uniform(0.4, 1.4, (1500, 3)).astype(np.float32)
        x[:, ax] = 0.0
        patches.append(x)
    tgt = np.concatenate(patches).astype(np.float32)
    Tg = O.perturb(np.eye(4), 3.0, 0.04, 17 + n_planes)
    src = ((tgt[::2].astype(np.float64) + rng.normal(0, 0.001, (tgt[::2].shape[0], 3)) - Tg[:3, 3]) @ Tg[:3, :3]).astype(np.float32)
    return tgt, src, Tg, O.perturb(Tg, 1.0, 0.02, 23 + n_planes)


@functools.lru_cache(maxsize=None)
def planes_normals(n_planes):
    return PO.normals(planes_pair(n_planes)[0], RANK_RADIUS, MIN_NB)


@functools.lru_cache(maxsize=None)
def planes_reference(n_planes):
    tgt, src, _, T0 = planes_pair(n_planes)
    trace = []
    return PO.icp(tgt, src, planes_normals(n_planes).table, T0, RANK_DIST, max_iter=RANK_ITER, trace=trace), trace


WALL_SEEDS = C.WALL_SEEDS


@functools.lru_cache(maxsize=None)
def wall_normals(seed):
    return PO.normals(C.wall_pair(seed)[0], RANK_RADIUS, MIN_NB)


@functools.lru_cache(maxsize=None)
def wall_reference(seed):
    q, p, _, T0 = C.wall_pair(seed)
    trace = []
    return PO.icp(q, p, wall_normals(seed).table, T0, C.WALL_DIST, max_iter=C.WALL_ITER, trace=trace), trace


# ---- chunk ---------------------------------------------------------------------------------------------------------------------------------
CHUNK_SRC_N = (1, 1023, 1024, 1025, 3073)
CHUNK_RADIUS = 0.2


@functools.lru_cache(maxsize=None)
def chunk_pairs():
    """-> [(name, target float32, source float32, T0)] with the target, the source rows and T0 of tests/_icp_cases.py chunk_pairs"""
    return [c for c in C.chunk_pairs() if c[0] in {f'src{n}' for n in CHUNK_SRC_N}]


@functools.lru_cache(maxsize=None)
def chunk_normals():
    return PO.normals(chunk_pairs()[0][1], CHUNK_RADIUS, MIN_NB)


@functools.lru_cache(maxsize=None)
def chunk_reference():
    """One iteration (its sums are what the chunking decides) and the full run, per pair -> [(PO.iterate dict, PO.Result)]"""
    N = chunk_normals().table
    out = []
    for _, q, p, T0 in chunk_pairs():
        out.append((PO.iterate(PO.widen(q), PO.widen(p), N, T0[:3, :3], T0[:3, 3], C.CHUNK_DIST), PO.icp(q, p, N, T0, C.CHUNK_DIST, max_iter=C.CHUNK_ITER)))
    return out
