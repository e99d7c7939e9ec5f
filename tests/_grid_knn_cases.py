"""Seeded input families of the grid k-nearest-neighbour and outlier-removal tests (tests/test_grid_knn_oracle.py checks each family's conditions
on the CPU with the oracle alone, tests/test_hip_grid_knn.py runs the same families on the device) and the oracle's result for each, computed
once per process.

  box       -- tests/_fpfh_cases.py box_case: n seeded points in a box, the mean ball of BOX_R holds about 30 (rows short of k and rows beyond it);
  lattice   -- tests/_icp_plane_cases.py lattice_case: neighbours at exactly d2 == r^2 across a cell face and a corner, lists full of exact ties;
  duplicate -- a box cloud with duplicated rows (d2 == 0 entries listed, the own row not);
  cluster   -- 2,001 points inside one ball;
  ray       -- 300 collinear points stored by descending and by ascending coordinate: for the end queries every candidate arrives better than
               the whole list in one and worse in the other (insert at the front / reject);
  foreign   -- queries inside the cloud, outside the grid's box on every side and far away, and a subset of own rows through self_rows;
  terrain   -- tests/_fpfh_cases.py terrain_view(0, 0), k = 16, r = 0.25;
  outlier   -- terrain_view(seed, 0) with n // 20 points injected into its bounding box: the statistical filter's family.
No GPU imports."""
import functools

import numpy as np

import _fpfh_cases as FK
import _grid_knn_oracle as KO
import _icp_plane_cases as PC

KS = (1, 8, 20, 32)

# ---- box, lattice, duplicate, cluster, terrain: (points float32, radius) ---------------------------------------------------------------------
BOX_N, BOX_R = FK.BOX_N, FK.BOX_R
LAT_R, LAT_BASES, LAT_GRID_DISTS = PC.LAT_R, PC.LAT_BASES, PC.LAT_GRID_DISTS
TERRAIN_K, TERRAIN_R = 16, 0.25
RAY_N, RAY_R = 300, 0.5


def ray_case(descending):
    """300 points k (2, 1, -2) / 256, k = 0 .. 299 (dyadic: every d2 exact, 3 / 256 apart), stored by descending or ascending k.  The grid's cells
    are walked in ascending cell, so the candidates of the query at the low end arrive nearest first (every later one is rejected once the list
    is full) and those of the query at the high end farthest first (every later one goes to the front)."""
    kk = np.arange(RAY_N, dtype=np.float32)
    if descending:
        kk = kk[::-1]
    return (kk[:, None] * np.float32([2, 1, -2]) / np.float32(256)).astype(np.float32)


def case(name, arg=None):
    """-> (points float32 [n,3], radius)"""
    if name == 'box':
        return FK.box_case(arg)[0], BOX_R
    if name == 'lattice':
        return PC.lattice_case(arg)[0], LAT_R
    if name == 'duplicate':
        return FK.duplicate_case()[0], BOX_R
    if name == 'cluster':
        return FK.cluster_case()[0], FK.CLUSTER_R
    if name == 'ray':
        return ray_case(arg == 'descending'), RAY_R
    if name == 'terrain':
        return FK.terrain_view(0, 0)[0], TERRAIN_R
    raise KeyError(name)


CASES = ([('box', n) for n in BOX_N] + [('lattice', b) for b in LAT_BASES] + [('duplicate', None), ('cluster', None), ('ray', 'descending'), ('ray', 'ascending'),
                                                                             ('terrain', None)])


def case_ks(c):
    """the list lengths a case runs at"""
    return tuple(sorted(set(KS + (TERRAIN_K,)))) if c[0] == 'terrain' else KS


def case_id(c):
    return c[0] if c[1] is None else f'{c[0]}-{c[1]}'


def shorten(ref, k):
    """The oracle's answer at list length k from its answer at a longer one: the first k entries, the same count, the mean of the shorter list
    (the definition orders the candidates before it cuts the list, so this IS the definition)."""
    d2 = np.ascontiguousarray(ref.d2[:, :k])
    return KO.Knn(np.ascontiguousarray(ref.idx[:, :k]), d2, ref.count, KO._mean(d2, np.minimum(ref.count, k)))


@functools.lru_cache(maxsize=None)
def _reference32(name, arg):
    pts, r = case(name, arg)
    return KO.knn(pts, 32, r)


@functools.lru_cache(maxsize=None)
def reference(name, arg, k):
    return shorten(_reference32(name, arg), k)


# ---- foreign queries -------------------------------------------------------------------------------------------------------------------------
FOREIGN_N, FOREIGN_R = 1025, 0.1


@functools.lru_cache(maxsize=None)
def foreign_case():
    """-> (cloud float32 [1025,3] (the box case), queries float32 [m,3], kind int [m]): 0 = inside the cloud's box, 1 = just outside it on one of
    its six sides (within the radius of the face), 2 = far away (several box sizes off, in every octant)."""
    pts = FK.box_case(FOREIGN_N)[0]
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    rng = np.random.default_rng(0xf02e)
    inside = rng.uniform(lo, hi, (200, 3))
    near = []
    for ax in range(3):
        for side in (0, 1):
            q = rng.uniform(lo, hi, (20, 3))
            q[:, ax] = (lo[ax] - rng.uniform(0.0, 0.05, 20)) if side == 0 else (hi[ax] + rng.uniform(0.0, 0.05, 20))
            near.append(q)
    ext = hi - lo
    far = np.stack([(lo + hi) / 2 + 5.0 * ext * np.array(s) for s in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1), (3, 0, 0), (0, -3, 0), (0, 0, 3))])
    q = np.concatenate([inside] + near + [far]).astype(np.float32)
    kind = np.concatenate([np.zeros(200, int), np.ones(120, int), np.full(far.shape[0], 2)])
    return pts, q, kind


@functools.lru_cache(maxsize=None)
def foreign_reference(k):
    pts, q, _ = foreign_case()
    return shorten(KO.knn(pts, 32, FOREIGN_R, q), k)


def subset_rows(n):
    """the own rows asked again through queries / self_rows: every seventh, the first and the last"""
    return np.unique(np.concatenate([np.arange(0, n, 7), [0, n - 1]])).astype(np.int32)


# ---- outlier family --------------------------------------------------------------------------------------------------------------------------
OUT_SEEDS = (0, 1, 2)
OUT_NB, OUT_STD = 16, 1.0
OUT_FAR = 0.15                         # an injected point farther than this from every surface sample is one the filter has to remove
OUT_START_RADIUS = None                # the starting radius the tests pass to neighbors.knn (None: its own choice from the density)


@functools.lru_cache(maxsize=None)
def outlier_cloud(seed):
    """-> (points float32 [n + n // 20, 3], n): the surface rows first, then the injected ones"""
    pts = FK.terrain_view(seed, 0)[0]
    n = pts.shape[0]
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    rng = np.random.default_rng([int(seed), 0x50f])
    x = rng.uniform(lo[0], hi[0], n // 20)
    y = rng.uniform(lo[1], hi[1], n // 20)
    z = rng.uniform(lo[2] - 0.5, hi[2] + 0.5, n // 20)
    inj = np.stack([x, y, z], 1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([pts, inj]), np.float32), n


@functools.lru_cache(maxsize=None)
def outlier_nearest(seed):
    """the brute-force OUT_NB nearest of every row (KO.knn at an infinite radius)"""
    return KO.knn(outlier_cloud(seed)[0], OUT_NB, np.inf)


@functools.lru_cache(maxsize=None)
def outlier_reference(seed):
    """-> KO.Statistical at (OUT_NB, OUT_STD); its score is outlier_nearest's mean"""
    score = outlier_nearest(seed).mean
    T = score.mean() + OUT_STD * score.std(ddof=1)
    return KO.Statistical(score, float(T), score <= T)


@functools.lru_cache(maxsize=None)
def outlier_far_rows(seed):
    """rows of the injected points farther than OUT_FAR from every surface sample"""
    pts, n = outlier_cloud(seed)
    X = pts.astype(np.float64)
    d2 = ((X[n:, None, :] - X[None, :n, :]) ** 2).sum(-1).min(1)
    return n + np.nonzero(d2 > OUT_FAR ** 2)[0]
