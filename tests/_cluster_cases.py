"""Seeded input families of the DBSCAN clustering tests (tests/test_cluster_oracle.py checks each family's conditions on the CPU with the oracle
alone, tests/test_hip_cluster.py runs the same families on the device) and the oracle's result for each, computed once per process.

  box       -- n uniform points in a unit cube, eps for a mean ball of about 4, min_points 1 and 4: several clusters, noise and border rows;
  chain     -- 4,097 points on a line at spacing 0.125 with eps = 0.125 (consecutive points at exactly d2 == eps^2), rows ascending along the
               line, descending (the root is the far end) or permuted: one component of diameter 4,096; with one gap widened to the next
               float32 above 0.125: two; with min_points = 3 the ends are border rows;
  lattice   -- tests/_icp_plane_cases.py lattice_case at LAT_R: neighbours at exactly r across a cell face and a corner;
  duplicate -- sites far apart, each repeated 1..5 times: min_points is met by duplicates alone (d2 == 0);
  bridge    -- two core groups joined only through one non-core row stay two clusters, twice: a bridge nearer to one group, and one at exactly
               equal d2 from a core of each;
  none      -- min_points > n: every row is noise; and n = 0;
  wide      -- tests/_fpfh_cases.py terrain_pair(0)[0] at full size (40,000 points), eps = 0.03: many workgroups hook into the same components;
  blobs     -- terrain_view(seed, 0) plus eight floating blobs of 40 points: the cluster filter's family.
No GPU imports."""
import functools

import numpy as np

import _cluster_oracle as CO
import _fpfh_cases as FK
import _icp_plane_cases as PC

# ---- box -------------------------------------------------------------------------------------------------------------------------------------
BOX_N = (1, 2, 5, 63, 64, 65, 257, 1025)
BOX_MIN_POINTS = (1, 4)


def box_eps(n):
    """the radius of the ball that holds 4 of n points spread over the unit cube"""
    return float((3.0 * 4.0 / (4.0 * np.pi * n)) ** (1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def box_case(n):
    rng = np.random.default_rng([int(n), 0xdb5c])
    return (rng.uniform(0.0, 1.0, (n, 3)) + np.array([0.3, -0.7, 1.1])).astype(np.float32)


# ---- chain -----------------------------------------------------------------------------------------------------------------------------------
CHAIN_N, CHAIN_EPS, CHAIN_GAP = 4097, 0.125, 1500
CHAIN_ORDERS = ('ascending', 'descending', 'permuted')
CHAIN_WIDE = np.nextafter(np.float32(0.125), np.float32(1.0))            # the next float32 above the spacing


def chain_line(gap=False):
    """The chain in line order.  Every coordinate is a multiple of 1 / 8 below 1024 (or CHAIN_WIDE): every d2 is exact.  gap: link CHAIN_GAP
    -> CHAIN_GAP + 1 goes sideways by CHAIN_WIDE instead of along the line by 0.125, and the chain goes on from there: that one link is longer
    than eps, every other stays at exactly eps."""
    k = np.arange(CHAIN_N)
    pts = np.zeros((CHAIN_N, 3), np.float32)
    if gap:
        pts[:, 0] = np.where(k <= CHAIN_GAP, k, k - 1).astype(np.float32) * np.float32(0.125) - np.float32(3.0)
        pts[k > CHAIN_GAP, 1] = CHAIN_WIDE
    else:
        pts[:, 0] = k.astype(np.float32) * np.float32(0.125) - np.float32(3.0)
    pts[:, 2] = np.float32(0.5)
    return pts


def chain_rows(order):
    """position along the line -> row"""
    if order == 'ascending':
        return np.arange(CHAIN_N)
    if order == 'descending':
        return np.arange(CHAIN_N)[::-1].copy()
    return np.random.default_rng(0xc4a1).permutation(CHAIN_N)


@functools.lru_cache(maxsize=None)
def chain_case(order, gap=False):
    pts = np.empty((CHAIN_N, 3), np.float32)
    pts[chain_rows(order)] = chain_line(gap)
    return pts


# ---- duplicate -------------------------------------------------------------------------------------------------------------------------------
DUP_SITES, DUP_EPS, DUP_MIN_POINTS = 20, 0.1, 3


@functools.lru_cache(maxsize=None)
def duplicate_case():
    """-> (points float32 [n,3], site int [n], copies int [DUP_SITES]): site s stands at (s, 0, 0) and is stored s % 5 + 1 times, in seeded order"""
    copies = np.arange(DUP_SITES) % 5 + 1
    site = np.repeat(np.arange(DUP_SITES), copies)
    site = site[np.random.default_rng(0xd0b1).permutation(site.shape[0])]
    pts = np.zeros((site.shape[0], 3), np.float32)
    pts[:, 0] = site
    return pts, site, copies


# ---- bridge ----------------------------------------------------------------------------------------------------------------------------------
BRIDGE_EPS, BRIDGE_MIN_POINTS = 0.125, 4
# rows of bridge_case(): A = 0..3, B = 4..7, the near bridge 8; C's first member 9, D = 10..13, the rest of C 14..16, the tie bridge 17
BRIDGE_A, BRIDGE_B, BRIDGE_NEAR = (0, 1, 2, 3), (4, 5, 6, 7), 8
BRIDGE_C, BRIDGE_D, BRIDGE_TIE = (9, 14, 15, 16), (10, 11, 12, 13), 17
BRIDGE_A_CORE, BRIDGE_B_CORE, BRIDGE_C_CORE, BRIDGE_D_CORE = 3, 4, 14, 10        # the cores next to the bridges


@functools.lru_cache(maxsize=None)
def bridge_case():
    """Four groups of four rows, each a core a with three rows 1 / 16 beside it (all four within eps of each other: all core at min_points 4).
    A's core (row 3) is at x = 0, B's (row 4) at 15 / 64, the bridge (row 8) at 8 / 64: 8 / 64 = eps from A, 7 / 64 from B, and farther than eps
    from every other row, so it counts 3 and is not core: it joins B, the nearer one, although A's core has the lower row.  C's core (row 14) is
    at x = 0, D's (row 10) at 1 / 4, the tie bridge (row 17) at 1 / 8: d2 == eps^2 to both; it joins D, whose core has the lower ROW, although C
    is the cluster with the lower number (C's row 9 comes before D).  Every coordinate is a multiple of 1 / 64: every d2 is exact."""
    s = 1.0 / 16.0

    def group(x, side):          # the core at (x, 0), the others away from the bridge
        return [(x, 0.0), (x, s), (x, -s), (x - side * s, 0.0)]
    A, B = group(0.0, 1.0), group(15.0 / 64.0, -1.0)
    C, D = group(0.0, 1.0), group(0.25, -1.0)
    xy = [A[1], A[2], A[3], A[0]] + B + [(8.0 / 64.0, 0.0)]
    lower = [C[1]] + D + [C[0], C[2], C[3]] + [(0.125, 0.0)]
    pts = np.zeros((18, 3), np.float32)
    pts[:9, :2] = xy
    pts[9:, :2] = lower
    pts[9:, 1] += 4.0
    pts[:, 2] = 0.25
    return pts


# ---- blobs -----------------------------------------------------------------------------------------------------------------------------------
BLOB_SEEDS = (0, 1, 2)
BLOB_COUNT, BLOB_POINTS, BLOB_SIGMA, BLOB_HEIGHT = 8, 40, 0.02, (1.2, 2.0)
BLOB_EPS, BLOB_MIN_POINTS, BLOB_MIN_SIZE = 0.08, 6, 100
BLOB_STAT_NB, BLOB_STAT_STD = 16, 2.0


@functools.lru_cache(maxsize=None)
def blobs_cloud(seed, which=0):
    """-> (points float32 [n + 320, 3], n): the surface rows of terrain_view(seed, which) first, then eight blobs of 40 points, sigma = 2 cm per
    coordinate, each centred 1.2 - 2.0 m above a surface row drawn at random"""
    pts = FK.terrain_view(seed, which)[0]
    n = pts.shape[0]
    rng = np.random.default_rng([int(seed), int(which), 0xb10b])
    cen = pts[rng.choice(n, BLOB_COUNT, replace=False)].astype(np.float64)
    cen[:, 2] += rng.uniform(BLOB_HEIGHT[0], BLOB_HEIGHT[1], BLOB_COUNT)
    blob = (cen[:, None, :] + rng.normal(0.0, BLOB_SIGMA, (BLOB_COUNT, BLOB_POINTS, 3))).reshape(-1, 3).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([pts, blob]), np.float32), n


def blobs_pair(seed):
    """-> (source = blobs_cloud(seed, 0), n surface rows of it, target = terrain_view(seed, 1), T_gt of the pair)"""
    src, n = blobs_cloud(seed, 0)
    return src, n, FK.terrain_view(seed, 1)[0], FK.terrain_pair(seed)[2]


# ---- the list --------------------------------------------------------------------------------------------------------------------------------
WIDE_EPS, WIDE_MIN_POINTS = 0.03, (1, 5)
LAT_R, LAT_BASES, LAT_MIN_POINTS = PC.LAT_R, PC.LAT_BASES, (1, 31)       # 31: a centre, its 6 face and 24 corner neighbours at exactly r
NONE_N = 65


def case(name, arg=None):
    """-> (points float32 [n,3], eps, min_points)"""
    if name == 'box':
        return box_case(arg[0]), box_eps(arg[0]), arg[1]
    if name == 'chain':
        return chain_case(arg), CHAIN_EPS, 1
    if name == 'chain_gap':
        return chain_case(arg, True), CHAIN_EPS, 1
    if name == 'chain_ends':
        return chain_case(arg), CHAIN_EPS, 3
    if name == 'lattice':
        return PC.lattice_case(arg[0])[0], LAT_R, arg[1]
    if name == 'duplicate':
        return duplicate_case()[0], DUP_EPS, DUP_MIN_POINTS
    if name == 'bridge':
        return bridge_case(), BRIDGE_EPS, BRIDGE_MIN_POINTS
    if name == 'none':
        return box_case(NONE_N), box_eps(NONE_N), NONE_N + 1
    if name == 'empty':
        return np.zeros((0, 3), np.float32), 0.1, 1
    if name == 'wide':
        return FK.terrain_pair(0)[0], WIDE_EPS, arg
    if name == 'blobs':
        return blobs_cloud(arg)[0], BLOB_EPS, BLOB_MIN_POINTS
    raise KeyError(name)


SMALL_CASES = ([('box', (n, p)) for n in BOX_N for p in BOX_MIN_POINTS] + [(kind, o) for kind in ('chain', 'chain_gap', 'chain_ends') for o in CHAIN_ORDERS]
               + [('lattice', (b, p)) for b in LAT_BASES for p in LAT_MIN_POINTS] + [('duplicate', None), ('bridge', None), ('none', None), ('empty', None)]
               + [('blobs', s) for s in BLOB_SEEDS])
CASES = SMALL_CASES + [('wide', p) for p in WIDE_MIN_POINTS]             # (wide: the vectorised oracle only)


def case_id(c):
    if c[1] is None:
        return c[0]
    return c[0] + '-' + ('-'.join(f'{v:g}' if isinstance(v, float) else str(v) for v in c[1]) if isinstance(c[1], tuple) else str(c[1]))


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    pts, eps, min_points = case(name, arg)
    return CO.dbscan(pts, eps, min_points)
