"""Seeded input families of the plane segmentation tests (tests/test_plane_oracle.py checks each family's conditions on the CPU with the oracle
alone, tests/test_hip_plane.py runs the same families on the device) and the oracle's result for each, computed once per process.  A case is
(family, argument) -> (points float32 [n,3], dist, n_hyp, max_planes, min_inliers, seed).

  small      -- n = 0, 1, 2, 3 (one possible plane), 4;
  tile       -- a noisy slab in a box of clutter, n at the scoring kernel's wave (64), workgroup (256 lanes), point tile (1024 rows) and two-tile
                edges - 1, + 0, + 1;
  hyp        -- n_hyp = 1, and the LDS hypothesis chunk (128) - 1, + 0, + 1, and two chunks + 1;
  caps       -- n_hyp and max_planes at their caps (one above is refused: the argument tests);
  lattice    -- the integer lattice 9 x 9 x 9 ascending, permuted and shifted by 4096: every product is exact, many hypotheses tie and the lowest
                h must win, the shift changes no label and no count;
  threshold  -- the lattice at dist = 1.0 (rows exactly one layer away satisfy s s == dist^2 q: inliers) and one float64 step below it;
  collinear  -- 200 points on one line: every hypothesis is invalid;
  copies     -- 257 copies of one point;
  dead       -- NaN and inf rows in the slab cloud; a cloud with two live rows;
  early      -- min_inliers above the best count; max_planes = 0; max_planes = 12 on a room view (it ends after the faces it sees);
  seeds      -- the slab cloud under two seeds;
  room       -- view 0 of synth.make_dense_pair(s, 4000), s in {7, 0, 1}, dist 0.01, 256 and 1024 hypotheses, 8 planes, min_inliers 100, seed 1;
  objects    -- the 40,000-point view of seeds 7 and 0, 256 hypotheses, min_inliers 2500: the room's faces go, the furniture stays.
SCORE_CASES are inputs of hip.plane_score alone: (points, triples int32 [H,3], dist).  No GPU imports."""
import functools

import numpy as np

import _plane_oracle as PO
from roreg_amd import hip, synth

WAVE, THREADS, TILE, CHUNK = 64, hip.PLANE_THREADS, hip.PLANE_TILE, hip.PLANE_HYP_CHUNK
LAT_SIDE = 9
LAT_N = LAT_SIDE ** 3
LAT_SHIFT = 4096.0
LAT_DIST = 0.25
THRESHOLD_BELOW = float(np.nextafter(1.0, 0.0))
SLAB_DIST = 0.02
ROOM_SEEDS, ROOM_HYP, ROOM_N = (7, 0, 1), (256, 1024), 4000
ROOM_DIST, ROOM_PLANES, ROOM_MIN, ROOM_SEED = 0.01, 8, 100, 1
OBJ_SEEDS, OBJ_N, OBJ_HYP, OBJ_MIN = (7, 0), 40000, 256, 2500
OBJ_EPS, OBJ_MIN_POINTS = 0.05, 4
DEAD_ROWS = (0, 1, 64, 150, 298, 299)
LOOPS_MAX_WORK = 150_000         # (hypothesis, row) visits of the literal loops per case


def slab_cloud(n, seed=0):
    """two thirds of the rows within 1 cm of the plane x + 2 y + 2 z = 1.5 inside the unit box, the rest anywhere in the box"""
    rng = np.random.default_rng([n, seed, 0x91a])
    pts = rng.uniform(0.0, 1.0, (n, 3))
    on = rng.uniform(0, 1, n) < 2.0 / 3.0
    nrm = np.array([1.0, 2.0, 2.0]) / 3.0
    off = pts @ nrm - 0.5
    pts[on] -= (off[on] - rng.uniform(-0.01, 0.01, int(on.sum())))[:, None] * nrm
    return pts.astype(np.float32)


def lattice_cloud(order='ascending', shift=0.0):
    g = np.arange(LAT_SIDE, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + shift
    if order == 'permuted':
        pts = pts[np.random.default_rng(0x1a7).permutation(LAT_N)]
    return pts.astype(np.float32)


def dead_cloud(which):
    if which == 'few':
        pts = slab_cloud(5, 2)
        pts[0, 0] = np.nan; pts[2, 1] = np.inf; pts[4] = -np.inf
        return pts
    pts = slab_cloud(300, 1)
    pts[0, 0] = np.nan; pts[1, 1] = np.inf; pts[64, 2] = -np.inf; pts[150] = np.nan; pts[298, 2] = np.nan; pts[299, 0] = np.inf
    return pts


@functools.lru_cache(maxsize=None)
def room_view(seed, n):
    return synth.make_dense_pair(seed, n)[0]


def case(name, arg=None):
    if name == 'small':
        return slab_cloud(8, 3)[:arg], 0.1, 16, 2, 3, 5
    if name == 'tile':
        return slab_cloud(arg), SLAB_DIST, 64, 2, 10, 2
    if name == 'hyp':
        return slab_cloud(300), SLAB_DIST, arg, 2, 10, 4
    if name == 'caps':
        if arg == 'n_hyp':
            return slab_cloud(50), SLAB_DIST, hip.PLANE_MAX_HYP, 1, 3, 6
        return slab_cloud(300), SLAB_DIST, 8, hip.PLANE_MAX_PLANES, 10, 6
    if name == 'lattice':
        return lattice_cloud(arg[0], arg[1]), LAT_DIST, 64, 9, 3, 3
    if name == 'threshold':
        return lattice_cloud(), arg, 64, 3, 3, 3
    if name == 'collinear':
        return (np.arange(200, dtype=np.float64)[:, None] * np.array([1.0, 2.0, 3.0])).astype(np.float32), 0.5, 64, 2, 3, 1
    if name == 'copies':
        return np.repeat(slab_cloud(1, 3), 257, 0), 0.5, 64, 2, 3, 1
    if name == 'dead':
        return dead_cloud(arg), SLAB_DIST, 64, 2, 3, 1
    if name == 'early':
        if arg == 'min_inliers':
            return slab_cloud(300), SLAB_DIST, 64, 3, 301, 1
        if arg == 'no_planes':
            return slab_cloud(300), SLAB_DIST, 64, 0, 3, 1
        return room_view(7, ROOM_N), ROOM_DIST, 256, 12, ROOM_MIN, ROOM_SEED
    if name == 'seeds':
        return slab_cloud(300), SLAB_DIST, 32, 1, 10, arg
    if name == 'room':
        return room_view(arg[0], ROOM_N), ROOM_DIST, arg[1], ROOM_PLANES, ROOM_MIN, ROOM_SEED
    if name == 'objects':
        return room_view(arg, OBJ_N), ROOM_DIST, OBJ_HYP, ROOM_PLANES, OBJ_MIN, ROOM_SEED
    raise KeyError(name)


SMALL_CASES = [('small', n) for n in (0, 1, 2, 3, 4)]
TILE_CASES = [('tile', e + d) for e in (WAVE, THREADS, TILE, 2 * TILE) for d in (-1, 0, 1)]
HYP_CASES = [('hyp', h) for h in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)]
CAPS_CASES = [('caps', 'n_hyp'), ('caps', 'max_planes')]
LATTICE_CASES = [('lattice', ('ascending', 0.0)), ('lattice', ('permuted', 0.0)), ('lattice', ('ascending', LAT_SHIFT))]
THRESHOLD_CASES = [('threshold', 1.0), ('threshold', THRESHOLD_BELOW)]
DEGENERATE_CASES = [('collinear', None), ('copies', None)]
DEAD_CASES = [('dead', 'some'), ('dead', 'few')]
EARLY_CASES = [('early', 'min_inliers'), ('early', 'no_planes'), ('early', 'room')]
SEED_CASES = [('seeds', 1), ('seeds', 2)]
ROOM_CASES = [('room', (s, h)) for s in ROOM_SEEDS for h in ROOM_HYP]
OBJECT_CASES = [('objects', s) for s in OBJ_SEEDS]
CASES = (SMALL_CASES + TILE_CASES + HYP_CASES + CAPS_CASES + LATTICE_CASES + THRESHOLD_CASES + DEGENERATE_CASES + DEAD_CASES + EARLY_CASES + SEED_CASES
         + ROOM_CASES + OBJECT_CASES)
FAMILIES = ('small', 'tile', 'hyp', 'caps', 'lattice', 'threshold', 'collinear', 'copies', 'dead', 'early', 'seeds', 'room', 'objects')


def case_id(c):
    if c[1] is None:
        return c[0]
    return c[0] + '-' + ('-'.join(f'{v:g}' if isinstance(v, float) else str(v) for v in c[1]) if isinstance(c[1], tuple) else repr(c[1]) if isinstance(c[1], float) else str(c[1]))


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    return PO.segment(*case(name, arg))


# ---- hip.plane_score alone ------------------------------------------------------------------------------------------------------------------------
def lattice_row(x, y, z):
    return (x * LAT_SIDE + y) * LAT_SIDE + z


AXIS_TRIPLE = (lattice_row(4, 0, 0), lattice_row(4, 1, 0), lattice_row(4, 0, 1))          # the inner axis plane x = 4: n = (1, 0, 0), q = 1


def score_case(name):
    """-> (points, triples int32 [H,3], dist)"""
    if name in ('axis-at', 'axis-below'):
        return lattice_cloud(), np.array([AXIS_TRIPLE], np.int32), 1.0 if name == 'axis-at' else THRESHOLD_BELOW
    if name == 'edges':
        pts = dead_cloud('some')
        n = pts.shape[0]
        t = [(5, 5, 9), (5, 9, 5), (9, 5, 5), (-1, 5, 9), (5, n, 9), (5, 9, DEAD_ROWS[2]), (DEAD_ROWS[0], 5, 9), (5, 9, 12), (n - 3, 9, 12), (12, 9, 5)]
        return pts, np.array(t, np.int32), SLAB_DIST
    if name == 'none':
        return slab_cloud(65), np.zeros((0, 3), np.int32), SLAB_DIST
    if name == 'empty-cloud':
        return np.zeros((0, 3), np.float32), np.array([(0, 1, 2)], np.int32), SLAB_DIST
    raise KeyError(name)


SCORE_CASES = ('axis-at', 'axis-below', 'edges', 'none', 'empty-cloud')


@functools.lru_cache(maxsize=None)
def score_reference(name):
    return PO.score(*score_case(name))


def loops_plan(c):
    """How the literal loops cover a case within LOOPS_MAX_WORK: ('rounds', k) = the whole definition for the first k rounds (a prefix: a run
    with max_planes = k), or ('score', hypotheses) = the literal count of a strided sample of round 0's hypotheses."""
    pts, _, H, K, _, _ = case(*c)
    per_round = max(1, H * pts.shape[0])
    if per_round <= LOOPS_MAX_WORK:
        return 'rounds', min(K, max(1, LOOPS_MAX_WORK // per_round))
    m = max(2, LOOPS_MAX_WORK // max(1, pts.shape[0]))
    return 'score', np.unique(np.linspace(0, H - 1, m).astype(np.int64))
