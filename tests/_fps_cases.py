"""Seeded input families of the farthest-point sampling tests (tests/test_fps_oracle.py checks each family's conditions on the CPU with the
oracle alone, tests/test_hip_fps.py runs the same families on the device) and the oracle's result for each, computed once per process.

  box       -- n seeded points in a unit box, n around the wave (64) and the workgroup (1024), k = n (a full permutation), 1 and n - 1;
  edge      -- n = each tier edge of the kernel - 1, + 0, + 1 (hip.FPS_TIER_EDGES), k = 64;
  lattice   -- the integer lattice 9 x 9 x 9: most steps have many rows at exactly the same D and the lowest-row rule decides; rows ascending,
               under a fixed permutation, and shifted by 4096 (float64 d2 of float32 values is exact there too);
  copies    -- a 64-point cloud repeated four times, and 257 copies of one point (D == 0: taken rows are excluded by a flag, not by D);
  start     -- start in {0, 1, n - 1};
  stop      -- the lattice stopped at exactly one lattice step (equality selects: all 729 rows), one float64 step above it (it stops at the
               first candidate at D == 1), and so far that only `start` is selected;
  dead      -- NaN and inf rows, a dead start (rows 0 and 1 dead: row 2 is first), an all-dead cloud (count 0);
  empty / k0 / over -- n = 0; k = 0; k > n;
  raw       -- one raw terrain view (tests/_fpfh_cases.py terrain_pair(0)[0], 40,000 points) at k = 2000.
No GPU imports."""
import functools

import numpy as np

import _fpfh_cases as FK
import _fps_oracle as PO
from roreg_amd import hip

BOX_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)
EDGE_K = 64
LAT_SIDE = 9
LAT_N = LAT_SIDE ** 3
LAT_SHIFT = 4096.0
COPIES_BASE, COPIES_TIMES, COPIES_ONE = 64, 4, 257
START_N, START_K = 1025, 64
DEAD_N = 1025
DEAD_ROWS = (0, 1, 64, 511, 1023, 1024)                          # row 0: NaN x, 1: +inf y, 64: -inf z, 511: all NaN, 1023: NaN z, 1024: +inf x
RAW_K = 2000
STOP_ABOVE = float(np.nextafter(1.0, 2.0))
STOP_FAR = 1.0e6


def box_case(n, seed=0):
    return np.random.default_rng([n, seed, 0xf95]).uniform(0.0, 1.0, (n, 3)).astype(np.float32)


def lattice_case(order='ascending', shift=0.0):
    g = np.arange(LAT_SIDE, dtype=np.float64)
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3) + shift
    if order == 'permuted':
        pts = pts[np.random.default_rng(0x1a7).permutation(LAT_N)]
    return pts.astype(np.float32)


def dead_case(which):
    pts = box_case(DEAD_N, 1)
    if which == 'all':
        pts = box_case(65, 2)
        pts[:, 0] = np.nan
        pts[1::2, 1] = np.inf
        return pts
    pts[0, 0] = np.nan; pts[1, 1] = np.inf; pts[64, 2] = -np.inf; pts[511] = np.nan; pts[1023, 2] = np.nan; pts[1024, 0] = np.inf
    return pts


def case(name, arg=None):
    """-> (points float32 [n,3], k, start, stop_dist or None)"""
    if name == 'box':
        return box_case(arg[0]), arg[1], 0, None
    if name == 'edge':
        return box_case(arg), EDGE_K, 0, None
    if name == 'lattice':
        return lattice_case(arg[0], arg[1]), LAT_N, 0, None
    if name == 'copies':
        if arg == 'one':
            return np.repeat(box_case(1, 3), COPIES_ONE, 0), COPIES_ONE, 5, None
        return np.tile(box_case(COPIES_BASE, 3), (COPIES_TIMES, 1)), COPIES_BASE * COPIES_TIMES, 0, None
    if name == 'start':
        return box_case(START_N), START_K, arg, None
    if name == 'stop':
        return lattice_case(), LAT_N, 0, arg
    if name == 'dead':
        return dead_case(arg[0]), arg[1], arg[2], None
    if name == 'empty':
        return np.zeros((0, 3), np.float32), 5, 0, None
    if name == 'k0':
        return box_case(65), 0, 0, None
    if name == 'over':
        return box_case(65), 100, 3, None
    if name == 'raw':
        return FK.terrain_pair(0)[0], RAW_K, 0, None
    raise KeyError(name)


BOX_CASES = [('box', (n, k)) for n in BOX_N for k in sorted({n, 1, n - 1}, reverse=True) if k > 0]
EDGE_CASES = [('edge', e + d) for e in hip.FPS_TIER_EDGES for d in (-1, 0, 1)]
LATTICE_CASES = [('lattice', ('ascending', 0.0)), ('lattice', ('permuted', 0.0)), ('lattice', ('ascending', LAT_SHIFT))]
COPIES_CASES = [('copies', 'tiled'), ('copies', 'one')]
START_CASES = [('start', s) for s in (0, 1, START_N - 1)]
STOP_CASES = [('stop', 1.0), ('stop', STOP_ABOVE), ('stop', STOP_FAR)]
DEAD_CASES = [('dead', ('some', DEAD_N, 0)), ('dead', ('some', 64, 1)), ('dead', ('some', 64, 7)), ('dead', ('all', 8, 0))]
INPUT_EDGE_CASES = [('empty', None), ('k0', None), ('over', None)]
CASES = BOX_CASES + EDGE_CASES + LATTICE_CASES + COPIES_CASES + START_CASES + STOP_CASES + DEAD_CASES + INPUT_EDGE_CASES + [('raw', None)]
FAMILIES = ('box', 'edge', 'lattice', 'copies', 'start', 'stop', 'dead', 'empty', 'k0', 'over', 'raw')
LOOPS_MAX_WORK = 300_000         # (step, row) visits of the literal double loop per case: a larger case is run to the k that stays under it (a prefix)


def stop2_of(stop_dist):
    """the square the binding hands to the kernel: one float64 product"""
    return 0.0 if stop_dist is None else float(stop_dist) * float(stop_dist)


def case_id(c):
    if c[1] is None:
        return c[0]
    return c[0] + '-' + ('-'.join(f'{v:g}' if isinstance(v, float) else str(v) for v in c[1]) if isinstance(c[1], tuple) else repr(c[1]) if isinstance(c[1], float) else str(c[1]))


@functools.lru_cache(maxsize=None)
def reference(name, arg=None):
    pts, k, start, stop = case(name, arg)
    return PO.fps(pts, k, start, stop2_of(stop))
