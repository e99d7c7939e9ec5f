"""Seeded input families of the FPFH matcher's tests (csrc/fpfh_match.hip), built in numpy.  tests/test_fpfh_match_cases.py
checks on the CPU that each family has the property it is named for (oracle.ref_numpy.knn(.., 1) is the definition), tests/test_hip_fpfh_match.py
runs them on the device.  "FPFH-like": float32 rows 33 wide, every third non-negative and summing to 200 (to float32 rounding; a perturbed row
exceeds it by its perturbation).

  random        -- every third 200 x a Dirichlet(1) draw;
  duplicates    -- side 1 all one row; a row duplicated across a tile boundary (first copy the last row of tile k, second the first of tile k + 1)
                   on side 1, on side 0, on both; both sides the same table;
  near          -- a base row plus one channel (0, 15, 16, 31, 32) moved by 1 ulp, 1e-5, 1e-3, 1e-1, the larger moves at the lower indices;
  channel32     -- targets equal to their source in channels 0..31: channel 32 alone decides every winner;
  collapse      -- targets at a distance of about 100 whose radicands fall by a few float32 steps from one index to the next: adjacent radicands share a root;
  large_norm    -- rows with each third in one bin (squared norm about 1.2e5) and separations near 1e-2;
  zero          -- zero rows on one side, on both.
No GPU imports."""
import functools

import numpy as np

from oracle import ref_numpy as O
from roreg_amd.hip import FPFH_MATCH_TILE as TILE, fpfh_match_margin

f32 = np.float32
W = 33


def fpfh_like(rng, m):
    return np.ascontiguousarray(np.concatenate([200.0 * rng.dirichlet(np.ones(11), m) for _ in range(3)], 1), f32).reshape(m, W)


@functools.lru_cache(maxsize=None)
def random_case(m0, m1):
    rng = np.random.default_rng([m0, m1, 0xf3a7])
    return fpfh_like(rng, m0), fpfh_like(rng, m1)


# the tile edge and two tile edges straddled, one row, and a shape of several tiles with unequal sides
SHAPES = ((1, 1), (1, 300), (300, 1), (2, 2), (TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1), (2 * TILE + 1, 2 * TILE - 1), (1000, 1300))


def concentrated(i):
    """row i of a family of rows with 200 in one bin of each third: rows i != i' differ by at least 200 sqrt(2)"""
    r = np.zeros(W, f32)
    r[i % 11] = 200.0; r[11 + (i // 11) % 11] = 200.0; r[22 + (i // 121) % 11] = 200.0
    return r


# ---- duplicates ----------------------------------------------------------------------------------------------------------------------------
def all_one_row_case():
    s, t = random_case(150, 1)
    return s, np.ascontiguousarray(np.repeat(t, 2 * TILE + 3, 0))


def boundary_duplicate_case(side):
    """side 0 / 1 / 2 (= both): row TILE - 1 and row TILE of that side are the same row, and the row they copy is some other side's best match"""
    s, t = (a.copy() for a in random_case(TILE + 40, TILE + 50))
    if side in (1, 2):
        t[TILE - 1] = t[TILE] = s[5]                  # source 5's exact copy twice: index TILE - 1 wins
    if side in (0, 2):
        s[TILE - 1] = s[TILE] = t[7]
    return s, t


def identical_case():
    s, _ = random_case(TILE + 70, 1)
    s = s.copy()
    s[TILE + 3] = s[11]                                # and one duplicate inside the table
    return s, s.copy()


# ---- near-duplicates -------------------------------------------------------------------------------------------------------------------------
NEAR_CHANNELS = (0, 15, 16, 31, 32)
NEAR_STEPS = ('ulp', 1e-5, 1e-3, 1e-1)


def near_case(channel):
    """40 base rows as sources (every perturbed channel at least 1); targets: per source, its copies with `channel` raised by 1e-1, 1e-3, 1e-5 and
    one ulp, in that order (the nearest copy has the greatest index of the four), then 20 unrelated rows"""
    rng = np.random.default_rng([channel, 0x4ea7])
    s = fpfh_like(rng, 40)
    s[:, channel] = np.maximum(s[:, channel], f32(1.0))
    t = []
    for row in s:
        for step in NEAR_STEPS[::-1]:
            c = row.copy()
            c[channel] = np.nextafter(row[channel], f32(np.inf)) if step == 'ulp' else f32(row[channel] + f32(step))
            assert c[channel] != row[channel]
            t.append(c)
    return s, np.ascontiguousarray(np.concatenate([np.array(t, f32), fpfh_like(rng, 20)], 0))


def channel32_case():
    """60 concentrated-like sources; targets: per source three rows equal to it in channels 0..31 whose channel 32 lies 3, 1 and 2 away
    (the winner is the middle one; with channel 32 ignored the three tie and the first would win)"""
    rng = np.random.default_rng(0xc32)
    s = fpfh_like(rng, 60)
    s[:, 32] = f32(10.0) + rng.uniform(0.0, 5.0, 60).astype(f32)
    s[:, 22:32] *= ((f32(200.0) - s[:, 32]) / s[:, 22:32].sum(1))[:, None]
    t = np.repeat(s, 3, 0)
    t[:, 32] += np.tile(np.array([3.0, 1.0, 2.0], f32), 60)
    return s, np.ascontiguousarray(t)


# ---- sqrt collapse ---------------------------------------------------------------------------------------------------------------------------
def radicand(s, t):
    """the literal float32 radicand (before + 1e-7) of row pairs"""
    return O.pdist(s, t, 'SquareL2')


def collapse_case():
    """121 sources: third 0 = 100 in two bins, thirds 1 and 2 concentrated (distinct sources are at least 200 sqrt(2) apart).  Targets, four per
    source: the source with a moved from the first of its two bins to the second, a = a_i, then one, two and three float32 steps less: the radicand
    2 a^2 ~ 1e4 falls from one index to the next, by less than the 2^-17 spacing of the root near 100 allows it to show."""
    s, t = [], []
    for i in range(121):
        row = np.zeros(W, f32)
        p, q = i % 11, (i % 11 + 1 + (i // 11) % 10) % 11
        row[p] = row[q] = 100.0
        row[11 + i % 11] = 200.0; row[22 + (i // 11) % 11] = 200.0
        s.append(row)
        a = f32(70.0 + 0.011 * i)
        for _ in range(4):
            c = row.copy()
            c[p] = f32(100.0) - a; c[q] = f32(100.0) + a
            t.append(c)
            a = np.nextafter(a, f32(0.0))
    return np.array(s, f32), np.array(t, f32)


# ---- large norm, small separation ----------------------------------------------------------------------------------------------------------
def large_norm_case():
    """300 x 260 rows, all (200 in bin 3, 200 in bin 14, 200 in bin 30) plus a non-negative jitter of about 1e-2 in every channel"""
    rng = np.random.default_rng(0x1a26e)
    base = np.zeros(W, f32)
    base[[3, 14, 30]] = 200.0
    return ((base[None] + rng.uniform(0.0, 0.01, (300, W))).astype(f32), (base[None] + rng.uniform(0.0, 0.01, (260, W))).astype(f32))


def rows_with_several_targets_within_the_margin(s, t):
    """float64, from the margin formula: per row of s, the number of targets whose squared distance is within the row's margin of the least"""
    S, T = s.astype(np.float64), t.astype(np.float64)
    x = ((S[:, None, :] - T[None, :, :]) ** 2).sum(-1)
    margin = fpfh_match_margin(x.min(1), (S * S).sum(1), (T * T).sum(1).max())
    return (x <= (x.min(1) + margin)[:, None]).sum(1)


# ---- zero rows -------------------------------------------------------------------------------------------------------------------------------
def zero_case(which):
    """which = 1: side 1 all zero; 0: side 0 holds zero rows among others; 2: both sides hold zero rows (and side 1 a row nearer to zero than any other)"""
    s, t = (a.copy() for a in random_case(TILE + 9, TILE + 2))
    if which == 1:
        t[:] = 0.0
    if which in (0, 2):
        s[::7] = 0.0
    if which == 2:
        t[3::5] = 0.0
    return s, t


FAMILIES = dict(
    [('all_one_row', all_one_row_case), ('identical', identical_case), ('channel32', channel32_case), ('collapse', collapse_case),
     ('large_norm', large_norm_case)]
    + [(f'boundary_dup_side{k}', functools.partial(boundary_duplicate_case, k)) for k in (0, 1, 2)]
    + [(f'near_ch{c}', functools.partial(near_case, c)) for c in NEAR_CHANNELS]
    + [(f'zero_{k}', functools.partial(zero_case, k)) for k in (0, 1, 2)])


@functools.lru_cache(maxsize=None)
def family(name):
    return FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (d01, nn01, nn10) of oracle.ref_numpy.knn for a family (all of them are at most a few hundred rows)"""
    s, t = family(name)
    d01, nn01 = O.knn(t, s, 1)
    _, nn10 = O.knn(s, t, 1)
    return d01, nn01, nn10
