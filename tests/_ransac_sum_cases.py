"""Seeded inputs of the float32-score RANSAC sum tests (tests/test_ransac_sum_cases.py checks their conditions on the CPU with the oracle alone,
tests/test_hip_ransac_f32_sums.py runs them on the device) and the oracle's result for each, computed once per process.

With float32 match scores the kernels of csrc/ransac.hip rebuild numpy's pairwise float32 reduction over the COMPACTED inlier array, so
which code runs depends on the number of inliers of a hypothesis, not on the problem size.  build() plants inlier sets of chosen sizes that
no rounding can change:
  * k1 lies on a grid of multiples of 1/8 in [0, 3)^3; hypothesis h is the identity plus the translation (4 (h + 1), 0, 0), so k1 moved by
    it is exact in float64;
  * point i of group h has k0 = k1 + t_h + U(-0.02, 0.02)^3: at most 0.035 from its image under hypothesis h (ird = 0.1), at least 3.9 from
    its image under any other; every point of no group is moved 40 along y instead, an outlier of every hypothesis;
  * groups are disjoint and sit at the positions a seeded permutation gives them, in among the outliers;
  * scores are uniform(0.1, 1) float32 with about 2 % of them times 1000: sums whose float32 value depends on the order of the additions.

Families (name -> M, inlier count per hypothesis):
  S -- M = 4096, one launch of 26 hypotheses around every branch of the tree: none, sequential (< 8), one leaf with and without a tail,
       the 128 | 129 leaf boundary, splits at and beside multiples of 8 and 16, 1000.  Kernel variant <4, 4096>.
  F -- M = 4096, one hypothesis owning all, all but one, 2049 and 2048 points: the small variant's buffer exactly full.
  L -- the groups of S in M = 4097 and M = 8192: the same counts through variant <2, 8192>.
  C -- one hypothesis with more than one numpy chunk of inliers (8192): counts at and beside one and two chunks, nearly all and all points.
       SPILL names the mixed cases for which build() asserts that the 8192nd inlier is NOT the last inlier of its 64-wide ballot group (the
       chunk is reduced with part of the group carried into the next one); with every point an inlier the boundary falls between groups.
No GPU imports."""
import functools

import numpy as np

from oracle import ref_numpy as O

IRD = 0.1
NP_CHUNK = 8192                                    # numpy's reduction buffer = csrc/ransac.hip NP_CHUNK
S_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 120, 127, 128, 129, 130, 136, 137, 143, 144, 255, 256, 257, 272, 273, 1000)

CASES = {
    'S': (4096, S_COUNTS),
    'F_4096': (4096, (4096,)), 'F_4095': (4096, (4095,)), 'F_2049': (4096, (2049,)), 'F_2048': (4096, (2048,)),
    'L_4097': (4097, S_COUNTS), 'L_8192': (8192, S_COUNTS),
    'C_8191': (20000, (8191,)), 'C_8192': (20000, (8192,)), 'C_8193': (20000, (8193,)), 'C_9000_8200': (9000, (8200,)),
    'C_16384': (20000, (16384,)), 'C_16385': (20000, (16385,)), 'C_19999': (20000, (19999,)), 'C_all': (20000, (20000,)),
}
SPILL = ('C_8193', 'C_9000_8200', 'C_16384', 'C_16385', 'C_19999')
# Seeds per case, chosen so that the inputs tell reduction orders apart (tests/test_ransac_sum_cases.py::test_cases_tell_orders_apart):
# for every count >= 16 some seed makes a sequential float32 sum differ from np.sum, for every count >= 129 some seed makes a float64
# accumulation rounded once differ from it.
SEEDS = {name: (0, 1, 2, 3) for name in CASES}
SEEDS.update({'S': (0, 1, 17, 19), 'L_4097': (0, 1, 15, 19), 'L_8192': (0, 1, 19, 22), 'F_4096': (0, 1, 2, 8), 'F_4095': (0, 1, 2, 9),
              'C_8191': (0, 1, 2, 6), 'C_8192': (0, 1, 2, 10), 'C_9000_8200': (0, 1, 2, 5), 'C_16384': (0, 2, 3, 4)})
# the refinement's float32 weight normalisation: groups on both sides of the sequential / leaf / split / chunk forms
REFINE_CASES = {'R_small': (6000, (1, 2, 3, 7, 8, 9, 128, 129, 137, 1000, 4096)), 'R_8193': (9000, (8193,)), 'R_16385': (20000, (16385,))}
REFINE_SEED = 5


@functools.lru_cache(maxsize=None)
def build(M, counts, seed):
    """-> k0 [M,3] f64, k1 [M,3] f64, scores [M] float32, Trans [H,3,4] f64, group [M] (the hypothesis a point is an inlier of, -1 = none).
    The arrays are shared between tests: do not write to them."""
    counts = tuple(int(c) for c in counts)
    assert sum(counts) <= M
    rng = np.random.default_rng(seed)
    H = len(counts)
    k1 = rng.integers(0, 24, (M, 3)) / 8.0
    group = np.full(M, -1, np.int64)
    place = rng.permutation(M)
    at = 0
    for h, c in enumerate(counts):
        group[place[at:at + c]] = h
        at += c
    Trans = np.zeros((H, 3, 4))
    Trans[:, :, :3] = np.eye(3)
    Trans[:, 0, 3] = 4.0 * (np.arange(H) + 1)
    shift = np.where(group[:, None] >= 0, Trans[np.maximum(group, 0), :, 3], np.array([0.0, 40.0, 0.0])[None])
    k0 = k1 + shift + rng.uniform(-0.02, 0.02, (M, 3))
    scores = rng.uniform(0.1, 1.0, M).astype(np.float32)
    scores[rng.random(M) < 0.02] *= np.float32(1000)
    return k0, k1, scores, Trans, group


def case(name, seed):
    M, counts = CASES[name] if name in CASES else REFINE_CASES[name]
    out = build(M, counts, seed)
    if name in SPILL or name == 'C_all':
        assert spills(out[4]) == (name in SPILL), (name, seed)
    return out


def spills(group):
    """True when a full numpy chunk of inliers (of the single hypothesis) ends inside a 64-wide ballot group that holds further inliers: the
    kernel then reduces the chunk and carries the rest of the group's inliers into the next one."""
    idx = np.where(group == 0)[0]
    out = False
    for k in range(NP_CHUNK, idx.size, NP_CHUNK):                  # idx[k - 1] closes a chunk, idx[k] opens the next
        out = out or idx[k] // 64 == idx[k - 1] // 64
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, seed):
    """-> (overlap float32 [H] as yohoo_ransac.overlap_cal gives it on the float32 scores, best = the first index of the strictly greatest
    overlap above 0 as O.yohoo_ransac's running '>' keeps it, or -1)."""
    k0, k1, sc, Tr, _ = case(name, seed)
    ov = np.array([O.overlap_cal(k0, k1, Tr[h], sc, IRD) for h in range(Tr.shape[0])])
    assert ov.dtype == np.float32
    return ov, first_best(ov)


def first_best(ov):
    best, at = 0, -1
    for h, v in enumerate(ov):
        if v > best:
            best, at = v, h
    return at
