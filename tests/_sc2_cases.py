"""Seeded cases of the spatial-compatibility hypothesis generator (tests/_sc2_oracle.py): rows k0, k1, scores of synth.make_ransac_case plus
hand-made ones.  Every case keeps each off-diagonal |a_ij - b_ij| at least MARGIN away from tau (a seed that does not is replaced by the
next), so the bit-exact comparisons of the integer stages do not hinge on the last bit of a square root.  Each case and its oracle result
are built once per process."""
import functools
from collections import namedtuple

import numpy as np

import _sc2_oracle as O
from roreg_amd import hip, synth
from roreg_amd.group import tables

MARGIN = 1e-10
TAU = 0.1
ANCHOR = 17                                                        # make_ransac_case's ground truth: R = tables().R[17], t = (0.2, -0.4, 0.1)
MAX_CONDITION_DROP = 0.10                                          # the share of fitted rows the conditioning filter may leave out of a case
SIGMA_RATIO = 1e-3

Case = namedtuple('Case', 'name P Q scores tau max_seeds K ref margin')


def ground_truth():
    T = np.eye(4)
    T[:3, :3] = tables().R[ANCHOR]; T[:3, 3] = [0.2, -0.4, 0.1]
    return T


def _finish(name, P, Q, scores, tau, max_seeds, K):
    ref = O.hypotheses(P, Q, tau, max_seeds, K)
    return Case(name, P, Q, scores, tau, max_seeds, K, ref, O.threshold_margin(ref.diff, tau))


@functools.lru_cache(maxsize=None)
def synth_case(seed, M, outlier, tau=TAU, max_seeds=1000, K=20):
    """rows of synth.make_ransac_case(seed', M, outlier=outlier), seed' = the first of seed, seed + 1000, ... that keeps the margin"""
    for attempt in range(20):
        k0, k1, scores, _, _ = synth.make_ransac_case(seed + 1000 * attempt, M, H=min(M, 10), outlier=outlier)
        case = _finish(f'synth{seed}+{attempt}-M{M}-o{outlier}-S{max_seeds}-K{K}', k0, k1, scores, tau, max_seeds, K)
        if case.margin >= MARGIN:
            return case
    raise AssertionError(f'no seed near {seed} keeps |a - b| {MARGIN} away from tau at M = {M}')


@functools.lru_cache(maxsize=None)
def duplicates_case():
    """correspondences repeated: a_ij = b_ij = 0 between the copies, which are compatible with each other and share every other bit"""
    base = synth_case(11, 65, 0.6)
    P, Q = base.P.copy(), base.Q.copy()
    for dst, src in ((5, 3), (40, 3), (64, 63), (17, 16)):
        P[dst] = P[src]; Q[dst] = Q[src]
    return _finish('duplicates-M65', P, Q, np.ones(65), TAU, 1000, 20)


@functools.lru_cache(maxsize=None)
def tied_case(M=70):
    """every correspondence an exact inlier of one rigid motion: every degree is M - 1 and every N2 is M - 2, so seeds and sets are in index order"""
    rng = np.random.default_rng(5)
    Q = rng.uniform(0, 3, (M, 3))
    T = ground_truth()
    P = Q @ T[:3, :3].T + T[:3, 3]
    return _finish(f'tied-M{M}', P, Q, np.ones(M), TAU, 1000, 20)


@functools.lru_cache(maxsize=None)
def all_outlier_case(M=129, tau=0.02):
    """no correspondence is right and tau is tight: degrees of 0, 1, 2, ... and many sets of fewer than 3 members"""
    return synth_case(23, M, 1.0, tau=tau)


@functools.lru_cache(maxsize=None)
def one_stripe_case(M=641, tau=0.002):
    """the right correspondences sit at j = 5, 69, 133, ...: one lane's stripe of columns holds every compatible column of their seeds (the
    selection's per-lane cache of four runs empty and is filled again), all others are wrong under a tight tau"""
    base = synth_case(29, M, 1.0, tau=tau)
    P, Q = base.P.copy(), base.Q.copy()
    T = ground_truth()
    rows = np.arange(5, M, 64)
    P[rows] = Q[rows] @ T[:3, :3].T + T[:3, 3]
    case = _finish(f'one-stripe-M{M}', P, Q, np.ones(M), tau, 1000, 20)
    h = int(np.where(case.ref.seeds == 5)[0][0])
    assert case.margin >= MARGIN and rows.shape[0] >= 10 and (case.ref.cons[h][:rows.shape[0]] % 64 == 5).all()
    return case


def stage_cases():
    """the cases of the bit-exact stage comparison"""
    tiles = sorted({hip.SC2_SEED_TILE - 1, hip.SC2_SEED_TILE + 1, hip.SC2_COL_TILE - 1, hip.SC2_COL_TILE + 1, 2 * hip.SC2_COL_TILE - 1, 2 * hip.SC2_COL_TILE + 1})
    sizes = sorted(set([0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 257] + tiles))
    out = [synth_case(11, M, 0.6) for M in sizes]
    out += [synth_case(11, M, 0.6, max_seeds=10) for M in (9, 10, 11, 257)]              # either side of max_seeds; S < M
    out += [synth_case(11, 257, 0.6, max_seeds=hip.SC2_SEED_TILE + 1)]                    # a second, one-row seed tile over five column tiles
    out += [synth_case(11, 129, 0.6, K=3), synth_case(11, 129, 0.6, K=64), synth_case(11, 65, 0.9, K=64)]
    out += [all_outlier_case(), duplicates_case(), tied_case()]
    out += [one_stripe_case(), synth_case(11, 257, 0.6, K=64), synth_case(11, 1500, 0.9, max_seeds=70, K=64)]     # a lane's cache of four refilled
    out += [synth_case(11, 1025, 0.9, max_seeds=70)]                                     # 17 words per row: a second, one-word chunk in the second-order kernel
    out += [synth_case(11, 1500, 0.9)]
    return out


def recovery_cases():
    return [synth_case(11, 257, 0.6), synth_case(11, 1500, 0.9), synth_case(11, 1500, 0.95)]


def fitted_rows(case):
    """(rows whose set has >= 3 members, those of them the conditioning filter admits)"""
    fitted = (case.ref.cons >= 0).sum(1) >= 3
    sv = case.ref.sigma
    with np.errstate(invalid='ignore', divide='ignore'):
        ok = fitted & (sv[:, 1] / sv[:, 0] >= SIGMA_RATIO)
    return fitted, ok


def unfixed_rotations(case, rows):
    """U V^T without the determinant fix of the oracle's fitted sets (how many rows exercise the fix)"""
    out = []
    for h in np.where(rows)[0]:
        m = case.ref.cons[h][case.ref.cons[h] >= 0]
        p, q = case.P[m], case.Q[m]
        U, _, VT = np.linalg.svd((q - q.mean(0)).T @ (p - p.mean(0)))
        out.append(VT.T @ U.T)
    return np.stack(out)
