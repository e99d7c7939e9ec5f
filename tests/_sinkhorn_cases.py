"""Seeded input families of the Sinkhorn convergence tests (tests/test_sinkhorn_oracle.py on the CPU, tests/test_sinkhorn_convergence.py on
the GPU) and the float64 reference of each case, computed once per process.

Classes, by what the early exit of the recomputed iterations (csrc/ot_flash.hip, conv_stop) does with them:
  slow  -- balanced clouds whose descriptors sit in a few tight clusters: a slow mode (contraction ~0.88 per iteration) whose steps cross
           the 1 .. 8-unit band of the rule while float64 shows the iteration still converging;
  fast  -- at the float32 fixed point within 40 iterations (planted matches at small scales, looser clusters);
  never -- planted matches with scores up to ~45: the steps never come near 8 units within 100 iterations.
"""
import functools

import numpy as np

from oracle import match_ot_numpy as MO

ITERS = 100
ALPHA_RM = 3.04                                    # the shipped ot_layer.bin_score


def clustered(rng, m, n, sc=3.4, ncl=12, spread=0.05):
    """final descriptors [m,32], [n,32] float32 around `ncl` common unit-norm centres"""
    c = rng.standard_normal((ncl, 32)); c /= np.linalg.norm(c, axis=1, keepdims=True)
    s = (c[rng.integers(0, ncl, m)] + spread * rng.standard_normal((m, 32))) * sc
    t = (c[rng.integers(0, ncl, n)] + spread * rng.standard_normal((n, 32))) * sc
    return s.astype(np.float32), t.astype(np.float32)


def planted(rng, m, n, sc):
    """i.i.d. Gaussian descriptors with min(m, n) // 2 planted strong matches (the family of tests/test_hip_rm.py)"""
    s = rng.standard_normal((m, 32)).astype(np.float32) * sc; t = rng.standard_normal((n, 32)).astype(np.float32) * sc
    k = min(m, n) // 2
    t[:k] = s[:k] * 3 + rng.standard_normal((k, 32)).astype(np.float32) * 0.05
    return s, t


def with_duplicates(s, t):
    """ten target rows and seven source rows copied (exact ties among the potentials and in the read-out)"""
    s, t = s.copy(), t.copy()
    t[40:50] = t[3:13]
    s[100:107] = s[20:27]
    return s, t


# name -> (class, family, seed, m, n, family arguments, alpha).  Which form of the iteration runs depends on the target length only:
# of_iter_kernel up to 2559 points, two passes (or 'coop') above.
CASES = {
    'slow_300x260':      ('slow', 'clustered', 0, 300, 260, {}, ALPHA_RM),
    'slow_300x260_24cl': ('slow', 'clustered', 0, 300, 260, {'ncl': 24}, ALPHA_RM),   # (the worst of a 144-case scan of sc, spread, ncl, seed
                                                                                       #  at this size: float32 replay stopped by the rule vs float64)
    'slow_1000x1000_dup': ('slow', 'clustered+dup', 4, 1000, 1000, {}, ALPHA_RM),
    'slow_2500x2500':    ('slow', 'clustered', 0, 2500, 2500, {}, ALPHA_RM),
    'slow_2600x2600':    ('slow', 'clustered', 0, 2600, 2600, {}, ALPHA_RM),
    'fast_planted_700x1200': ('fast', 'planted', 5, 700, 1200, {'sc': 0.25}, 1.5),
    'fast_planted_64x2600':  ('fast', 'planted', 6, 64, 2600, {'sc': 0.2}, 1.5),
    'fast_clustered_300x260': ('fast', 'clustered', 2, 300, 260, {'sc': 2.8}, ALPHA_RM),
    'never_planted_600x200': ('never', 'planted', 7, 600, 200, {'sc': 0.5}, 1.5),
}
SLOW = [k for k, c in CASES.items() if c[0] == 'slow']


@functools.lru_cache(maxsize=None)
def descriptors(name):
    _, family, seed, m, n, kw, _ = CASES[name]
    rng = np.random.default_rng(seed)
    if family == 'planted':
        return planted(rng, m, n, **kw)
    s, t = clustered(rng, m, n, **kw)
    return with_duplicates(s, t) if family.endswith('+dup') else (s, t)


def bar_Z(Z_ref):
    """the bar tests/test_hip_rm.py holds the kernels' log-couplings to (there against the float32 oracle)"""
    return 1e-4 * max(1.0, float(np.abs(Z_ref).max()) / 20)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (Z_ref float64 after all ITERS iterations, its step record): scores as the float64 product of the float32 descriptors"""
    s, t = descriptors(name)
    return MO.log_sinkhorn_steps(s.astype(np.float64) @ t.astype(np.float64).T, CASES[name][6], ITERS, 'float64')


@functools.lru_cache(maxsize=None)
def replay32(name):
    """-> (Z float32 after all ITERS iterations, its step record): the reference's own arithmetic"""
    s, t = descriptors(name)
    return MO.log_sinkhorn_steps(s @ t.T, CASES[name][6], ITERS, 'float32')


def decided(Z_ref, m, n, gap_min=1e-3):
    """rows / columns whose arg-max in Z_ref is decided by more than gap_min on both sides of the mutual check (the convention of
    test_sinkhorn_recomputed_on_the_matrix_cores_equals_the_materialised_iterations) -> keep0 [m], keep1 [n]"""
    P = Z_ref[:m, :n]

    def gap(A):
        if A.shape[1] < 2:
            return np.full(A.shape[0], np.inf)
        top = np.partition(A, -2, axis=1)[:, -2:]
        return top[:, 1] - top[:, 0]
    row_ok, col_ok = gap(P) > gap_min, gap(P.T) > gap_min
    return row_ok & col_ok[P.argmax(1)], col_ok & row_ok[P.argmax(0)]
