"""Seeded input families of the robust-loss ICP tests ("v6p") and the oracle's result for each, computed once per process.
tests/test_icp_robust_oracle.py checks each family's conditions on the CPU with the oracle alone (tests/_icp_robust_oracle.py, normal
tables from the numpy normals); tests/test_hip_icp_robust.py runs the same families on the device with the device's tables (the `*_run`
functions take the tables as arguments for that).

  tie     -- the one-iteration pair of tests/_icp_plane_cases.py (PC) at d = 0.1, every loss under both methods at the scale ONE_SCALE: at least
             a tenth of the residuals on each side of the scale, so that both branches of huber and tukey carry weight;
  conv    -- PC's convergence pair from both starts, every loss under both methods at CONV_SCALE;
  wall    -- the noisy walls of tests/_icp_cases.py (C) under tukey and the plane method: the ill-conditioned normal equations;
  chunk   -- source counts at the slot boundaries against a whole target (PC / GC chunk families), huber;
  outlier -- a height field of 40 Gaussian bumps over [-1, 1]^2 seen twice (3,000 independent samples each, noise N(0, 2 mm)); the source
             points inside a 0.7 x 0.7 patch are raised by 0.08 -- an object only the source saw --, and the source is moved by a known
             transform of about 2 degrees and 4 cm; the start is the identity.  Without a loss the raised points, all inside the 0.15 gate,
             pull the plane method more than 5 mm off; tukey at 0.03 ends within a tenth of that.
No GPU imports."""
import functools

import numpy as np

import _icp_cases as C
import _icp_gicp_cases as GC
import _icp_oracle as O
import _icp_plane_cases as PC
import _icp_plane_oracle as PO
import _icp_robust_oracle as RO

LOSSES = RO.LOSSES
METHODS = ('plane', 'gicp')
EPSILON = GC.EPSILON

# ---- tie: one iteration ------------------------------------------------------------------------------------------------------------------------
ONE_DIST = PC.TIE_DISTS[1]
ONE_SCALE = 0.01
ONE_SHARE = 0.1                    # of the residuals on each side of the scale, at least


def one_run(method, q, p, Nq, Np, T0, d, loss, scale, epsilon=EPSILON):
    """One weighted iteration from T0 -> RO.iterate_plane's / RO.iterate_gicp's dict (gicp: 'n_valid' = n and 'sum_e2' = sum d^T M d added, so
    that both methods' dicts read alike)."""
    Q, P = PO.widen(q), PO.widen(p)
    if method == 'plane':
        return RO.iterate_plane(Q, P, Nq, T0[:3, :3], T0[:3, 3], d, loss, scale)
    it = RO.iterate_gicp(Q, P, Nq, Np, T0[:3, :3], T0[:3, 3], d, epsilon, loss, scale)
    it.update(n_valid=it['n'], sum_e2=it['sum_md'])
    return it


def full_run(method, q, p, Nq, Np, T0, d, loss, scale, max_iter, epsilon=EPSILON):
    """-> (RO.Result, trace)"""
    trace = []
    if method == 'plane':
        return RO.icp_plane(q, p, Nq, T0, d, loss, scale, max_iter=max_iter, trace=trace), trace
    return RO.icp_gicp(q, p, Nq, Np, T0, d, epsilon, loss, scale, max_iter=max_iter, trace=trace), trace


def sides(it, scale):
    """-> the shares of the counted residuals with |r| <= scale and with |r| > scale"""
    inside = float((np.abs(it['e']) <= scale).mean())
    return inside, 1.0 - inside


@functools.lru_cache(maxsize=None)
def tie_source_normals():
    return PO.normals(PC.tie_pair()[1], 2 * ONE_DIST, PC.MIN_NB)


@functools.lru_cache(maxsize=None)
def tie_reference(method, loss):
    p0, p1, T0 = PC.tie_pair()
    return one_run(method, p0, p1, PC.tie_normals(ONE_DIST).table, tie_source_normals().table, T0, ONE_DIST, loss, ONE_SCALE)


# ---- conv, wall: full runs ---------------------------------------------------------------------------------------------------------------------
CONV_DIST, CONV_RADIUS, CONV_ITER, CONV_SCALE = PC.CONV_DIST, PC.CONV_RADIUS, 30, 0.02
MARGIN = 1.01                      # every step of a full run's trace at least 1 % away from tol_deg and tol_t
WALL_LOSS, WALL_SCALE = 'tukey', 0.03


@functools.lru_cache(maxsize=None)
def conv_reference(method, loss, start):
    p0, p1, _ = PC.conv_pair()
    return full_run(method, p0, p1, PC.conv_normals(CONV_RADIUS).table, GC.conv_source_normals(CONV_RADIUS).table, PC.conv_starts()[start], CONV_DIST, loss,
                    CONV_SCALE, CONV_ITER)


@functools.lru_cache(maxsize=None)
def wall_reference(seed):
    q, p, _, T0 = C.wall_pair(seed)
    return full_run('plane', q, p, PC.wall_normals(seed).table, None, T0, C.WALL_DIST, WALL_LOSS, WALL_SCALE, C.WALL_ITER)


# ---- chunk -------------------------------------------------------------------------------------------------------------------------------------
CHUNK_LOSS, CHUNK_SCALE = 'huber', 0.01


# ---- outlier -----------------------------------------------------------------------------------------------------------------------------------
OUT_SEEDS = (0, 1, 2)
OUT_N, OUT_NOISE, OUT_RAISE = 3000, 0.002, 0.08
OUT_PATCH = ((0.3, -0.2), 0.35)    # centre and half edge of the patch only the source saw
OUT_DIST, OUT_RADIUS, OUT_ITER = 0.15, 0.1, 30
OUT_LOSS, OUT_SCALE = 'tukey', 0.03
OUT_PLAIN_MM, OUT_FACTOR = 5.0, 0.1          # without a loss: at least 5 mm from the truth; with it: at most a tenth of that run's errors


@functools.lru_cache(maxsize=None)
def outlier_pair(seed):
    """-> (target float32 [n,3], source float32 [n,3], T_gt: target ~ source R^T + t; the start is the identity)"""
    rng = np.random.default_rng([int(seed), 77])
    amp, wid = rng.uniform(-0.5, 0.5, 40), rng.uniform(0.15, 0.45, 40)
    cen = np.stack([rng.uniform(-2, 2, 40), rng.uniform(-1.5, 1.5, 40)], 1)

    def surface(n):
        xy = rng.uniform(-1.0, 1.0, (n, 2))
        z = (amp[None] * np.exp(-((xy[:, None] - cen[None]) ** 2).sum(-1) / (2 * wid[None] ** 2))).sum(1)
        return np.concatenate([xy, z[:, None]], 1)

    Q = surface(OUT_N) + rng.normal(0, OUT_NOISE, (OUT_N, 3))
    P = surface(OUT_N) + rng.normal(0, OUT_NOISE, (OUT_N, 3))
    (cx, cy), half = OUT_PATCH
    obj = (np.abs(P[:, 0] - cx) < half) & (np.abs(P[:, 1] - cy) < half)
    P[obj, 2] += OUT_RAISE
    Tg = np.eye(4)
    Tg[:3, :3] = PO.rodrigues(np.array([0.02, -0.015, 0.03])); Tg[:3, 3] = [0.03, -0.02, 0.025]
    moved = (P.astype(np.float32).astype(np.float64) - Tg[:3, 3]) @ Tg[:3, :3]
    return Q.astype(np.float32), moved.astype(np.float32), Tg


@functools.lru_cache(maxsize=None)
def outlier_normals(seed):
    return PO.normals(outlier_pair(seed)[0], OUT_RADIUS, PC.MIN_NB)


@functools.lru_cache(maxsize=None)
def outlier_reference(seed, loss):
    """-> (RO.Result, trace) of the plane method from the identity, under OUT_LOSS at OUT_SCALE or (loss None) without a loss"""
    q, p, _ = outlier_pair(seed)
    return full_run('plane', q, p, outlier_normals(seed).table, None, np.eye(4), OUT_DIST, loss, OUT_SCALE if loss else None, OUT_ITER)


def verdict_margin(trace):
    return GC.verdict_margin(trace)
