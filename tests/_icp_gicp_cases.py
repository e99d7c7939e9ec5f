"""Seeded input families of the plane-to-plane (generalized) ICP tests: the inputs of tests/_icp_plane_cases.py (PC) and tests/_icp_cases.py (C)
with a normal table for the source cloud beside the target's.  tests/test_icp_gicp_oracle.py checks each family's conditions on the CPU with the
oracle alone (tables from the numpy normals, cached per process: the target tables are PC's own); tests/test_hip_icp_gicp.py runs the same
families on the device with the device's tables (`run_full` / `run_one` take the tables as arguments for that).

  tie    -- the one-iteration pair of PC (1000 duplicated target rows), at both TIE_DISTS, normal radius 2 d;
  conv   -- the convergence pair from both starts at normal radius 0.2 and 0.1 (where the plane method cycles);
  rank   -- targets on one, two and three exact planes (epsilon regularises what the plane method refuses) and the noisy walls;
  chunk  -- source counts at the slot boundaries against a whole target; every source is a cloud of its own, with its own table
            (one point: a zero row; about half the rows of the 1023 .. 1025-point sources are zero).  Normal radius 0.25 and not PC's 0.2: at
            0.2 the oracle's fifth iteration of the 1023 .. 1025-point runs has a translation step of 1.95 tol_t, within the factor 2 of
            the tolerance that the full-run cases keep clear of (verdict_margin); at 0.25 the nearest step is a factor 2.96 away.
No GPU imports."""
import functools

import numpy as np

import _icp_cases as C
import _icp_gicp_oracle as GO
import _icp_plane_cases as PC
import _icp_plane_oracle as PO

MIN_NB = PC.MIN_NB
EPSILON = GO.EPSILON
EPSILONS = (1e-3, 1e-2, 1.0)
TIE_DISTS = PC.TIE_DISTS
CONV_DIST, CONV_ITER = PC.CONV_DIST, 30
CONV_RADII = (PC.CONV_RADIUS, PC.CYCLE_RADIUS)
RANK_DIST, RANK_RADIUS, RANK_ITER, RANK_PLANES = PC.RANK_DIST, PC.RANK_RADIUS, PC.RANK_ITER, PC.RANK_PLANES
WALL_SEEDS = PC.WALL_SEEDS
CHUNK_SRC_N, CHUNK_RADIUS = PC.CHUNK_SRC_N, 0.25


def run_one(q, p, Nq, Np, T0, d, epsilon=EPSILON):
    return GO.iterate(PO.widen(q), PO.widen(p), Nq, Np, T0[:3, :3], T0[:3, 3], d, epsilon)


def run_full(q, p, Nq, Np, T0, d, max_iter, epsilon=EPSILON):
    """-> (GO.Result, trace)"""
    trace = []
    return GO.icp(q, p, Nq, Np, T0, d, epsilon, max_iter=max_iter, trace=trace), trace


def verdict_margin(trace, tol_deg=1e-4, tol_t=1e-6):
    """How far the run's verdicts are from flipping: the smallest factor by which a step would have to change for any iteration's verdict
    (converged iff step_deg < tol_deg and step_t < tol_t) to be the other one.  An iteration that ended in 'no_support' has no step."""
    margin = np.inf
    for x in trace:
        if x['step_deg'] is None:
            continue
        rd, rt = x['step_deg'] / tol_deg, x['step_t'] / tol_t
        if rd < 1 and rt < 1:                            # converged: both would have to stay below; the nearer one decides
            margin = min(margin, 1.0 / max(rd, rt, 1e-300))
        else:                                            # not converged: every step at or above its tolerance would have to drop below it
            margin = min(margin, max(rd, rt))
    return margin


# ---- conv ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_source_normals(radius):
    return PO.normals(PC.conv_pair()[1], radius, MIN_NB)


@functools.lru_cache(maxsize=None)
def conv_reference(start, radius):
    p0, p1, _ = PC.conv_pair()
    return run_full(p0, p1, PC.conv_normals(radius).table, conv_source_normals(radius).table, PC.conv_starts()[start], CONV_DIST, CONV_ITER)


# ---- rank ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes_source_normals(n_planes):
    return PO.normals(PC.planes_pair(n_planes)[1], RANK_RADIUS, MIN_NB)


@functools.lru_cache(maxsize=None)
def planes_reference(n_planes):
    tgt, src, _, T0 = PC.planes_pair(n_planes)
    return run_full(tgt, src, PC.planes_normals(n_planes).table, planes_source_normals(n_planes).table, T0, RANK_DIST, RANK_ITER)


@functools.lru_cache(maxsize=None)
def wall_source_normals(seed):
    return PO.normals(C.wall_pair(seed)[1], RANK_RADIUS, MIN_NB)


@functools.lru_cache(maxsize=None)
def wall_reference(seed):
    q, p, _, T0 = C.wall_pair(seed)
    return run_full(q, p, PC.wall_normals(seed).table, wall_source_normals(seed).table, T0, C.WALL_DIST, C.WALL_ITER)


# ---- chunk ---------------------------------------------------------------------------------------------------------------------------------
chunk_pairs = PC.chunk_pairs


@functools.lru_cache(maxsize=None)
def chunk_normals():
    return PO.normals(chunk_pairs()[0][1], CHUNK_RADIUS, MIN_NB)


@functools.lru_cache(maxsize=None)
def chunk_source_normals():
    return [PO.normals(p, CHUNK_RADIUS, MIN_NB) for _, _, p, _ in chunk_pairs()]


@functools.lru_cache(maxsize=None)
def chunk_reference():
    """One iteration and the full run, per pair -> [(GO.iterate dict, GO.Result, trace)]"""
    Nq = chunk_normals().table
    out = []
    for (_, q, p, T0), Np in zip(chunk_pairs(), chunk_source_normals()):
        out.append((run_one(q, p, Nq, Np.table, T0, C.CHUNK_DIST),) + run_full(q, p, Nq, Np.table, T0, C.CHUNK_DIST, C.CHUNK_ITER))
    return out
