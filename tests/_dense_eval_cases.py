"""Seeded input families of the dense pair evaluation tests (tests/test_dense_eval_oracle.py proves each family's property on the CPU with the
oracle alone, tests/test_hip_dense_eval.py runs them on the device) and the oracle's result for each, computed once per process.

  pair      -- synth.make_dense_pair(5, 3000) under its ground truth at three radii;
  chunk     -- _icp_cases.chunk_pairs: source AND target counts at the boundaries of a wave, a workgroup pass and a 1024-record slot (the
               backward direction chunks the target);
  threshold -- _icp_cases.threshold_case in both role orders: correspondences at exactly max_dist in both directions, one step beyond out;
  disjoint  -- pairs without a single brute-force match either way: far apart, and interleaved slabs (bounding boxes nested);
  box face  -- two clouds whose only correspondences sit at exactly max_dist across the gap of their bounding boxes.
No GPU imports."""
import functools

import numpy as np

import _dense_eval_oracle as E
import _icp_cases as C
import _icp_oracle as O
from roreg_amd import synth

PAIR_SEED, PAIR_N = 5, 3000
PAIR_DISTS = (0.02, 0.05, 0.1)
FIRST_ORDER_DIST, FIRST_ORDER_DRAWS, FIRST_ORDER_DEG, FIRST_ORDER_SHIFT = 0.1, 50, 0.5, 0.005


@functools.lru_cache(maxsize=None)
def pair():
    return synth.make_dense_pair(PAIR_SEED, PAIR_N)


@functools.lru_cache(maxsize=None)
def pair_reference(d):
    p0, p1, Tg = pair()
    return E.evaluate(p0, p1, Tg, d)


@functools.lru_cache(maxsize=None)
def chunk_reference():
    return [E.evaluate(q, p, T0, C.CHUNK_DIST) for _, q, p, T0 in C.chunk_pairs()]


@functools.lru_cache(maxsize=None)
def threshold_pairs():
    """-> [(name, cloud 0, cloud 1)], evaluated under the identity with C.THR_DIST"""
    out = []
    for base in C.THR_BASES:
        tgt, qry, _ = C.threshold_case(base)
        out += [(f'base{base:g}', tgt, qry), (f'base{base:g}swapped', qry, tgt)]
    return out


@functools.lru_cache(maxsize=None)
def threshold_reference():
    return [E.evaluate(a, b, np.eye(4), C.THR_DIST, nn=O.nearest_full) for _, a, b in threshold_pairs()]


DISJOINT_DIST = 0.05


@functools.lru_cache(maxsize=None)
def disjoint_pairs():
    """-> [(name, cloud 0, cloud 1, T)]"""
    rng = np.random.default_rng(0xd15)
    plane = lambda n, z: np.concatenate([rng.uniform(-1, 1, (n, 2)), np.full((n, 1), z)], 1).astype(np.float32)
    p0, p1, Tg = synth.make_dense_pair(9, 1500)
    far = Tg.copy(); far[:3, 3] += 100.0
    slab = np.concatenate([plane(1200, 0.0), plane(1200, 2.0)])
    return [('far', p0, p1, far), ('slab', slab, plane(900, 1.0), np.eye(4))]


FACE_DIST = 0.125


@functools.lru_cache(maxsize=None)
def box_face_pair():
    """Cloud A fills [0, 1]^3 with a 9 x 9 lattice on its face x = 1 and everything else at x <= 0.5; cloud B starts at x = 1 + d with the
    same lattice on that face and everything else at x >= 1.625 + ...: under the identity the lattice points pair up at exactly d and nothing
    else is within d.  Lattice coordinates are multiples of 1/8: every d2 is exact."""
    rng = np.random.default_rng(0xface)
    yz = np.stack(np.meshgrid(np.arange(9) / 8.0, np.arange(9) / 8.0, indexing='ij'), -1).reshape(-1, 2)
    a = np.concatenate([np.concatenate([np.ones((81, 1)), yz], 1), rng.uniform(0, 1, (1919, 3)) * [0.5, 1, 1]])
    b = np.concatenate([np.concatenate([np.full((81, 1), 1.0 + FACE_DIST), yz], 1), rng.uniform(0, 1, (1919, 3)) * [0.5, 1, 1] + [1.625, 0, 0]])
    a[81] = (0, 0, 0); a[82] = (0.5, 1, 1); b[81] = (1.625, 0, 0); b[82] = (2.125, 1, 1)
    pa, pb = rng.permutation(2000), rng.permutation(2000)
    return a[pa].astype(np.float32), b[pb].astype(np.float32)


# ---- the scene of the overlap-matrix test: 6 clouds of 2000 points, world <- cloud poses -------------------------------------------------
SCENE_DIST = 0.125


@functools.lru_cache(maxsize=None)
def scene():
    """-> (clouds [6] float32 [2000,3], poses [6] float64 [4,4]): clouds 0..1 are two views of one surface, 2..3 the box-face pair under identity
    poses, 4..5 placed far away (4 by its pose, 5 by its coordinates)."""
    p0, p1, Tg = synth.make_dense_pair(13, 2000)
    a, b = box_face_pair()
    q0, q1, Th = synth.make_dense_pair(14, 2000)
    P0 = O.perturb(np.eye(4), 25.0, 0.4, 3)
    far = O.perturb(np.eye(4), 70.0, 0.0, 4); far[:3, 3] = (40.0, -35.0, 20.0)
    clouds = [p0, p1, a + np.float32([0, 3, 0]), b + np.float32([0, 3, 0]), q0, (q1 + np.float32([-60, 10, 5])).astype(np.float32)]
    poses = [P0, P0 @ Tg, np.eye(4), np.eye(4), far, np.eye(4)]
    return clouds, poses


def relative(poses, i, j):
    return np.linalg.inv(poses[i]) @ poses[j]
