"""Seeded input families of the dense-ICP edge tests (tests/test_icp_oracle.py checks each family's conditions on the CPU with the oracle
alone, tests/test_hip_icp_edges.py runs the same families on the device) and the oracle's result for each, computed once per process.

  solve     -- 256 pairs of 3..8 points whose 3x3 problem H spans the conditioning the solve can meet: isotropic, planar, nearly
               collinear and collinear inlier sets, mirrored targets (det(U V^T) = -1), equal singular values, H over sixteen decades;
  grid      -- clouds in boxes whose cell tables sit at the boundaries of the three-launch exclusive scan (csrc/icp.hip SCAN_BLOCK = 4096
               cells per scan block, 256 block sums per thread pass of the top scan, 2^24 cells at most);
  chunk     -- source and target counts at the boundaries of a wave (64), a workgroup pass (256) and a slot (ICP_CHUNK = 1024);
  threshold -- queries at exactly max_dist from their target across a cell face, one float32 step beyond it, just inside and just outside
               across a cell corner, and exactly midway between two targets at max_dist (coordinates on a dyadic lattice: every d2 exact);
  wall      -- a noisy planar scan, a third singular value of H at the noise level: full runs that pass through det(U V^T) = -1.
No GPU imports."""
import functools

import numpy as np

import _icp_oracle as O
from roreg_amd import synth


def rotation(rng):
    """A seeded random proper rotation (QR of a Gaussian matrix, signs fixed)."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


# ---- solve -------------------------------------------------------------------------------------------------------------------------------
SOLVE_SEED, SOLVE_PAIRS = 1, 256
SOLVE_FAMILIES = ((1, 1, 1), (1, .5, .2), (1, .7, 1e-3), (1, .7, 0), (1, 1e-4, 1e-5), (1, .3, .3), (1, 1e-9, 0), (1, 1e-12, 0))
SOLVE_DECADES = tuple(range(-4, 4))                # whole pairs times 10^k: H = sum q p^T over sixteen decades
SOLVE_DIST = 1e5                                   # one max_dist for the batch: every source point of every pair is an inlier
SOLVE_BAND = (0.25e-10, 4e-10)                     # sigma2 / sigma1 here: 'rank <= 1' and 'rank 2' are both legitimate verdicts


@functools.lru_cache(maxsize=None)
def _solve_raw():
    rng = np.random.default_rng(SOLVE_SEED)
    out = []
    for i in range(SOLVE_PAIRS):
        mirrored, fam, dec = i % 2 == 1, (i // 2) % 8, (i // 16) % 8
        n = int(rng.integers(3, 9))
        g = rng.standard_normal((n, 3)) * np.array(SOLVE_FAMILIES[fam], np.float64)
        Rs, Rm, tm = rotation(rng), rotation(rng), rng.standard_normal(3)
        gt = g * np.array([1.0, 1.0, -1.0]) if mirrored else g                  # the thinnest axis of every family is its last
        src = g @ Rs.T
        tgt = (gt @ Rs.T) @ Rm.T + tm + 1e-3 * rng.standard_normal((n, 3))
        s = 10.0 ** SOLVE_DECADES[dec]
        T0 = np.eye(4); T0[:3, :3] = Rm; T0[:3, 3] = tm * s
        out.append(dict(Q=(tgt * s).astype(np.float32), P=(src * s).astype(np.float32), T0=T0, family=fam, mirrored=mirrored, decade=SOLVE_DECADES[dec]))
    return out


def solve_one(c):
    """The oracle on one pair of the family: one search under T0, both sums, the 3x3 solve -> dict(it, R, t, S, sign, status, d2)."""
    Q, P = c['Q'].astype(np.float64), c['P'].astype(np.float64)
    it = O.iterate(Q, P, c['T0'][:3, :3], c['T0'][:3, 3], SOLVE_DIST, O.nearest_full)
    R, t, S, sign = O.solve_full(it['H'], it['cq'], it['cp']) if it['n'] >= 3 else (None, None, None, 0.0)
    Pt = O.transform(P, c['T0'][:3, :3], c['T0'][:3, 3])
    e = Q[None] - Pt[:, None]
    d2 = np.sort((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], axis=1)
    return dict(it=it, R=R, t=t, S=S, sign=sign, status='max_iter' if R is not None else 'no_support', d2=d2)


@functools.lru_cache(maxsize=None)
def solve_family():
    """-> (pairs, oracle results, number of pairs dropped): the seeded pairs less those whose sigma2 / sigma1 lies in SOLVE_BAND (the only
    rule by which a pair leaves the family)."""
    pairs, refs, dropped = [], [], 0
    for c in _solve_raw():
        r = solve_one(c)
        if r['S'] is not None and r['S'][0] > 0 and SOLVE_BAND[0] <= r['S'][1] / r['S'][0] <= SOLVE_BAND[1]:
            dropped += 1
            continue
        pairs.append(c); refs.append(r)
    return pairs, refs, dropped


def solve_bound(r):
    """max |R_dev - R_ref| a backward-stable solver may show on this pair: the rotation factor of H moves by at most 2 |dH| / gap, both
    solvers (one-sided Jacobi on the device, LAPACK here) are backward stable to a few tens of eps |H| -> ~5e-14 sigma1 / gap; a factor 20
    on top.  gap = sigma2 + sign sigma3 (the distance of the two singular values that the constrained rotation must keep apart)."""
    return 1e-12 * r['S'][0] / (r['S'][1] + r['sign'] * r['S'][2])


# ---- grid --------------------------------------------------------------------------------------------------------------------------------
# max_dist = 1 and the box [0, dims - 2.5] per axis give exactly these dims (floor(extent) + 3): the scan runs over cells + 1 words
GRID_DIMS = ((3, 3, 3),                    # 27 cells, a single point
             (15, 13, 21),                 # 4095 cells: cells + 1 = 4096, exactly one scan block
             (16, 16, 16),                 # 4096 cells: two blocks, one word in the second
             (75, 341, 41),                # 2^20 - 1 cells: 256 blocks, the top scan's threads take one block sum each
             (64, 128, 128),               # 2^20 cells: 257 blocks, two block sums per thread
             (256, 256, 256))              # 2^24 cells, the maximum: a 64 MB table, 4097 blocks


@functools.lru_cache(maxsize=None)
def grid_case(dims):
    """-> (points float32 [n,3], box float64 [2,3]): uniform over the box, clusters in the first and in the last interior cell, a few
    duplicated rows.  (3,3,3): one point."""
    dims = np.array(dims, np.float64)
    box = np.stack([np.zeros(3), dims - 2.5])
    rng = np.random.default_rng([int(v) for v in dims] + [0x6c1d])
    if tuple(int(v) for v in dims) == (3, 3, 3):
        return rng.uniform(0, 0.5, (1, 3)).astype(np.float32), box
    p = np.concatenate([rng.uniform(0, 1, (3000, 3)) * box[1], rng.uniform(0, 1, (300, 3)), (dims - 3.0) + rng.uniform(0, 0.5, (300, 3))])
    p = p[rng.permutation(p.shape[0])].astype(np.float32)
    p[100:140] = p[2000:2040]                                                # duplicated rows share a cell
    return np.minimum(p, box[1].astype(np.float32)), box


def grid_expected(points, origin, edge, dims):
    """The counting sort the grid must be -> (original rows in (cell, row) order, cell starts [cells + 1]); the cell of a point is
    floor((v - origin) * (1 / edge)) per axis in float64, clamped to the table (csrc/icp.hip cell_of)."""
    c = np.floor((points.astype(np.float64) - np.asarray(origin, np.float64)) * (1.0 / float(edge))).astype(np.int64)
    c = np.clip(c, 0, np.array(dims, np.int64) - 1)
    cid = (c[:, 2] * int(dims[1]) + c[:, 1]) * int(dims[0]) + c[:, 0]
    order = np.argsort(cid, kind='stable')
    starts = np.concatenate([[0], np.cumsum(np.bincount(cid, minlength=int(np.prod(np.array(dims, np.int64)))))])
    return order.astype(np.int32), starts.astype(np.int32), cid


# ---- chunk -------------------------------------------------------------------------------------------------------------------------------
CHUNK_SEED, CHUNK_N, CHUNK_DIST, CHUNK_ITER = 51, 4000, 0.1, 10
CHUNK_SRC_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3073)       # sources p1[:n] against the whole target
CHUNK_TGT_N = (1, 2, 3, 64, 1025)                                                                 # targets p0[:n] against the whole source


@functools.lru_cache(maxsize=None)
def chunk_pairs():
    """-> [(name, target float32, source float32, T0)]: one batch"""
    p0, p1, Tg = synth.make_dense_pair(CHUNK_SEED, CHUNK_N)
    T0 = O.perturb(Tg, 1.0, 0.02, CHUNK_SEED)
    return [(f'src{n}', p0, p1[:n], T0) for n in CHUNK_SRC_N] + [(f'tgt{n}', p0[:n], p1, T0) for n in CHUNK_TGT_N]


@functools.lru_cache(maxsize=None)
def chunk_reference():
    return [O.icp(q, p, T0, CHUNK_DIST, max_iter=CHUNK_ITER) for _, q, p, T0 in chunk_pairs()]


# ---- threshold ---------------------------------------------------------------------------------------------------------------------------
THR_DIST = 0.125
THR_BASES = (0.0, -3.0, 1024.0)
THR_GRID_DISTS = (THR_DIST, 2 * THR_DIST, THR_DIST / 2)          # the radius the grids are built for; the batch searches with THR_DIST
# |offset| per axis of the corner queries: 3 a^2 against d^2 = 0.015625.  0.072 is inside and 0.0722 outside where float32 resolves them
# (bases 0 and -3); at base 1024 a float32 step is 2^-13 and both sums round to 591 steps (inside), 0.0723 to 592 steps (outside).
THR_CORNERS = (0.072, 0.0722, 0.0723)
KIND_FACE, KIND_BEYOND, KIND_CORNER, KIND_TIE = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def threshold_case(base):
    """-> (targets float32 [27 + 12, 3], queries float32 [m,3], kind int [m]) around a 3x3x3 lattice of spacing 4 d based at `base`.  Lattice
    coordinates and face offsets are multiples of d / 8, so the cell arithmetic and those d2 are exact in float32 and float64."""
    d = THR_DIST
    b = np.float32(base)
    k = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing='ij'), -1).reshape(-1, 3)
    lat = (b + np.float32(4 * d) * k.astype(np.float32)).astype(np.float32)
    q, kind = [], []
    for t in lat:
        for ax in range(3):
            for sg in (-1.0, 1.0):
                x = t.copy(); x[ax] = np.float32(t[ax] + np.float32(sg * d))                # exactly d away across the cell face at t
                q.append(x); kind.append(KIND_FACE)
                y = x.copy(); y[ax] = np.nextafter(x[ax], np.float32(sg * np.inf))          # one step of the SUM further (an offset's last bit is lost in the addition)
                q.append(y); kind.append(KIND_BEYOND)
        for a in THR_CORNERS:
            for sx in (-1, 1):
                for sy in (-1, 1):
                    for sz in (-1, 1):
                        q.append((t + np.float32(a) * np.float32([sx, sy, sz])).astype(np.float32)); kind.append(KIND_CORNER)
    # exact ties at the threshold: two extra targets at +-d around the centre of a lattice cube, the query at the centre; the lowest row wins,
    # and that is the +d target for the first three centres, the -d target for the last three
    extra = []
    centres = [(0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0), (1, 0, 0), (1, 1, 1)]
    for i, c in enumerate(centres):
        cen = (b + np.float32(4 * d) * np.float32(c) + np.float32(2 * d)).astype(np.float32)
        e = np.zeros(3, np.float32); e[i % 3] = np.float32(d)
        extra += [cen + e, cen - e] if i < 3 else [cen - e, cen + e]
        q.append(cen); kind.append(KIND_TIE)
    targets = np.concatenate([lat, np.stack(extra)]).astype(np.float32)
    return targets, np.stack(q).astype(np.float32), np.array(kind)


@functools.lru_cache(maxsize=None)
def threshold_reference(base):
    """-> (assign, d2) of the unpruned float64 search on the rounded coordinates, T0 = I"""
    Q, P, _ = threshold_case(base)
    return O.nearest_full(Q.astype(np.float64), O.transform(P.astype(np.float64), np.eye(3), np.zeros(3)), THR_DIST)


# ---- wall --------------------------------------------------------------------------------------------------------------------------------
WALL_DIST, WALL_ITER = 0.1, 12
WALL_SEEDS = (4, 7, 13)                            # of seeds 0..15, three whose oracle run passes through det(U V^T) = -1: from the third iteration
                                                   # on, in every iteration, in the second and third only (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def wall_pair(seed):
    """Two scans of the square [-1,1]^2, 1200 and (its first) 960 points, each with its own 3 mm Gaussian noise along the normal, tilted;
    -> (target float32, source float32, T_gt, T0) with target ~ source R_gt^T + t_gt."""
    rng = np.random.default_rng([int(seed), 0x3a11])
    xy = rng.uniform(-1, 1, (1200, 2))
    views = [np.concatenate([xy, rng.normal(0, 0.003, (1200, 1))], 1) for _ in range(2)]
    tilt = synth.dense_gt(33.0, (2.0, -1.0, 0.5), (0, 0, 0))[:3, :3]
    Tg = O.perturb(np.eye(4), 4.0, 0.05, seed)
    tgt = views[0] @ tilt.T
    src = (views[1][:960] @ tilt.T - Tg[:3, 3]) @ Tg[:3, :3]
    return tgt.astype(np.float32), src.astype(np.float32), Tg, O.perturb(Tg, 1.0, 0.02, seed + 100)


def det_signs(Q, P, T0, d, max_iter):
    """sign det(U V^T) of every iteration the oracle executes and solves (O.icp's loop with the solve's factors kept)"""
    Q = np.asarray(Q, np.float32).astype(np.float64); P = np.asarray(P, np.float32).astype(np.float64)
    R, t = T0[:3, :3].copy(), T0[:3, 3].copy()
    signs = []
    for _ in range(max_iter):
        it = O.iterate(Q, P, R, t, d)
        Rn, tn, S, sign = O.solve_full(it['H'], it['cq'], it['cp']) if it['n'] >= 3 else (None, None, None, 0.0)
        if Rn is None:
            break
        signs.append(sign)
        done = O.rotation_step_deg(Rn, R) < 1e-4 and np.sqrt(((tn - t) ** 2).sum()) < 1e-6
        R, t = Rn, tn
        if done:
            break
    return signs


@functools.lru_cache(maxsize=None)
def wall_reference(seed):
    q, p, _, T0 = wall_pair(seed)
    return O.icp(q, p, T0, WALL_DIST, max_iter=WALL_ITER)
