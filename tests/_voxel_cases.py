"""Seeded input families of the voxel-grid tests (tests/test_voxel_oracle.py asserts on the CPU that each family reaches its branch,
tests/test_hip_voxel.py runs the same families on the device).  No GPU imports.

  lattice    -- per voxel size, float32(k v) and its two float32 neighbours for k in -4000..3999 (24000 values per axis pattern), +-0.0,
                keys at -2^20 and 2^20 - 1; a float32 division would move more than 1000 of them to another voxel;
  sizes      -- n around a wave, a workgroup and one scan block; one point per voxel (17^3 lattice); 3000 points in one voxel;
  structured -- 4096 voxels in a line along each axis, a 64 x 64 plane, keys that differ only in the top bits of one axis;
  room       -- the six faces of a 4 x 3 x 2.5 m box with 3 mm noise, centred on the origin;
  order      -- voxels whose ascending sequential float64 sum differs from the descending sum and from a pairwise tree;
  outlier    -- a room plus one point at (2e4, -2e4, 1e4)."""
import functools

import numpy as np

LATTICE_VOXELS = (0.25, 0.025, 0.05, 0.15)
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
SIZES_VOXEL = 0.1
ROOM_N, ROOM_VOXELS = 30000, (0.025, 0.05, 0.1)
ROOM_EXPECT = {0.025: (27611, 4), 0.05: (21909, 6), 0.1: (8817, 15)}        # voxel -> (m, maximum occupancy)
KEY_LIM = 1 << 20


def lattice_values(v):
    """The 24000 values of one axis pattern: float32(k v) and its two float32 neighbours, k = -4000..3999."""
    c = (np.arange(-4000, 4000, dtype=np.float64) * v).astype(np.float32)
    return np.concatenate((np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))))


def lattice(v):
    """-> float32 [n,3]: the family's values (lattice_values, +-0.0, the two edge keys) on each axis in turn, the other two axes held in the
    middle of a voxel, so that a value and its neighbours share a voxel or do not by their own key alone; rows shuffled."""
    vals = np.concatenate((lattice_values(v), np.array([0.0, -0.0], np.float32), edge_values(v)))
    rest = (np.float32(0.5 * v), np.float32(-0.5 * v))
    rows = []
    for a in range(3):
        q = np.empty((vals.shape[0], 3), np.float32)
        q[:, a], q[:, (a + 1) % 3], q[:, (a + 2) % 3] = vals, rest[0], rest[1]
        rows.append(q)
    p = np.concatenate(rows)
    return np.ascontiguousarray(p[np.random.default_rng(int(round(v * 1000))).permutation(p.shape[0])], np.float32)


def edge_values(v):
    """float32 values whose keys are exactly -2^20 and 2^20 - 1 (both valid)."""
    lo = np.float32(-KEY_LIM * v)
    while np.floor(np.float64(lo) / v) < -KEY_LIM:
        lo = np.nextafter(lo, np.float32(np.inf))
    hi = np.float32(KEY_LIM * v)
    while np.floor(np.float64(hi) / v) >= KEY_LIM:
        hi = np.nextafter(hi, np.float32(-np.inf))
    return np.array([lo, hi], np.float32)


def beyond_value(v):
    """The smallest float32 whose key is 2^20: one row of it must raise."""
    hi = edge_values(v)[1]
    while np.floor(np.float64(hi) / v) < KEY_LIM:
        hi = np.nextafter(hi, np.float32(np.inf))
    return hi


def cube(n, seed=0):
    return np.random.default_rng(1000 + seed + n).random((n, 3)).astype(np.float32)


def all_distinct():
    """17^3 points, one per voxel of edge 0.1, shuffled."""
    g = np.stack(np.meshgrid(*[np.arange(17)] * 3, indexing='ij'), -1).reshape(-1, 3)
    rng = np.random.default_rng(17)
    return ((g[rng.permutation(g.shape[0])] + 0.5) * 0.1).astype(np.float32), 0.1


def one_voxel():
    return (0.3 + 0.09 * np.random.default_rng(18).random((3000, 3))).astype(np.float32), 0.1


def structured(name, v=0.05):
    """-> float32 [n,3], 1 to 3 points per voxel, rows shuffled."""
    if name in ('line_x', 'line_y', 'line_z'):
        K = np.zeros((4096, 3), np.int64)
        K[:, 'xyz'.index(name[-1])] = np.arange(4096) - 2048
    elif name == 'plane':
        K = np.zeros((4096, 3), np.int64)
        K[:, 0], K[:, 2] = np.divmod(np.arange(4096), 64)
        K[:, 1] = 7
    elif name == 'top_bits':
        K = np.zeros((256, 3), np.int64)
        K[:, 1] = (np.arange(256) - 128) * 4096
        K[:, 0], K[:, 2] = -3, 5
    else:
        raise KeyError(name)
    rng = np.random.default_rng(sum(name.encode()))
    K = np.repeat(K, rng.integers(1, 4, K.shape[0]), 0)
    p = (K + 0.25 + 0.5 * rng.random(K.shape)) * v
    return np.ascontiguousarray(p[rng.permutation(p.shape[0])], np.float32)


STRUCTURED = ('line_x', 'line_y', 'line_z', 'plane', 'top_bits')


@functools.lru_cache(maxsize=None)
def room(n=ROOM_N, seed=4):
    """The six faces of a 4 x 3 x 2.5 m box centred on the origin, 3 mm noise."""
    rng = np.random.default_rng(seed)
    half = np.array([2.0, 1.5, 1.25])
    p = (rng.random((n, 3)) * 2.0 - 1.0) * half
    face = rng.integers(0, 6, n)
    ax, side = face // 2, (face % 2) * 2.0 - 1.0
    p[np.arange(n), ax] = side * half[ax]
    p += 0.003 * rng.standard_normal((n, 3))
    return np.ascontiguousarray(p, np.float32)


ORDER_T, ORDER_B = 2.0 ** -57, np.float32(0.2)


def order_rows():
    """One voxel's rows along one axis: (t, t, b, t, t, t, t), all inside [0, 0.25)."""
    t = np.float32(ORDER_T)
    return np.array([t, t, ORDER_B, t, t, t, t], np.float32)


def tree_sum(x):
    x = [float(v) for v in x]
    while len(x) > 1:
        x = [x[i] + x[i + 1] if i + 1 < len(x) else x[i] for i in range(0, len(x), 2)]
    return x[0]


def order_cloud(seed=9):
    """-> (float32 [n,3], voxel 0.25, the rows of the 200 special voxels as int [200,7]): 200 voxels that each hold order_rows() in x and z
    (keys 0) and sit at y key 100 + j, mixed among 5000 ordinary points in [-2, 2)^3 (keys -8..7), the special rows keeping their order."""
    rng = np.random.default_rng(seed)
    r = order_rows()
    special = []
    for j in range(200):
        q = np.stack((r, r, r), 1).astype(np.float64)
        q[:, 1] += 0.25 * (100 + j)                 # a voxel of its own: y key 100 + j (x and z carry the summation order)
        special.append(q)
    special = np.concatenate(special).astype(np.float32)
    ordinary = (rng.random((5000, 3)) * 4.0 - 2.0).astype(np.float32)
    n = special.shape[0] + ordinary.shape[0]
    pos = np.sort(rng.permutation(n)[:special.shape[0]])          # where the special rows go, in their own order
    out = np.empty((n, 3), np.float32)
    mask = np.zeros(n, bool); mask[pos] = True
    out[mask] = special
    out[~mask] = ordinary
    return out, 0.25, pos.reshape(200, 7)


def outlier_cloud():
    return np.ascontiguousarray(np.concatenate((room(5000, 6), np.array([[2e4, -2e4, 1e4]], np.float32))), np.float32), 0.025
