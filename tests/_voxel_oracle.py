"""Numpy restatement of the voxel-grid downsampling (roreg_amd/csrc/voxel.hip; include/roreg_hip.h "v6e"): the device must equal it exactly.

  key      per axis k = floor(float64(x) / voxel) on the float32-rounded coordinates: one IEEE float64 division (the reference's
           np.floor(xyz / voxel_size), testset.py); -0.0 falls in voxel 0; valid keys -2^20 <= k < 2^20;
  order    voxels are numbered 0..m-1 in ascending order of their lowest original row;
  outputs  coords int32 [m,3], first int32 [m] (lowest original row, strictly ascending), counts int32 [m], inverse int32 [n],
           centroid float64 [m,3] = (the members' float64 coordinates added sequentially in ascending original row, starting from the
           first member) / count, points float32 [m,3] = the centroid rounded once to float32 ('centroid') or points[first] ('first').
np.unique on the integer keys gives the voxels, np.add.at adds sequentially in index order (tests/test_voxel_oracle.py checks both against
a plain Python loop).  No GPU imports."""
from collections import namedtuple

import numpy as np

KEY_LIM = 1 << 20
Voxels = namedtuple('Voxels', 'points coords first counts inverse centroid')


class BadInput(ValueError):
    pass


def keys(points, voxel):
    """float32 [n,3] -> int64 [n,3] voxel coordinates; BadInput for a non-finite coordinate or a key outside [-2^20, 2^20)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    if not np.isfinite(p).all():
        raise BadInput('non-finite coordinate')
    K = np.floor(p.astype(np.float64) / np.float64(voxel))
    if not ((K >= -KEY_LIM) & (K < KEY_LIM)).all():
        raise BadInput('key out of range')
    return K.astype(np.int64)                      # -0.0 -> 0


def keys_float32(points, voxel):
    """What a float32 division would give (the shortcut the definition excludes): the lattice family must tell it apart."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return np.floor(p / np.float32(voxel)).astype(np.int64)


def downsample(points, voxel, mode='centroid'):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = p.shape[0]
    if n == 0:
        z = np.zeros((0, 3))
        return Voxels(z.astype(np.float32), z.astype(np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), z)
    K = keys(p, voxel)
    uniq, first, inverse, counts = np.unique(K, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind='stable')       # ascending lowest original row
    number = np.empty(order.shape[0], np.int64)
    number[order] = np.arange(order.shape[0])
    coords, first, counts, inverse = uniq[order], first[order], counts[order], number[inverse]
    p64 = p.astype(np.float64)
    s = p64[first].copy()                          # the sum starts from the first member ...
    rest = np.ones(n, bool)
    rest[first] = False
    np.add.at(s, inverse[rest], p64[rest])         # ... and adds the others one by one in ascending original row
    centroid = s / counts[:, None].astype(np.float64)
    pts = centroid.astype(np.float32) if mode == 'centroid' else p[first]
    return Voxels(pts, coords.astype(np.int32), first.astype(np.int32), counts.astype(np.int32), inverse.astype(np.int32), centroid)


def downsample_loop(points, voxel):
    """The same definition as a dict and a loop over the rows: what the vectorised form is checked against."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    table, coords, first, counts, sums, inverse = {}, [], [], [], [], []
    for i in range(p.shape[0]):
        x = [float(v) for v in p[i]]
        k = tuple(int(np.floor(v / float(voxel))) for v in x)
        v = table.get(k)
        if v is None:
            v = table[k] = len(coords)
            coords.append(k); first.append(i); counts.append(1); sums.append(list(x))
        else:
            counts[v] += 1
            for a in range(3):
                sums[v][a] = sums[v][a] + x[a]
        inverse.append(v)
    centroid = np.array([[s / c for s in row] for row, c in zip(sums, counts)], np.float64).reshape(-1, 3)
    return Voxels(centroid.astype(np.float32), np.array(coords, np.int32).reshape(-1, 3), np.array(first, np.int32), np.array(counts, np.int32),
                  np.array(inverse, np.int32), centroid)
