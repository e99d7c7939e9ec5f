"""The definition of roreg_grid_dbscan (include/roreg_hip.h "v6r") and of the cluster filter built on it, restated in
numpy, in two independent forms.  No GPU imports.

Coordinates are float32 values widened to float64.  d2 = (dx dx + dy dy) + dz dz in float64 (numpy has no FMA); rows i and j are neighbours iff
d2 <= eps * eps.  count_i = the rows within eps of row i, itself included (a duplicated point counts); row i is core iff count_i >= min_points.
A cluster is a connected component of the graph on core rows whose edges join core rows that are neighbours.  A non-core row with a core
neighbour is a border row and belongs to the cluster of the core neighbour first in (d2, row) order.  Every other row is noise, label -1.
Clusters are numbered 0..C-1 by ascending lowest core row.  sizes[c] counts core and border rows; entries behind C - 1 are 0.

Both forms return Clusters(labels int32 [n], core uint8 [n], sizes int32 [n], n_border); n_clusters is labels.max() + 1."""
from collections import namedtuple

import numpy as np

Clusters = namedtuple('Clusters', 'labels core sizes n_border')


def widen(p):
    p = np.asarray(p)
    assert p.dtype == np.float32
    return p.astype(np.float64).reshape(-1, 3)


def n_clusters(res):
    return int(res.labels.max()) + 1 if res.labels.shape[0] else 0


def _d2(A, B):
    dx, dy, dz = B[..., 0] - A[..., 0], B[..., 1] - A[..., 1], B[..., 2] - A[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def pairs(X, eps):
    """Every ordered pair (i, j), i == j included, with d2 <= eps^2 -> (i, j, d2), from a sort by cell.  The cells are a little wider than
    eps, so two neighbours are never more than one cell apart on an axis (the rounding of the cell arithmetic is far below the margin)."""
    n = X.shape[0]
    h = float(eps) * (1.0 + 1e-6)
    c = np.floor((X - X.min(0)) / h).astype(np.int64) + 1
    dims = c.max(0) + 2
    key = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    order = np.argsort(key, kind='stable')
    sk = key[order]
    thr2 = np.float64(eps) * np.float64(eps)
    I, J, D = [], [], []
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for oz in (-1, 0, 1):
                t = key + (ox * dims[1] + oy) * dims[2] + oz
                lo, hi = np.searchsorted(sk, t, 'left'), np.searchsorted(sk, t, 'right')
                cnt = hi - lo
                i = np.repeat(np.arange(n), cnt)
                within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                j = order[np.repeat(lo, cnt) + within]
                d2 = _d2(X[i], X[j])
                keep = d2 <= thr2
                I.append(i[keep]); J.append(j[keep]); D.append(d2[keep])
    return np.concatenate(I), np.concatenate(J), np.concatenate(D)


def _finish(n, root, core):
    """root int [n]: the lowest core row of the row's cluster, -1 for noise -> Clusters"""
    roots = np.unique(root[root >= 0])
    labels = np.where(root >= 0, np.searchsorted(roots, np.maximum(root, 0)), -1).astype(np.int32)
    sizes = np.bincount(labels[labels >= 0], minlength=n).astype(np.int32)[:n] if n else np.zeros(0, np.int32)
    return Clusters(labels, core.astype(np.uint8), sizes, int(((labels >= 0) & ~core).sum()))


def dbscan(points, eps, min_points):
    """The vectorised form: the pair list from a cell sort, then min-label propagation with pointer jumping to the fixed point."""
    X = widen(points)
    n = X.shape[0]
    if n == 0:
        return Clusters(np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.int32), 0)
    i, j, d2 = pairs(X, eps)
    core = np.bincount(i, minlength=n) >= int(min_points)
    cc = core[i] & core[j]
    ei, ej = i[cc], j[cc]
    lab = np.arange(n)
    while True:
        new = lab.copy()
        np.minimum.at(new, ei, lab[ej])                  # a row takes the lowest label among its neighbours ...
        np.minimum.at(new, lab[ei], lab[ej])             # ... and so does the row its label names
        while True:                                      # pointer jumping: labels are rows, follow them to where they end
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    root = np.where(core, lab, -1)
    b = ~core[i] & core[j]                               # border candidates: (non-core row, core neighbour)
    bi, bj, bd = i[b], j[b], d2[b]
    o = np.lexsort((bj, bd, bi))                         # by row, then d2, then neighbour row
    bi, bj = bi[o], bj[o]
    first = np.ones(bi.shape[0], bool)
    first[1:] = bi[1:] != bi[:-1]
    root[bi[first]] = lab[bj[first]]
    return _finish(n, root, core)


def dbscan_loops(points, eps, min_points):
    """The literal form: every row's ball by brute force, clusters grown breadth-first from the core rows in ascending row order."""
    X = widen(points)
    n = X.shape[0]
    thr2 = float(eps) * float(eps)
    ball, dist = [], []
    for r in range(n):
        d2 = _d2(X[r], X)
        nb = np.nonzero(d2 <= thr2)[0]
        ball.append(nb); dist.append(d2[nb])
    core = np.array([len(b) >= int(min_points) for b in ball], bool).reshape(n)
    root = np.full(n, -1)
    for seed in range(n):
        if not core[seed] or root[seed] >= 0:
            continue
        root[seed] = seed                                # the lowest core row of a cluster not seen before
        queue = [seed]
        while queue:
            nxt = []
            for r in queue:
                for q in ball[r]:
                    if core[q] and root[q] < 0:
                        root[q] = seed
                        nxt.append(int(q))
            queue = nxt
    for r in range(n):
        if core[r]:
            continue
        cand = sorted((float(d), int(q)) for d, q in zip(dist[r], ball[r]) if core[q])
        if cand:
            root[r] = root[cand[0][1]]
    return _finish(n, root, core)


def cluster_mask(res, min_size=None, largest=False):
    """The cluster filter: keep a row iff its label is >= 0 and its cluster has at least min_size rows; largest=True: iff it is in the largest
    cluster (ties to the lower label).  -> (mask bool [n], score float64 [n]: the size of the row's cluster, 0 for noise)."""
    assert (min_size is None) == bool(largest)
    lab = res.labels.astype(np.int64)
    n = lab.shape[0]
    score = np.where(lab >= 0, res.sizes[np.maximum(lab, 0)] if n else 0, 0).astype(np.float64)
    if largest:
        return ((lab == int(np.argmax(res.sizes))) if n_clusters(res) else np.zeros(n, bool)), score
    return (lab >= 0) & (score >= int(min_size)), score
