"""The definition of roreg_grid_knn (include/roreg_hip.h "v6q") and of the outlier filters built on it, restated in numpy.  No GPU imports.

Coordinates are float32 values widened to float64.  For query x and cloud row j: dx = x_j.x - x.x, dy, dz likewise (exact), d2 = (dx dx + dy dy)
+ dz dz in float64 (numpy has no FMA).  Row j is a candidate iff it is not the query's excluded row and d2 <= r * r; candidates are ordered by
(d2, j) ascending.  count = the number of candidates (not capped); idx / d2 = the first f = min(k, count) of them, then -1 / +inf; mean_dist =
(((sqrt(d2_0) + sqrt(d2_1)) + sqrt(d2_2)) ...) / f, +inf when f == 0."""
from collections import namedtuple

import numpy as np

Knn = namedtuple('Knn', 'idx d2 count mean')
CHUNK = 512


def widen(p):
    p = np.asarray(p)
    assert p.dtype == np.float32
    return p.astype(np.float64).reshape(-1, 3)


def _mean(d2, f):
    """sqrt of the listed entries summed in list order, divided by their number"""
    m, k = d2.shape
    s = np.zeros(m)
    for t in range(k):
        held = t < f
        s = np.where(held, s + np.sqrt(np.where(held, d2[:, t], 0.0)), s)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(f > 0, s / f, np.inf)


def knn(points, k, radius, queries=None, self_rows=None):
    """-> Knn(idx int32 [m,k], d2 f64 [m,k], count int32 [m], mean f64 [m]).  radius=np.inf: the brute-force k nearest."""
    X = widen(points)
    n = X.shape[0]
    if queries is None:
        assert self_rows is None
        Q, excl = X, np.arange(n)
    else:
        Q = widen(queries)
        excl = np.full(Q.shape[0], -1) if self_rows is None else np.asarray(self_rows).astype(np.int64)
    m = Q.shape[0]
    thr2 = np.float64(radius) * np.float64(radius)
    idx = np.full((m, k), -1, np.int32); d2o = np.full((m, k), np.inf); count = np.zeros(m, np.int32)
    for a in range(0, m if n else 0, CHUNK):
        q = Q[a:a + CHUNK]
        dx, dy, dz = (X[None, :, c] - q[:, None, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        cand = d2 <= thr2
        rows = np.arange(q.shape[0])
        e = excl[a:a + CHUNK]
        cand[rows[e >= 0], e[e >= 0]] = False
        count[a:a + CHUNK] = cand.sum(1)
        key = np.where(cand, d2, np.inf)
        kk = min(k, n)
        order = np.argsort(key, axis=1, kind='stable')[:, :kk]           # stable: among equal d2 the lower row first
        dsel = np.take_along_axis(key, order, 1)
        held = np.arange(kk)[None, :] < np.minimum(count[a:a + CHUNK], k)[:, None]
        idx[a:a + CHUNK, :kk] = np.where(held, order, -1)
        d2o[a:a + CHUNK, :kk] = np.where(held, dsel, np.inf)
    return Knn(idx, d2o, count, _mean(d2o, np.minimum(count, k)))


def knn_loops(points, k, radius, queries=None, self_rows=None):
    """The same definition as a plain double loop (small inputs only): what the vectorised form is checked against."""
    X = widen(points)
    Q = X if queries is None else widen(queries)
    n, m = X.shape[0], Q.shape[0]
    thr2 = float(radius) * float(radius)
    idx = np.full((m, k), -1, np.int32); d2o = np.full((m, k), np.inf); count = np.zeros(m, np.int32); mean = np.full(m, np.inf)
    for i in range(m):
        excl = i if queries is None else (-1 if self_rows is None else int(self_rows[i]))
        cand = []
        for j in range(n):
            if j == excl:
                continue
            dx, dy, dz = X[j, 0] - Q[i, 0], X[j, 1] - Q[i, 1], X[j, 2] - Q[i, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= thr2:
                cand.append((d2, j))
        cand.sort()
        count[i] = len(cand)
        s = 0.0
        for t, (d2, j) in enumerate(cand[:k]):
            idx[i, t], d2o[i, t] = j, d2
            s = s + np.sqrt(d2)
        if cand:
            mean[i] = s / min(k, len(cand))
    return Knn(idx, d2o, count, mean)


Statistical = namedtuple('Statistical', 'score T mask')


def statistical(points, nb_neighbors, std_ratio):
    """score = the mean distance to the exact min(nb_neighbors, n - 1) nearest other rows; T = mean + std_ratio * SAMPLE standard deviation;
    keep iff score <= T.  Fewer than 2 points: kept whole (T = +inf)."""
    n = np.asarray(points).reshape(-1, 3).shape[0]
    if n < 2:
        return Statistical(np.full(n, np.inf), np.inf, np.ones(n, bool))
    score = knn(points, nb_neighbors, np.inf).mean
    T = score.mean() + float(std_ratio) * score.std(ddof=1)
    return Statistical(score, float(T), score <= T)


def radius_mask(points, radius, min_neighbors):
    count = knn(points, 1, radius).count
    return count, count >= int(min_neighbors)
