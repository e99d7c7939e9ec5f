"""The definition of roreg_fps_batch (include/roreg_hip.h "v6s") restated in numpy, twice: fps() one vector operation
per step, fps_loops() a literal double loop.  No GPU imports.

Coordinates are float32 values widened to float64; d2(i, j) = (dx dx + dy dy) + dz dz.  A row with a non-finite coordinate is dead.  D = +inf
for every live row.  Step 0 selects `start`, or the lowest live row when start is dead; step s >= 1 selects the live row not yet taken of
greatest D, the lowest row among equal D; after a selection c, D[i] = min(D[i], d2(i, c)).  Taken rows are excluded by a flag.  The selection
ends when k rows are selected, when no live row is left, or when (s >= 1) the candidate's D < stop2."""
from collections import namedtuple

import numpy as np

Fps = namedtuple('Fps', 'rows dist2 count tied')
Fps.__doc__ = ('rows int32 [k] (-1 behind count), dist2 float64 [k] (0 behind count), count int, tied int64 [k]: the number of candidates that held the '
               'selected row\'s D at step s (the lowest of them was selected), 0 behind count')


def widen(points):
    return np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)


def _d2(p, c):
    with np.errstate(invalid='ignore', over='ignore'):
        d = p - c
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fps(points, k, start=0, stop2=0.0):
    p = widen(points)
    n, k = p.shape[0], int(k)
    rows, dist2, tied = np.full(k, -1, np.int32), np.zeros(k, np.float64), np.zeros(k, np.int64)
    if n == 0 or k == 0:
        return Fps(rows, dist2, 0, tied)
    assert 0 <= start < n and stop2 >= 0.0
    live = np.isfinite(p).all(1)
    taken = np.zeros(n, bool)
    D = np.where(live, np.inf, np.nan)
    count = 0
    for s in range(k):
        cand = live & ~taken
        if not cand.any():
            break
        if s == 0:
            c = int(start) if live[start] else int(np.nonzero(live)[0][0])
        else:
            c = int(np.argmax(np.where(cand, D, -1.0)))          # the first of the greatest: the lowest row
            if D[c] < stop2:
                break
        rows[s], dist2[s], tied[s] = c, D[c], int((cand & (D == D[c])).sum())
        taken[c] = True
        count += 1
        D = np.where(live, np.minimum(D, _d2(p, p[c])), D)
    return Fps(rows, dist2, count, tied)


def fps_loops(points, k, start=0, stop2=0.0):
    """the same, row by row"""
    p = [tuple(float(v) for v in r) for r in widen(points)]
    n, k = len(p), int(k)
    rows, dist2, tied = [-1] * k, [0.0] * k, [0] * k
    live = [all(np.isfinite(v) for v in r) for r in p]
    taken = [False] * n
    D = [float('inf')] * n
    count = 0
    for s in range(k):
        best, best_d, ties = -1, -1.0, 0
        for i in range(n):
            if not live[i] or taken[i]:
                continue
            if s == 0:
                key = 2.0 if i == start else 1.0                 # start before every other live row, then the lowest row
            else:
                key = D[i]
            if key > best_d:
                best, best_d, ties = i, key, 1
            elif key == best_d:
                ties += 1
        if best < 0:
            break
        if s == 0:
            ties = sum(1 for i in range(n) if live[i])
        elif D[best] < stop2:
            break
        rows[s], dist2[s], tied[s] = best, D[best], ties
        taken[best] = True
        count += 1
        cx, cy, cz = p[best]
        for i in range(n):
            if live[i]:
                dx, dy, dz = p[i][0] - cx, p[i][1] - cy, p[i][2] - cz
                d2 = (dx * dx + dy * dy) + dz * dz
                if d2 < D[i]:
                    D[i] = d2
    return Fps(np.array(rows, np.int32).reshape(k), np.array(dist2, np.float64).reshape(k), count, np.array(tied, np.int64).reshape(k))
