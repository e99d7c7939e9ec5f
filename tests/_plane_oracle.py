"""The numpy restatement of the RANSAC plane segmentation (include/roreg_hip.h "v6t", csrc/plane.hip), twice: `segment` / `score` vectorised
over hypotheses and rows, `segment_loops` / `score_loops` as literal loops over Python integers and floats.  Both follow the header's
operation order; numpy's elementwise products and sums are separately rounded float64 operations (no FMA), and so are Python's.  No GPU imports."""
from collections import namedtuple
import math

import numpy as np

Planes = namedtuple('Planes', 'labels n_planes counts triples raw fit rms lam hyp_triples hyp_counts')
Planes.__doc__ = ('labels int32 [n], n_planes int, counts int32 [K], triples int32 [K,3], raw float64 [K,4], fit float64 [K,4], rms float64 [K] as the '
                  'header defines them; lam float64 [K,3]: the ascending eigenvalues of each plane\'s inlier covariance; hyp_triples int32 [H,3] / '
                  'hyp_counts int32 [H]: round 0\'s triples (original rows; -1 where two indices were equal or fewer than 3 rows were live) and counts')

MASK = (1 << 64) - 1
C0, C1, C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
HYP_BLOCK = 64           # hypotheses per block of the vectorised support matrix


def widen(p):
    """float32 [n,3] -> float64 [n,3] (exact)"""
    return np.ascontiguousarray(p, np.float32).astype(np.float64).reshape(-1, 3)


# ---- draws ------------------------------------------------------------------------------------------------------------------------------------
def mix_int(x):
    x = (x + C0) & MASK
    x = ((x ^ (x >> 30)) * C1) & MASK
    x = ((x ^ (x >> 27)) * C2) & MASK
    return x ^ (x >> 31)


def draw_int(seed, r, h, j, L):
    base = mix_int(seed ^ (r << 32))
    w = mix_int((base + 3 * h + j) & MASK)
    return ((w >> 32) * L) >> 32


def mix(x):
    """uint64 arrays; numpy's unsigned array arithmetic wraps mod 2^64"""
    x = x + np.uint64(C0)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(C1)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(C2)
    return x ^ (x >> np.uint64(31))


def draws(seed, r, H, L):
    """-> int64 [H,3]: the live-row numbers of every hypothesis of round r"""
    base = mix(np.array([(seed ^ (r << 32)) & MASK], np.uint64))
    k = np.uint64(3) * np.arange(H, dtype=np.uint64)[:, None] + np.arange(3, dtype=np.uint64)[None, :]
    w = mix(base + k)
    return (((w >> np.uint64(32)) * np.uint64(L)) >> np.uint64(32)).astype(np.int64)


# ---- planes and support -------------------------------------------------------------------------------------------------------------------------
def planes_of(A, B, C):
    """float64 [H,3] each -> (normals [H,3], q [H], valid [H])"""
    e1, e2 = B - A, C - A
    nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    q = (nx * nx + ny * ny) + nz * nz
    return np.stack([nx, ny, nz], 1), q, (q != 0.0) & np.isfinite(q)


def support(N, A, thr, X):
    """normals [H,3], anchors [H,3], thresholds [H], rows [L,3] -> bool [H,L]: s s <= thr"""
    out = np.zeros((N.shape[0], X.shape[0]), bool)
    for h0 in range(0, N.shape[0], HYP_BLOCK):
        n, a = N[h0:h0 + HYP_BLOCK], A[h0:h0 + HYP_BLOCK]
        dx, dy, dz = (X[None, :, k] - a[:, None, k] for k in range(3))
        s = (n[:, None, 0] * dx + n[:, None, 1] * dy) + n[:, None, 2] * dz
        out[h0:h0 + HYP_BLOCK] = s * s <= thr[h0:h0 + HYP_BLOCK, None]
    return out


def counts_of(N, A, thr, X):
    out = np.zeros(N.shape[0], np.int64)
    for h0 in range(0, N.shape[0], HYP_BLOCK):
        out[h0:h0 + HYP_BLOCK] = support(N[h0:h0 + HYP_BLOCK], A[h0:h0 + HYP_BLOCK], thr[h0:h0 + HYP_BLOCK], X).sum(1)
    return out


def threshold(dist, q):
    d2 = float(dist) * float(dist)
    return d2 * q


def fit_of(X, a, raw_n):
    """The least-squares plane through the rows X [m,3] (float64), moments taken about a: -> (fit [4], rms, ascending eigenvalues [3])"""
    d = X - a
    m = d.mean(0)
    c = d - m
    lam, V = np.linalg.eigh(c.T @ c / X.shape[0])
    n = V[:, 0] / np.sqrt((V[:, 0] ** 2).sum())
    if (n * raw_n).sum() < 0.0:
        n = -n
    cen = a + m
    dist = (X - cen) @ n
    return np.array([n[0], n[1], n[2], -(n * cen).sum()]), float(np.sqrt((dist * dist).mean())), lam


def _empty(n, K, H):
    return dict(labels=np.full(n, -1, np.int32), counts=np.zeros(K, np.int32), triples=np.full((K, 3), -1, np.int32), raw=np.zeros((K, 4)), fit=np.zeros((K, 4)),
                rms=np.zeros(K), lam=np.zeros((K, 3)), hyp_triples=np.full((H, 3), -1, np.int32), hyp_counts=np.full(H, -1, np.int32))


def segment(points, dist, n_hyp, max_planes, min_inliers, seed):
    X = widen(points)
    n, H, K = X.shape[0], int(n_hyp), int(max_planes)
    o = _empty(n, K, H)
    alive = np.isfinite(X).all(1)
    n_planes = 0
    for r in range(K):
        live = np.flatnonzero(alive & (o['labels'] < 0))
        L = live.shape[0]
        if L < 3:
            break
        idx = draws(seed, r, H, L)
        distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
        rows = live[idx]
        N, q, ok = planes_of(X[rows[:, 0]], X[rows[:, 1]], X[rows[:, 2]])
        valid = distinct & ok
        cnt = np.full(H, -1, np.int64)
        A = X[rows[:, 0]]
        thr = threshold(dist, q)
        cnt[valid] = counts_of(N[valid], A[valid], thr[valid], X[live])
        if r == 0:
            o['hyp_triples'][:] = np.where(distinct[:, None], rows, -1)
            o['hyp_counts'][:] = cnt
        if not valid.any():
            break
        h = int(np.argmax(cnt))                                   # the first of the greatest: the lowest h
        if cnt[h] < min_inliers:
            break
        inl = live[support(N[h:h + 1], A[h:h + 1], thr[h:h + 1], X[live])[0]]
        o['labels'][inl] = r
        o['counts'][r] = cnt[h]
        o['triples'][r] = rows[h]
        o['raw'][r] = [N[h, 0], N[h, 1], N[h, 2], -((N[h, 0] * A[h, 0] + N[h, 1] * A[h, 1]) + N[h, 2] * A[h, 2])]
        o['fit'][r], o['rms'][r], o['lam'][r] = fit_of(X[inl], A[h], N[h])
        n_planes = r + 1
    return Planes(n_planes=n_planes, **o)


def score(points, triples, dist):
    """hip.plane_score in numpy: triples int [H,3] of original rows -> counts int32 [H]"""
    X = widen(points)
    n = X.shape[0]
    T = np.asarray(triples, np.int64).reshape(-1, 3)
    out = np.full(T.shape[0], -1, np.int32)
    alive = np.isfinite(X).all(1)
    ok = ((T >= 0) & (T < n)).all(1) & (T[:, 0] != T[:, 1]) & (T[:, 0] != T[:, 2]) & (T[:, 1] != T[:, 2])
    ok[ok] = alive[T[ok]].all(1)
    if not ok.any():
        return out
    Tk = T[ok]
    N, q, valid = planes_of(X[Tk[:, 0]], X[Tk[:, 1]], X[Tk[:, 2]])
    cnt = np.full(Tk.shape[0], -1, np.int64)
    cnt[valid] = counts_of(N[valid], X[Tk[valid, 0]], threshold(dist, q[valid]), X[alive])
    out[ok] = cnt
    return out


# ---- the literal loops ----------------------------------------------------------------------------------------------------------------------------
def _plane_loop(a, b, c):
    e1 = [b[k] - a[k] for k in range(3)]
    e2 = [c[k] - a[k] for k in range(3)]
    nx = e1[1] * e2[2] - e1[2] * e2[1]
    ny = e1[2] * e2[0] - e1[0] * e2[2]
    nz = e1[0] * e2[1] - e1[1] * e2[0]
    q = (nx * nx + ny * ny) + nz * nz
    return nx, ny, nz, q, q != 0.0 and math.isfinite(q)


def _inlier_loop(nx, ny, nz, a, thr, p):
    s = (nx * (p[0] - a[0]) + ny * (p[1] - a[1])) + nz * (p[2] - a[2])
    return s * s <= thr


def _rows_as_floats(points):
    return [[float(v) for v in row] for row in widen(points)]


def segment_loops(points, dist, n_hyp, max_planes, min_inliers, seed):
    """-> (labels, n_planes, counts, triples, raw, round-0 hypothesis counts) as Python lists: the definition read out loud"""
    P = _rows_as_floats(points)
    n = len(P)
    dead = [not all(math.isfinite(v) for v in p) for p in P]
    labels = [-1] * n
    counts, triples, raw, hyp0 = [0] * max_planes, [[-1, -1, -1] for _ in range(max_planes)], [[0.0] * 4 for _ in range(max_planes)], [-1] * n_hyp
    n_planes = 0
    d2 = float(dist) * float(dist)
    for r in range(max_planes):
        live = [i for i in range(n) if not dead[i] and labels[i] < 0]
        L = len(live)
        if L < 3:
            break
        best, best_h, best_plane = -1, -1, None
        for h in range(n_hyp):
            i0, i1, i2 = (draw_int(seed, r, h, j, L) for j in range(3))
            cnt = -1
            if i0 != i1 and i0 != i2 and i1 != i2:
                a, b, c = P[live[i0]], P[live[i1]], P[live[i2]]
                nx, ny, nz, q, ok = _plane_loop(a, b, c)
                if ok:
                    thr = d2 * q
                    cnt = 0
                    for i in live:
                        if _inlier_loop(nx, ny, nz, a, thr, P[i]):
                            cnt += 1
                    if cnt > best:                               # strictly: among equal counts the lowest h stays
                        best, best_h, best_plane = cnt, h, (nx, ny, nz, a, thr, [live[i0], live[i1], live[i2]])
            if r == 0:
                hyp0[h] = cnt
        if best_h < 0 or best < min_inliers:
            break
        nx, ny, nz, a, thr, rows = best_plane
        for i in live:
            if _inlier_loop(nx, ny, nz, a, thr, P[i]):
                labels[i] = r
        counts[r], triples[r] = best, rows
        raw[r] = [nx, ny, nz, -((nx * a[0] + ny * a[1]) + nz * a[2])]
        n_planes = r + 1
    return labels, n_planes, counts, triples, raw, hyp0


def score_loops(points, triples, dist):
    P = _rows_as_floats(points)
    n = len(P)
    dead = [not all(math.isfinite(v) for v in p) for p in P]
    d2 = float(dist) * float(dist)
    out = []
    for t in triples:
        t = [int(v) for v in t]
        cnt = -1
        if all(0 <= v < n for v in t) and len(set(t)) == 3 and not any(dead[v] for v in t):
            nx, ny, nz, q, ok = _plane_loop(P[t[0]], P[t[1]], P[t[2]])
            if ok:
                thr = d2 * q
                cnt = sum(1 for i in range(n) if not dead[i] and _inlier_loop(nx, ny, nz, P[t[0]], thr, P[i]))
        out.append(cnt)
    return out


# ---- helpers of the tests --------------------------------------------------------------------------------------------------------------------------
def unit(planes):
    """[k,4] -> the same planes with unit normals"""
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    return planes / np.sqrt((planes[:, :3] ** 2).sum(1, keepdims=True))


def axis_angle_deg(normal):
    """the angle between a normal and the nearest coordinate axis, in degrees, and that axis"""
    u = np.abs(np.asarray(normal, np.float64)) / np.sqrt((np.asarray(normal, np.float64) ** 2).sum())
    k = int(np.argmax(u))
    return float(np.degrees(np.arccos(min(1.0, u[k])))), k


def gap_ratio(lam):
    """(lambda_mid - lambda_min) / lambda_max of ascending eigenvalues [k,3]"""
    lam = np.asarray(lam, np.float64).reshape(-1, 3)
    return (lam[:, 1] - lam[:, 0]) / lam[:, 2]
