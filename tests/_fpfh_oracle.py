"""numpy restatement of the FPFH descriptor (include/roreg_hip.h "v6n"; roreg_amd/csrc/fpfh.hip, fpfh_math.h): what the
device must compute.  Stands alone: imports nothing of roreg_amd.  Every operation is float64 in the order written (no dot, no einsum, no
matmul): dot products are (a0 b0 + a1 b1) + a2 b2, cross products (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0).

  orientation  n_i <- -n_i iff n_i . (c - x_i) < 0 (a dot of exactly 0 keeps the sign; a zero row stays zero)
  pair (i, j)  contributes iff j != i, both normals valid, 0 < d2 = |x_j - x_i|^2 <= r r and |dp x na| != 0;
               d = sqrt(d2), a1 = n_i . dp / d, a2 = n_j . dp / d; |a1| < |a2|: (na, nb, dp, f3) = (n_j, n_i, -dp, -a2), else (n_i, n_j, dp, a1);
               v = dp x na / |dp x na|, w = na x v, f2 = v . nb, y = w . nb, x = na . nb
  bins         b2 = clamp(floor((11 (f2 + 1)) 0.5), 0, 10), b3 likewise of f3, b1 = bin of atan2(y, x) by half-plane tests (bin_angle)
  SPFH         count_i[33] (b1, 11 + b2, 22 + b3 once per contributing pair), m_i pairs, S_i = count_i (100 / m_i) or 0
  FPFH         W_i = sum_j S_j / d2_ij over j != i, 0 < d2 <= r r, m_j > 0; s_g = sum of W_i over third g (ascending bin);
               F_i = (s_g > 0 ? (100 W_i) / s_g : 0) + S_i; out = float32(F_i); row i valid iff m_i > 0, else 33 zeros.
`spfh` / `fpfh` visit, for a block of points, only the points inside the block's bounding box grown by r (every point they skip is farther than
r from every point of the block); spfh_loop / fpfh_loop are the plain double loops, tests/test_fpfh_oracle.py checks one against the other."""
import numpy as np

BINS, WIDTH = 11, 33
# cos and sin of theta_k = pi (2 k - 11) / 11, k = 6..10: the same digits as csrc/fpfh_math.h bin_angle
EDGE_C = (0.9594929736144974, 0.6548607339452851, 0.14231483827328512, -0.4154150130018863, -0.8412535328311811)
EDGE_S = (0.28173255684142967, 0.7557495743542583, 0.9898214418809327, 0.9096319953545184, 0.5406408174555978)


def widen(P):
    return np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def valid_normals(N):
    return (np.asarray(N)[:, :3] != 0).any(1)


def orient_flags(X, N, c):
    """-> bool [n]: the rows that are negated (c: one viewpoint, or one per row)"""
    return dot(np.asarray(N, np.float64)[:, :3], np.asarray(c, np.float64).reshape(-1, 3) - widen(X)) < 0.0


def orient(X, N, c):
    """N [n,3] or [n,4] -> the same table oriented towards c (further columns copied)"""
    out = np.array(N, np.float64)
    flip = orient_flags(X, out, c)
    out[flip, :3] = -out[flip, :3]
    return out


def bin_linear(f):
    return np.clip(np.floor((11.0 * (np.asarray(f, np.float64) + 1.0)) * 0.5), 0.0, 10.0).astype(np.int64)


def bin_angle(y, x):
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    up, z = y >= 0.0, -y
    n_up = np.zeros(y.shape, np.int64); n_dn = np.zeros(y.shape, np.int64)
    for c, s in zip(EDGE_C, EDGE_S):
        n_up += (c * y - s * x >= 0.0)
        n_dn += (c * z - s * x > 0.0)
    return np.where((x == 0.0) & (y == 0.0), 5, np.where(up, 5 + n_up, 5 - n_dn))


def bin_angle_atan2(y, x):
    """The transcendental form the half-plane rule replaces: clamp(floor(11 (atan2(y, x) + pi) / (2 pi)), 0, 10)"""
    return np.clip(np.floor(11.0 * (np.arctan2(y, x) + np.pi) / (2.0 * np.pi)), 0, 10).astype(np.int64)


def pair_feature(dp, d2, ni, nj):
    """Broadcast arrays [..., 3], d2 [...] > 0 -> (ok bool, y, x, f2, f3); where ok is False (no frame) the other values mean nothing."""
    with np.errstate(divide='ignore', invalid='ignore'):
        d = np.sqrt(d2)
        a1, a2 = dot(ni, dp) / d, dot(nj, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        s3 = swap[..., None]
        na, nb, p = np.where(s3, nj, ni), np.where(s3, ni, nj), np.where(s3, -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = cross(p, na)
        vn = np.sqrt(dot(v, v))
        ok = vn != 0.0
        v = v / vn[..., None]
        w = cross(na, v)
        return ok, dot(w, nb), dot(na, nb), dot(v, nb), f3


def pair_bins(dp, d2, ni, nj):
    """-> (ok, b1, b2, b3)"""
    ok, y, x, f2, f3 = pair_feature(dp, d2, ni, nj)
    y, x, f2, f3 = (np.where(ok, v, 0.0) for v in (y, x, f2, f3))
    return ok, bin_angle(y, x), bin_linear(f2), bin_linear(f3)


# ---- blocks of points against their pruned candidates ------------------------------------------------------------------------------------
def _blocks(X, r, block):
    """-> [(rows of the block, rows of its candidates)]: every point within r of a point of the block is among its candidates."""
    n = X.shape[0]
    order = np.argsort(X[:, 0], kind='stable')
    xs = X[order, 0]
    reach = r * (1.0 + 1e-9)
    cell = np.floor(X / max(2.0 * r, 1e-12))
    rows = np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))
    out = []
    for s in range(0, n, block):
        idx = rows[s:s + block]
        lo3, hi3 = X[idx].min(0) - reach, X[idx].max(0) + reach
        cand = order[np.searchsorted(xs, lo3[0], 'left'):np.searchsorted(xs, hi3[0], 'right')]
        keep = (X[cand, 1] >= lo3[1]) & (X[cand, 1] <= hi3[1]) & (X[cand, 2] >= lo3[2]) & (X[cand, 2] <= hi3[2])
        out.append((idx, np.sort(cand[keep])))
    return out


def _offsets(X, idx, cand, r):
    dp = X[cand][None, :, :] - X[idx][:, None, :]
    d2 = dot(dp, dp)
    near = (idx[:, None] != cand[None, :]) & (d2 <= r * r) & (d2 > 0.0)
    return dp, d2, near


def spfh(X, N, r, block=128):
    """X [n,3], N the ORIENTED normals [n,3] or [n,4] -> (counts int32 [n,33], m int32 [n])"""
    X, N = widen(X), np.asarray(N, np.float64)[:, :3]
    n = X.shape[0]
    valid = valid_normals(N)
    counts = np.zeros((n, WIDTH), np.int32); m = np.zeros(n, np.int32)
    for idx, cand in _blocks(X, r, block):
        dp, d2, near = _offsets(X, idx, cand, r)
        use = near & valid[idx][:, None] & valid[cand][None, :]
        bi, kj = np.nonzero(use)
        if bi.size == 0:
            continue
        ok, b1, b2, b3 = pair_bins(dp[bi, kj], d2[bi, kj], N[idx[bi]], N[cand[kj]])
        rows = idx[bi[ok]]
        np.add.at(m, rows, 1)
        for off, b in ((0, b1), (BINS, b2), (2 * BINS, b3)):
            np.add.at(counts, (rows, off + b[ok]), 1)
    return counts, m


def scaled(counts, m):
    """S = count (100 / m), 0 where m <= 0"""
    m = np.asarray(m, np.int64)
    scale = np.where(m > 0, 100.0 / np.maximum(m, 1).astype(np.float64), 0.0)
    return np.asarray(counts).astype(np.float64) * scale[:, None]


def _finish(W, S, m):
    F = np.zeros_like(W)
    for g in range(3):
        sg = np.zeros(W.shape[0])
        for b in range(g * BINS, (g + 1) * BINS):
            sg = sg + W[:, b]
        with np.errstate(divide='ignore', invalid='ignore'):
            F[:, g * BINS:(g + 1) * BINS] = np.where((sg > 0.0)[:, None], (100.0 * W[:, g * BINS:(g + 1) * BINS]) / sg[:, None], 0.0)
    valid = np.asarray(m) > 0
    F = np.where(valid[:, None], F + S, 0.0)
    return F.astype(np.float32), valid, F


def fpfh(X, counts, m, r, block=128):
    """-> (features float32 [n,33], valid bool [n], the float64 values before the rounding)"""
    X = widen(X)
    S = scaled(counts, m)
    has = np.asarray(m) > 0
    W = np.zeros((X.shape[0], WIDTH))
    for idx, cand in _blocks(X, r, block):
        _, d2, near = _offsets(X, idx, cand, r)
        use = near & has[cand][None, :]
        with np.errstate(divide='ignore', invalid='ignore'):
            for b in range(WIDTH):          # (cumsum adds in ascending candidate = ascending row, like the loop form; the zeros change no bit)
                if cand.size:
                    W[idx, b] = np.cumsum(np.where(use, S[cand, b][None, :] / d2, 0.0), axis=1)[:, -1]
    return _finish(W, S, m)


def describe(X, N, c, r):
    """points, raw normal table, viewpoint, radius -> (oriented table, counts, m, features float32, valid)"""
    No = orient(X, N, c)
    counts, m = spfh(X, No, r)
    F, valid, _ = fpfh(X, counts, m, r)
    return No, counts, m, F, valid


# ---- the plain double loops -----------------------------------------------------------------------------------------------------------------
def spfh_loop(X, N, r):
    X, N = widen(X), np.asarray(N, np.float64)[:, :3]
    n = X.shape[0]
    valid = valid_normals(N)
    counts = np.zeros((n, WIDTH), np.int32); m = np.zeros(n, np.int32)
    for i in range(n):
        for j in range(n):
            if j == i or not (valid[i] and valid[j]):
                continue
            dp = X[j] - X[i]
            d2 = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]
            if not (d2 <= r * r and d2 > 0.0):
                continue
            ok, b1, b2, b3 = pair_bins(dp, d2, N[i], N[j])
            if not ok:
                continue
            m[i] += 1
            counts[i, int(b1)] += 1; counts[i, BINS + int(b2)] += 1; counts[i, 2 * BINS + int(b3)] += 1
    return counts, m


def fpfh_loop(X, counts, m, r):
    X = widen(X)
    n = X.shape[0]
    S = scaled(counts, m)
    W = np.zeros((n, WIDTH))
    for i in range(n):
        for j in range(n):
            if j == i or m[j] <= 0:
                continue
            dp = X[j] - X[i]
            d2 = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]
            if d2 <= r * r and d2 > 0.0:
                W[i] = W[i] + S[j] / d2
    return _finish(W, S, m)


def neighbours_f32(a):
    """float32 array -> (the next float32 below, the next above)"""
    a = np.asarray(a, np.float32)
    return np.nextafter(a, np.float32(-np.inf)), np.nextafter(a, np.float32(np.inf))
