"""numpy restatement of the surface normals and the point-to-plane ICP iteration (include/roreg_hip.h "v6d"; roreg_amd/csrc/icp.hip): what
the device must compute.  tests/_icp_oracle.py (O) supplies the search, the transform and the convergence test.

Normals of a cloud for (radius r, min_neighbors k), coordinates float32 widened to float64: the neighbourhood of point i is every point j
of the cloud, itself included, with d2 = (dx dx + dy dy) + dz dz <= r r; on the offsets y_j = x_j - x_i: m, ybar = sum y / m, then
C = sum (y - ybar)(y - ybar)^T; numpy.linalg.eigh; the normal is the eigenvector of the smallest eigenvalue (sign free); valid iff m >= k and
lambda_mid > 1e-8 lambda_max; an invalid row is the zero vector.  Table [n,4] = (nx, ny, nz, m) in original row order.
`normals` visits, for a block of points, only the points inside the block's bounding box grown by r (every point it skips is farther than r
from every point of the block); normals_full is the unpruned form, test_icp_plane_oracle.py checks one against the other.

One point-to-plane iteration under (R, t): O.nearest gives the assignment; c = R c_p + t, c_p the centroid of the untransformed source points
of ALL distance inliers; a correspondence counts iff it is a distance inlier and its target normal is valid; p' = transform(p), a = p' - c,
e = (nx dx + ny dy) + nz dz with d = p' - q, J = [a x n, n]; A = sum J J^T, b = -sum J e; eigh(A); 'no_support' (T kept) when n_valid < 6 or
lambda_min <= 1e-10 lambda_max; else x = V diag(1 / lambda) V^T b = (w, v), dR = exp([w]x), R+ = dR R, t+ = dR (t - c) + c + v.  The
convergence test, max_iter and 'nonfinite' are O.icp's; inliers = n_valid, rmse = sqrt(sum e^2 / n_valid) of the last executed search.
numpy only."""
from collections import namedtuple

import numpy as np

import _icp_oracle as O

Normals = namedtuple('Normals', 'table normals valid counts lam')
Normals.__doc__ = 'table [n,4] = (n, m); normals [n,3] (zero where invalid); valid bool [n]; counts int64 [n]; lam [n,3] ascending eigenvalues of C'
Result = O.Result
VALID_RATIO, SUPPORT_RATIO, MIN_VALID = 1e-8, 1e-10, 6


def widen(P):
    return np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3)


def _block_normals(X, cand, r):
    """X [b,3] against the candidates cand [k,3] (which hold every point within r of every row of X) -> (m [b], C [b,3,3])."""
    Y = cand[None, :, :] - X[:, None, :]
    d2 = (Y[..., 0] * Y[..., 0] + Y[..., 1] * Y[..., 1]) + Y[..., 2] * Y[..., 2]
    w = (d2 <= r * r)
    m = w.sum(1)
    ybar = (Y * w[..., None]).sum(1) / np.maximum(m, 1)[:, None]
    Z = (Y - ybar[:, None, :]) * w[..., None]
    return m, np.einsum('bki,bkj->bij', Z, Z)


def _finish(m, C, k):
    lam, V = np.linalg.eigh(C)
    valid = (m >= k) & (lam[:, 1] > VALID_RATIO * lam[:, 2])
    nrm = np.where(valid[:, None], V[:, :, 0], 0.0)
    return Normals(np.concatenate([nrm, m[:, None].astype(np.float64)], 1), nrm, valid, m.astype(np.int64), lam)


def normals_full(X, r, k=MIN_VALID, block=64):
    X = widen(X)
    m = np.zeros(X.shape[0], np.int64); C = np.zeros((X.shape[0], 3, 3))
    for s in range(0, X.shape[0], block):
        m[s:s + block], C[s:s + block] = _block_normals(X[s:s + block], X, r)
    return _finish(m, C, k)


def normals(X, r, k=MIN_VALID, block=256):
    X = widen(X)
    n = X.shape[0]
    m = np.zeros(n, np.int64); C = np.zeros((n, 3, 3))
    order = np.argsort(X[:, 0], kind='stable')
    Xs, xs = X[order], X[order, 0]
    reach = r * (1.0 + 1e-9)
    cell = np.floor(X / max(2.0 * r, 1e-12))
    rows = np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))
    for s in range(0, n, block):
        idx = rows[s:s + block]
        lo3, hi3 = X[idx].min(0) - reach, X[idx].max(0) + reach
        lo = np.searchsorted(xs, lo3[0], 'left'); hi = np.searchsorted(xs, hi3[0], 'right')
        cand = Xs[lo:hi]
        keep = (cand[:, 1] >= lo3[1]) & (cand[:, 1] <= hi3[1]) & (cand[:, 2] >= lo3[2]) & (cand[:, 2] <= hi3[2])
        m[idx], C[idx] = _block_normals(X[idx], cand[keep], r)
    return _finish(m, C, k)


def angle_to(a, b):
    """The angle between unit vectors a and b [n,3] up to sign, from the cross product (well conditioned at small angles)."""
    return np.arcsin(np.minimum(1.0, np.sqrt((np.cross(a, b) ** 2).sum(1))))


def gap_ratio(lam):
    """(lambda_mid - lambda_min) / lambda_max: what the normal's direction is conditioned by."""
    return (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0)


# ---- the iteration ---------------------------------------------------------------------------------------------------------------------------
def rodrigues(w):
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * K + b * (K @ K)


def iterate(Q, P, N, R, t, d, nn=O.nearest):
    """One search + the plane pass under (R, t); N is the target's normal table [n,4] (or [n,3]) -> dict(assign, n, n_valid, c, A, b, sum_e2)."""
    assign, _ = nn(Q, O.transform(P, R, t), d)
    sel = assign >= 0
    n = int(sel.sum())
    out = dict(assign=assign, n=n, n_valid=0, c=np.zeros(3), A=np.zeros((6, 6)), b=np.zeros(6), sum_e2=0.0)
    if n == 0:
        return out
    cp = P[sel].sum(0) / n
    c = O.transform(cp[None], R, t)[0]
    nrm_all = N[np.maximum(assign, 0), :3]
    use = sel & (nrm_all != 0).any(1)
    pt = O.transform(P[use], R, t)
    q, nrm = Q[assign[use]], nrm_all[use]
    a = pt - c
    dq = pt - q
    e = (nrm[:, 0] * dq[:, 0] + nrm[:, 1] * dq[:, 1]) + nrm[:, 2] * dq[:, 2]
    J = np.concatenate([np.cross(a, nrm), nrm], 1)
    out.update(n_valid=int(use.sum()), c=c, A=J.T @ J, b=-(J * e[:, None]).sum(0), sum_e2=float((e * e).sum()))
    return out


def solve(A, b, n_valid):
    """-> (x [6], eigenvalues ascending) or (None, eigenvalues or None): None when n_valid < 6 or lambda_min <= 1e-10 lambda_max."""
    if n_valid < MIN_VALID or not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None, None
    lam, V = np.linalg.eigh(A)
    if not (lam[-1] > 0.0 and lam[0] > SUPPORT_RATIO * lam[-1]):
        return None, lam
    return V @ ((V.T @ b) / lam), lam


def update(R, t, c, x):
    dR = rodrigues(x[:3])
    return dR @ R, dR @ (t - c) + c + x[3:]


def icp(Q, P, N, T0, d, max_iter=30, tol_deg=1e-4, tol_t=1e-6, nn=O.nearest, trace=None):
    """trace: an optional list that receives, per executed iteration, dict(n_valid, lam, step_deg, step_t)."""
    Q, P = widen(Q), widen(P)
    T = np.array(T0, np.float64)
    if not np.isfinite(T[:3]).all():
        return Result(T, 0, 0, float('nan'), 'nonfinite', None, None)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    iters, status, it = 0, 'max_iter', None
    for k in range(max_iter):
        it = iterate(Q, P, N, R, t, d, nn)
        iters = k + 1
        x, lam = solve(it['A'], it['b'], it['n_valid'])
        if x is None:
            status = 'no_support'
            if trace is not None:
                trace.append(dict(n_valid=it['n_valid'], lam=lam, step_deg=None, step_t=None))
            break
        Rn, tn = update(R, t, it['c'], x)
        step = O.rotation_step_deg(Rn, R); dt = np.sqrt(((tn - t) ** 2).sum())
        if trace is not None:
            trace.append(dict(n_valid=it['n_valid'], lam=lam, step_deg=step, step_t=dt))
        R, t = Rn, tn
        if step < tol_deg and dt < tol_t:
            status = 'converged'
            break
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    if it is None:
        return Result(T, 0, 0, float('nan'), status, None, None)
    rmse = np.sqrt(it['sum_e2'] / it['n_valid']) if it['n_valid'] else float('nan')
    return Result(T, iters, it['n_valid'], float(rmse), status, it['assign'], it)


def upper(A):
    """The 21 upper entries of a 6x6 matrix row by row (the layout of the device's slots and of its stats row)."""
    return A[np.triu_indices(6)]
