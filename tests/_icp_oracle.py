"""numpy restatement of the dense ICP refinement (include/roreg_hip.h "v6c"; roreg_amd/csrc/icp.hip): what the device must compute.

Coordinates are float32 values widened to float64; one iteration under (R, t):
  p' = ((R_r0 x + R_r1 y) + R_r2 z) + t_r;  q* = argmin d2, d2 = (dx dx + dy dy) + dz dz, an exact tie going to the LOWEST target row;
  inlier iff d2 <= d d;  n, c_q, c_p over the inliers (p untransformed);  H = sum (q - c_q)(p - c_p)^T in a second pass;
  H = U S V^T (numpy.linalg.svd), R+ = U diag(1, 1, det(U V^T)) V^T, t+ = c_q - R+ c_p;
  stop when the rotation step is below tol_deg degrees AND |t+ - t| < tol_t ('converged'), after max_iter searches ('max_iter'), or when
  n < 3 or rank(H) <= 1 ('no_support': (R, t) kept).  A non-finite T0 comes back unchanged ('nonfinite', 0 searches).
The search is brute force in float64.  `nearest` visits, for a block of queries, only the targets inside the block's bounding box grown
by d -- every target it skips is farther than d from every query of the block, so the inlier assignment is the full search's
(nearest_full is the unpruned form; test_icp_oracle.py checks one against the other)."""
from collections import namedtuple

import numpy as np

STATUS = ('converged', 'max_iter', 'no_support', 'nonfinite')
Result = namedtuple('Result', 'T iters inliers rmse status assign stats')


def transform(P, R, t):
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)], 1)


def _block_nearest(Q, rows, Pt):
    """Pt [m,3] against the candidates Q [k,3] with original rows `rows` -> (row of the nearest, lowest row on an exact tie; its d2)."""
    if Q.shape[0] == 0:
        return np.full(Pt.shape[0], -1, np.int64), np.full(Pt.shape[0], np.inf)
    dx = Q[None, :, 0] - Pt[:, None, 0]; dy = Q[None, :, 1] - Pt[:, None, 1]; dz = Q[None, :, 2] - Pt[:, None, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    best = d2.min(1)
    row = np.where(d2 == best[:, None], rows[None, :], np.iinfo(np.int64).max).min(1)
    return row, best


def nearest_full(Q, Pt, d, block=256):
    """Every query against every target.  -> (assign int32 [m]: target row, -1 = nothing within d; d2 of the nearest)."""
    rows = np.arange(Q.shape[0], dtype=np.int64)
    a = np.empty(Pt.shape[0], np.int64); b = np.empty(Pt.shape[0])
    for s in range(0, Pt.shape[0], block):
        a[s:s + block], b[s:s + block] = _block_nearest(Q, rows, Pt[s:s + block])
    ok = (a >= 0) & (b <= d * d)
    return np.where(ok, a, -1).astype(np.int32), b


def nearest(Q, Pt, d, block=256):
    order = np.argsort(Q[:, 0], kind='stable')
    Qs, qx = Q[order], Q[order, 0]
    a = np.full(Pt.shape[0], -1, np.int64); b = np.full(Pt.shape[0], np.inf)
    reach = d * (1.0 + 1e-9)
    live = np.flatnonzero(np.isfinite(Pt).all(1))
    # blocks of queries that are close together: ordered by a coarse cell (any order is correct; a compact block has few candidates)
    cell = np.floor(Pt[live] / max(4.0 * d, 1e-12))
    live = live[np.lexsort((cell[:, 2], cell[:, 1], cell[:, 0]))]
    for s in range(0, live.shape[0], block):
        idx = live[s:s + block]
        lo3, hi3 = Pt[idx].min(0) - reach, Pt[idx].max(0) + reach
        lo = np.searchsorted(qx, lo3[0], 'left'); hi = np.searchsorted(qx, hi3[0], 'right')
        C = Qs[lo:hi]
        keep = np.flatnonzero((C[:, 1] >= lo3[1]) & (C[:, 1] <= hi3[1]) & (C[:, 2] >= lo3[2]) & (C[:, 2] <= hi3[2]))
        a[idx], b[idx] = _block_nearest(C[keep], order[lo:hi][keep].astype(np.int64), Pt[idx])
    ok = (a >= 0) & (b <= d * d)
    return np.where(ok, a, -1).astype(np.int32), b


def iterate(Q, P, R, t, d, nn=nearest):
    """One search + both summation passes under (R, t) -> dict(assign, d2, n, cq, cp, H, sum_d2)."""
    assign, d2 = nn(Q, transform(P, R, t), d)
    sel = assign >= 0
    n = int(sel.sum())
    q, p = Q[assign[sel]], P[sel]
    out = dict(assign=assign, n=n, sum_d2=float(d2[sel].sum()), cq=np.zeros(3), cp=np.zeros(3), H=np.zeros((3, 3)))
    if n:
        out['cq'] = q.sum(0) / n; out['cp'] = p.sum(0) / n
        out['H'] = (q - out['cq']).T @ (p - out['cp'])
    return out


def solve(H, cq, cp):
    """-> (R+, t+), or None when rank(H) <= 1."""
    if not np.isfinite(H).all():
        return None
    U, S, Vt = np.linalg.svd(H)
    if not (S[1] > 1e-10 * S[0]):
        return None
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    return R, cq - transform(cp[None], R, np.zeros(3))[0]


def solve_full(H, cq, cp):
    """solve() and what decided it -> (R+ or None, t+ or None, singular values [3] or None for a non-finite H, sign det(U V^T)).  The
    rotation moves by at most 2 |dH| / gap under a change dH of H, gap = S[1] + sign * S[2] (tests/_icp_cases.py, the solve family)."""
    if not np.isfinite(H).all():
        return None, None, None, 0.0
    U, S, Vt = np.linalg.svd(H)
    sign = 1.0 if np.linalg.det(U @ Vt) > 0 else -1.0
    new = solve(H, cq, cp)
    return (None, None, S, sign) if new is None else (new[0], new[1], S, sign)


def rotation_step_deg(Ra, Rb):
    """The angle between two rotations from |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2) (well conditioned at small angles)."""
    return np.rad2deg(2.0 * np.arcsin(min(1.0, np.sqrt(((Ra - Rb) ** 2).sum()) / (2.0 * np.sqrt(2.0)))))


def icp(Q, P, T0, d, max_iter=30, tol_deg=1e-4, tol_t=1e-6, nn=nearest):
    Q = np.asarray(Q, np.float32).astype(np.float64).reshape(-1, 3); P = np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.array(T0, np.float64)
    if not np.isfinite(T[:3]).all():
        return Result(T, 0, 0, float('nan'), 'nonfinite', None, None)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    iters, status, it = 0, 'max_iter', None
    for k in range(max_iter):
        it = iterate(Q, P, R, t, d, nn)
        iters = k + 1
        new = solve(it['H'], it['cq'], it['cp']) if it['n'] >= 3 else None
        if new is None:
            status = 'no_support'
            break
        step = rotation_step_deg(new[0], R); dt = np.sqrt(((new[1] - t) ** 2).sum())
        R, t = new
        if step < tol_deg and dt < tol_t:
            status = 'converged'
            break
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    if it is None:
        return Result(T, 0, 0, float('nan'), status, None, None)
    rmse = np.sqrt(it['sum_d2'] / it['n']) if it['n'] else float('nan')
    return Result(T, iters, it['n'], float(rmse), status, it['assign'], it)


def pose_error(T, T_gt):
    """-> (rotation error in degrees, translation error in metres)."""
    return rotation_step_deg(T[:3, :3], T_gt[:3, :3]), float(np.sqrt(((T[:3, 3] - T_gt[:3, 3]) ** 2).sum()))


def perturb(T_gt, deg, shift, seed):
    """T_gt composed with a rotation by `deg` degrees about a seeded random axis and a seeded translation of length `shift`."""
    rng = np.random.default_rng([int(seed), 0x9e1])
    k = rng.standard_normal(3); k /= np.sqrt((k * k).sum())
    u = rng.standard_normal(3); u *= shift / np.sqrt((u * u).sum())
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    th = np.deg2rad(deg)
    dR = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T = np.array(T_gt, np.float64)
    T[:3, :3] = dR @ T_gt[:3, :3]
    T[:3, 3] = T_gt[:3, 3] + u
    return T


# the input of the convergence tests, CPU and GPU: make_dense_pair(CONV_SEED, CONV_N); the starts are perturb(T_gt, deg, shift, CONV_SEED)
CONV_SEED, CONV_N = 11, 20000
CONV_STARTS = ((3.0, 0.05), (5.0, 0.10))
