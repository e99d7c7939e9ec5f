"""numpy restatement of the plane-to-plane (generalized) ICP iteration (include/roreg_hip.h "v6i"; roreg_amd/csrc/icp.hip icp_gicp_kernel): what
the device must compute.  There is no other reference for this method: this file is its definition.  tests/_icp_oracle.py (O) supplies the
search, the transform and the convergence test, tests/_icp_plane_oracle.py (PO) the 6x6 solve, the update and the widening.

One iteration under (R, t), Nq / Np the target's and the source's normal tables in original row order (rows (nx, ny, nz[, m]); a zero row
means "no valid normal"): O.nearest gives the assignment; c = R c_p + t, c_p the centroid of the untransformed source points of the distance
inliers; for EVERY distance inlier (p, q): p' = transform(p), d = p' - q, a = p' - c, m = R n_p, kappa = 1 - epsilon,
S = 2 I - kappa (n_q n_q^T + m m^T) -- the sum C_q + R C_p R^T of the surface-aligned covariances C = V diag(1, 1, epsilon) V^T =
I - kappa n n^T --, M = S^-1 by the adjugate over the determinant, J = [-[a]x, I]; A = sum J^T M J, b = -sum J^T M d, and sum d^T M d.  A zero
normal contributes no n n^T term; nothing is skipped.  PO.solve / PO.update as they are ('no_support' when n < 6 or lambda_min <=
1e-10 lambda_max); inliers = n, rmse = sqrt(sum d^T M d / n) of the last executed search.  numpy only."""
import numpy as np

import _icp_oracle as O
import _icp_plane_oracle as PO

Result = O.Result
EPSILON = 1e-3


def inverse_sym3(S):
    """S [k,3,3] symmetric -> S^-1 by the adjugate over the determinant (the device's closed form), checked against numpy.linalg.inv within
    50 cond(S) 2^-53 of |S^-1|."""
    s00, s01, s02, s11, s12, s22 = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    c00 = s11 * s22 - s12 * s12; c01 = s02 * s12 - s01 * s22; c02 = s01 * s12 - s02 * s11
    c11 = s00 * s22 - s02 * s02; c12 = s01 * s02 - s00 * s12; c22 = s00 * s11 - s01 * s01
    inv = 1.0 / ((s00 * c00 + s01 * c01) + s02 * c02)
    M = np.stack([np.stack([c00, c01, c02], 1), np.stack([c01, c11, c12], 1), np.stack([c02, c12, c22], 1)], 1) * inv[:, None, None]
    if S.shape[0]:
        ref = np.linalg.inv(S)
        scale = np.abs(ref).max((1, 2))
        assert (np.abs(M - ref).max((1, 2)) <= 50 * np.linalg.cond(S) * 2.0 ** -53 * scale).all(), 'closed-form inverse differs from numpy.linalg.inv'
    return M


def cross_matrix(a):
    """a [k,3] -> [a]x [k,3,3]"""
    z = np.zeros(a.shape[0])
    return np.stack([np.stack([z, -a[:, 2], a[:, 1]], 1), np.stack([a[:, 2], z, -a[:, 0]], 1), np.stack([-a[:, 1], a[:, 0], z], 1)], 1)


def weights(nq, m, epsilon):
    """Unit (or zero) normals nq, m [k,3] -> M [k,3,3] = (2 I - kappa (nq nq^T + m m^T))^-1"""
    kappa = 1.0 - epsilon
    S = 2.0 * np.eye(3)[None] - kappa * (nq[:, :, None] * nq[:, None, :] + m[:, :, None] * m[:, None, :])
    return inverse_sym3(S)


def iterate(Q, P, Nq, Np, R, t, d, epsilon=EPSILON, nn=O.nearest):
    """One search + the gicp pass under (R, t) -> dict(assign, n, c, A, b, sum_md)."""
    assign, _ = nn(Q, O.transform(P, R, t), d)
    sel = assign >= 0
    n = int(sel.sum())
    out = dict(assign=assign, n=n, c=np.zeros(3), A=np.zeros((6, 6)), b=np.zeros(6), sum_md=0.0)
    if n == 0:
        return out
    cp = P[sel].sum(0) / n
    c = O.transform(cp[None], R, t)[0]
    pt = O.transform(P[sel], R, t)
    q = Q[assign[sel]]
    nq = np.asarray(Nq)[assign[sel], :3]
    m = O.transform(np.asarray(Np)[sel, :3], R, np.zeros(3))
    M = weights(nq, m, epsilon)
    a = pt - c
    dq = pt - q
    J = np.concatenate([-cross_matrix(a), np.broadcast_to(np.eye(3), (n, 3, 3))], 2)             # [n,3,6]
    MJ = M @ J
    w = np.einsum('kij,kj->ki', M, dq)
    out.update(c=c, A=np.einsum('kji,kjl->il', J, MJ), b=-np.einsum('kji,kj->i', J, w), sum_md=float((dq * w).sum()))
    return out


def icp(Q, P, Nq, Np, T0, d, epsilon=EPSILON, max_iter=30, tol_deg=1e-4, tol_t=1e-6, nn=O.nearest, trace=None):
    """trace: an optional list that receives, per executed iteration, dict(n_valid, lam, step_deg, step_t) (n_valid = n: the keys of
    PO.icp's trace)."""
    Q, P = PO.widen(Q), PO.widen(P)
    T = np.array(T0, np.float64)
    if not np.isfinite(T[:3]).all():
        return Result(T, 0, 0, float('nan'), 'nonfinite', None, None)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    iters, status, it = 0, 'max_iter', None
    for k in range(max_iter):
        it = iterate(Q, P, Nq, Np, R, t, d, epsilon, nn)
        iters = k + 1
        x, lam = PO.solve(it['A'], it['b'], it['n'])
        if x is None:
            status = 'no_support'
            if trace is not None:
                trace.append(dict(n_valid=it['n'], lam=lam, step_deg=None, step_t=None))
            break
        Rn, tn = PO.update(R, t, it['c'], x)
        step = O.rotation_step_deg(Rn, R); dt = np.sqrt(((tn - t) ** 2).sum())
        if trace is not None:
            trace.append(dict(n_valid=it['n'], lam=lam, step_deg=step, step_t=dt))
        R, t = Rn, tn
        if step < tol_deg and dt < tol_t:
            status = 'converged'
            break
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    if it is None:
        return Result(T, 0, 0, float('nan'), status, None, None)
    rmse = np.sqrt(it['sum_md'] / it['n']) if it['n'] else float('nan')
    return Result(T, iters, it['n'], float(rmse), status, it['assign'], it)
