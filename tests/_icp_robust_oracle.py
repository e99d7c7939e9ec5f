"""numpy restatement of the robust losses inside the point-to-plane and plane-to-plane ICP iterations (include/roreg_hip.h "v6p";
roreg_amd/csrc/icp.hip, roreg_amd/csrc/icp_math.h robust_weight): what the device must compute.  There is no other reference: this file is
the definition.  tests/_icp_plane_oracle.py (PO) and tests/_icp_gicp_oracle.py (GO) supply everything a loss leaves alone -- the search, the
centre c, which correspondences count, the solve, the update and the convergence test.

loss in LOSSES and scale k > 0, finite; with u = r / k the weight of a correspondence is
    huber 1 if |u| <= 1 else 1 / |u|;  cauchy 1 / (1 + u^2);  gm 1 / (1 + u^2)^2;  tukey (1 - u^2)^2 if |u| <= 1 else 0.
plane: r = e, the signed plane residual; A = sum w J J^T, b = -sum w J e.
gicp:  r = sqrt(2 epsilon max(d^T M d, 0)); A = sum w J^T M J, b = -sum w J^T M d.
The count (n_valid / n) and sum e^2 / sum d^T M d stay unweighted.  `weight` performs the operations of the C++ in its order (one division
for u, one by a denominator chosen first), so the two agree value by value.  numpy only."""
import numpy as np

import _icp_gicp_oracle as GO
import _icp_oracle as O
import _icp_plane_oracle as PO

LOSSES = ('huber', 'cauchy', 'gm', 'tukey')
Result = O.Result


def weight(loss, r, k):
    """loss None: ones."""
    r = np.asarray(r, np.float64)
    if loss is None:
        return np.ones_like(r)
    assert loss in LOSSES and np.all(np.asarray(k) > 0) and np.all(np.isfinite(k)), (loss, k)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        u = r / np.float64(k)
        a, u2 = np.abs(u), u * u
        inside = a <= 1.0
        if loss == 'huber':
            den = np.where(inside, 1.0, a)
        elif loss in ('cauchy', 'gm'):
            den = 1.0 + u2
        else:
            den = np.ones_like(u)
        inv = 1.0 / den
        t = 1.0 - u2
        if loss == 'tukey':
            return np.where(inside, t * t, 0.0)
        return inv * inv if loss == 'gm' else inv


def gicp_residual(q, epsilon):
    with np.errstate(over='ignore'):
        return np.sqrt((2.0 * epsilon) * np.maximum(q, 0.0))


def iterate_plane(Q, P, N, R, t, d, loss=None, scale=None, nn=O.nearest):
    """PO.iterate with every correspondence weighted -> dict(assign, n, n_valid, c, A, b, sum_e2, e, w): e and w per counted correspondence."""
    assign, _ = nn(Q, O.transform(P, R, t), d)
    sel = assign >= 0
    n = int(sel.sum())
    out = dict(assign=assign, n=n, n_valid=0, c=np.zeros(3), A=np.zeros((6, 6)), b=np.zeros(6), sum_e2=0.0, e=np.zeros(0), w=np.zeros(0))
    if n == 0:
        return out
    cp = P[sel].sum(0) / n
    c = O.transform(cp[None], R, t)[0]
    nrm_all = np.asarray(N)[np.maximum(assign, 0), :3]
    use = sel & (nrm_all != 0).any(1)
    pt = O.transform(P[use], R, t)
    q, nrm = Q[assign[use]], nrm_all[use]
    a = pt - c
    dq = pt - q
    e = (nrm[:, 0] * dq[:, 0] + nrm[:, 1] * dq[:, 1]) + nrm[:, 2] * dq[:, 2]
    w = weight(loss, e, scale)
    J = np.concatenate([np.cross(a, nrm), nrm], 1)
    WJ = J * w[:, None]
    out.update(n_valid=int(use.sum()), c=c, A=WJ.T @ J, b=-(WJ * e[:, None]).sum(0), sum_e2=float((e * e).sum()), e=e, w=w)
    return out


def iterate_gicp(Q, P, Nq, Np, R, t, d, epsilon=GO.EPSILON, loss=None, scale=None, nn=O.nearest):
    """GO.iterate with every correspondence weighted -> dict(assign, n, c, A, b, sum_md, e, w): e = sqrt(2 epsilon d^T M d) per inlier."""
    assign, _ = nn(Q, O.transform(P, R, t), d)
    sel = assign >= 0
    n = int(sel.sum())
    out = dict(assign=assign, n=n, c=np.zeros(3), A=np.zeros((6, 6)), b=np.zeros(6), sum_md=0.0, e=np.zeros(0), w=np.zeros(0))
    if n == 0:
        return out
    cp = P[sel].sum(0) / n
    c = O.transform(cp[None], R, t)[0]
    pt = O.transform(P[sel], R, t)
    q = Q[assign[sel]]
    nq = np.asarray(Nq)[assign[sel], :3]
    m = O.transform(np.asarray(Np)[sel, :3], R, np.zeros(3))
    M = GO.weights(nq, m, epsilon)
    a = pt - c
    dq = pt - q
    J = np.concatenate([-GO.cross_matrix(a), np.broadcast_to(np.eye(3), (n, 3, 3))], 2)             # [n,3,6]
    md = np.einsum('kij,kj->ki', M, dq)
    qf = (dq * md).sum(1)
    e = gicp_residual(qf, epsilon)
    w = weight(loss, e, scale)
    MJ = (M * w[:, None, None]) @ J
    out.update(c=c, A=np.einsum('kji,kjl->il', J, MJ), b=-np.einsum('kji,kj->i', J, md * w[:, None]), sum_md=float(qf.sum()), e=e, w=w)
    return out


def _run(step, count, total, T0, max_iter, tol_deg, tol_t, trace):
    """PO.icp's / GO.icp's loop over `step(R, t)` -> dict with the count under `count` and the squared-residual sum under `total`."""
    T = np.array(T0, np.float64)
    if not np.isfinite(T[:3]).all():
        return Result(T, 0, 0, float('nan'), 'nonfinite', None, None)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    iters, status, it = 0, 'max_iter', None
    for k in range(max_iter):
        it = step(R, t)
        iters = k + 1
        x, lam = PO.solve(it['A'], it['b'], it[count])
        if x is None:
            status = 'no_support'
            if trace is not None:
                trace.append(dict(n_valid=it[count], lam=lam, step_deg=None, step_t=None))
            break
        Rn, tn = PO.update(R, t, it['c'], x)
        step_deg = O.rotation_step_deg(Rn, R); dt = np.sqrt(((tn - t) ** 2).sum())
        if trace is not None:
            trace.append(dict(n_valid=it[count], lam=lam, step_deg=step_deg, step_t=dt))
        R, t = Rn, tn
        if step_deg < tol_deg and dt < tol_t:
            status = 'converged'
            break
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = t
    if it is None:
        return Result(T, 0, 0, float('nan'), status, None, None)
    rmse = np.sqrt(it[total] / it[count]) if it[count] else float('nan')
    return Result(T, iters, it[count], float(rmse), status, it['assign'], it)


def icp_plane(Q, P, N, T0, d, loss=None, scale=None, max_iter=30, tol_deg=1e-4, tol_t=1e-6, nn=O.nearest, trace=None):
    """PO.icp under a loss (loss None: PO.icp's own result); trace as PO.icp's."""
    Q, P = PO.widen(Q), PO.widen(P)
    return _run(lambda R, t: iterate_plane(Q, P, N, R, t, d, loss, scale, nn), 'n_valid', 'sum_e2', T0, max_iter, tol_deg, tol_t, trace)


def icp_gicp(Q, P, Nq, Np, T0, d, epsilon=GO.EPSILON, loss=None, scale=None, max_iter=30, tol_deg=1e-4, tol_t=1e-6, nn=O.nearest, trace=None):
    """GO.icp under a loss."""
    Q, P = PO.widen(Q), PO.widen(P)
    return _run(lambda R, t: iterate_gicp(Q, P, Nq, Np, R, t, d, epsilon, loss, scale, nn), 'n', 'sum_md', T0, max_iter, tol_deg, tol_t, trace)
