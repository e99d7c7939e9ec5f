"""numpy restatement of the pose-graph optimiser's definitions (include/roreg_hip.h "v6h"), written from the definitions and not from the
kernels: dense 6x6 Jacobians, a dense normal matrix, numpy's Cholesky.  Host only."""
from collections import deque

import numpy as np

DEC_ACCEPT, DEC_REJECT, DEC_PIVOT, DEC_STOP = 1, 2, 3, 4
STATUS = ('converged', 'max_iter', 'stalled', 'nonfinite')


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = skew(w)
    if th < 1e-8:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def rigid_inv(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def quat_shepperd(R):
    """(w, x, y, z), unit, w >= 0: the largest of the four components from its square root, the others from the off-diagonal sums."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cand = np.array([tr, R[0, 0], R[1, 1], R[2, 2]])
    k = int(np.argmax(cand))                                  # ties go to the first: w, then x, y, z
    if k == 0:
        w = 0.5 * np.sqrt(1.0 + tr); s = 0.25 / w
        q = np.array([w, (R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s])
    elif k == 1:
        x = 0.5 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]); s = 0.25 / x
        q = np.array([(R[2, 1] - R[1, 2]) * s, x, (R[0, 1] + R[1, 0]) * s, (R[0, 2] + R[2, 0]) * s])
    elif k == 2:
        y = 0.5 * np.sqrt(1.0 - R[0, 0] + R[1, 1] - R[2, 2]); s = 0.25 / y
        q = np.array([(R[0, 2] - R[2, 0]) * s, (R[0, 1] + R[1, 0]) * s, y, (R[1, 2] + R[2, 1]) * s])
    else:
        z = 0.5 * np.sqrt(1.0 - R[0, 0] - R[1, 1] + R[2, 2]); s = 0.25 / z
        q = np.array([(R[1, 0] - R[0, 1]) * s, (R[0, 2] + R[2, 0]) * s, (R[1, 2] + R[2, 1]) * s, z])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def residual(Pi, Pj, T):
    """-> (e [6], q [4], E [4,4], M [4,4]) with M = inv(P_i) P_j, E = inv(T) M."""
    M = rigid_inv(Pi) @ Pj
    E = rigid_inv(T) @ M
    q = quat_shepperd(E[:3, :3])
    return np.concatenate([E[:3, 3], q[1:]]), q, E, M


def pose_update(P, delta):
    D = np.eye(4)
    D[:3, :3] = exp_so3(delta[3:]); D[:3, 3] = delta[:3]
    return P @ D


def adjoint(X):
    """Ad(X) for twists ordered (v, omega): X [Exp(omega), v] X^-1 ~ Exp(Ad(X) (v, omega)) to first order."""
    R, t = X[:3, :3], X[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R; A[:3, 3:] = skew(t) @ R; A[3:, 3:] = R
    return A


def jacobians(Pi, Pj, T):
    """-> (e, J_i, J_j): the first derivatives of e under P <- P [Exp(omega), v; 0, 1], delta = (v, omega)."""
    e, q, E, M = residual(Pi, Pj, T)
    Jj = np.zeros((6, 6))
    Jj[:3, :3] = E[:3, :3]
    Jj[3:, 3:] = 0.5 * (q[0] * np.eye(3) + skew(q[1:]))
    Ji = -Jj @ adjoint(rigid_inv(M))
    return e, Ji, Jj


def numeric_jacobians(Pi, Pj, T, h=1e-6):
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Ji[:, k] = (residual(pose_update(Pi, d), Pj, T)[0] - residual(pose_update(Pi, -d), Pj, T)[0]) / (2 * h)
        Jj[:, k] = (residual(Pi, pose_update(Pj, d), T)[0] - residual(Pi, pose_update(Pj, -d), T)[0]) / (2 * h)
    return Ji, Jj


def rho_w(chi2, lam00, tau):
    if lam00 == 0:
        return 0.0, 0.0
    if tau is None:
        return chi2, 1.0
    mu = tau * tau * lam00
    return mu * chi2 / (mu + chi2), (mu / (mu + chi2)) ** 2


def topology(n_nodes, edges, anchor):
    """-> (reached bool [C], walk [(node, edge)]): breadth-first from the anchor, a node's edges in ascending edge index."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    reached = np.zeros(n_nodes, bool); reached[anchor] = True
    walk, queue = [], deque([anchor])
    while queue:
        u = queue.popleft()
        for k in range(edges.shape[0]):
            if u in (edges[k, 0], edges[k, 1]):
                v = edges[k, 1] if edges[k, 0] == u else edges[k, 0]
                if not reached[v]:
                    reached[v] = True; walk.append((int(v), k)); queue.append(int(v))
    return reached, walk


def initial_poses(n_nodes, edges, transforms, anchor):
    reached, walk = topology(n_nodes, edges, anchor)
    P = np.tile(np.eye(4), (n_nodes, 1, 1))
    for v, k in walk:
        i, j = edges[k]
        P[v] = P[i] @ transforms[k] if v == j else P[j] @ rigid_inv(transforms[k])
    return P


class Graph:
    def __init__(self, n_nodes, edges, transforms, infos, anchor=0, tau=None):
        self.C = int(n_nodes)
        self.edges = np.asarray(edges, np.int64).reshape(-1, 2)
        self.T = np.asarray(transforms, np.float64).reshape(-1, 4, 4)
        self.Lam = np.asarray(infos, np.float64).reshape(-1, 6, 6)
        self.anchor, self.tau = int(anchor), tau
        self.reached, self.walk = topology(self.C, self.edges, self.anchor)
        self.var = np.full(self.C, -1, np.int64)
        act = np.flatnonzero(self.reached & (np.arange(self.C) != self.anchor))
        self.var[act] = np.arange(act.shape[0])
        self.n = 6 * act.shape[0]
        self.edge_on = self.reached[self.edges[:, 0]] & self.reached[self.edges[:, 1]] if self.edges.shape[0] else np.zeros(0, bool)

    def edge_terms(self, P):
        """-> (e [E,6], chi2 [E], rho [E], w [E], qw [E]) at the poses P."""
        E = self.edges.shape[0]
        e, chi2, rho, w, qw = np.zeros((E, 6)), np.zeros(E), np.zeros(E), np.zeros(E), np.ones(E)
        for k, (i, j) in enumerate(self.edges):
            e[k], q, _, _ = residual(P[i], P[j], self.T[k])
            qw[k] = q[0]
            chi2[k] = e[k] @ self.Lam[k] @ e[k]
            if self.edge_on[k]:
                rho[k], w[k] = rho_w(chi2[k], self.Lam[k, 0, 0], self.tau)
        return e, chi2, rho, w, qw

    def cost(self, P):
        return float(self.edge_terms(P)[2].sum())

    def linearise(self, P):
        """-> (e, chi2, w, J_i [E,6,6], J_j [E,6,6])."""
        e, chi2, _, w, _ = self.edge_terms(P)
        Ji, Jj = np.zeros((len(e), 6, 6)), np.zeros((len(e), 6, 6))
        for k, (i, j) in enumerate(self.edges):
            _, Ji[k], Jj[k] = jacobians(P[i], P[j], self.T[k])
        return e, chi2, w, Ji, Jj

    def assemble(self, P):
        """-> (H [n,n], g [n], Habs, gabs): the sums and the sums of absolute values sum w |J|^T |Lambda| |J| (resp. |e|) that bound any summation order."""
        e, _, w, Ji, Jj = self.linearise(P)
        n = self.n
        H, g, Ha, ga = np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), np.zeros(n)
        for k, (i, j) in enumerate(self.edges):
            if w[k] == 0:
                continue
            L = self.Lam[k]
            for a, Ja in ((i, Ji[k]), (j, Jj[k])):
                va = self.var[a]
                if va < 0:
                    continue
                sa = slice(6 * va, 6 * va + 6)
                g[sa] += w[k] * (Ja.T @ L @ e[k]); ga[sa] += w[k] * (np.abs(Ja).T @ np.abs(L) @ np.abs(e[k]))
                for b, Jb in ((i, Ji[k]), (j, Jj[k])):
                    vb = self.var[b]
                    if vb < 0:
                        continue
                    sb = slice(6 * vb, 6 * vb + 6)
                    H[sa, sb] += w[k] * (Ja.T @ L @ Jb); Ha[sa, sb] += w[k] * (np.abs(Ja).T @ np.abs(L) @ np.abs(Jb))
        return H, g, Ha, ga

    def g_sensitivity(self, P):
        """sum w |J|^T |Lambda| 1 [n]: what an error of size 1 in every component of every e moves g by, at most."""
        _, _, w, Ji, Jj = self.linearise(P)
        s = np.zeros(self.n)
        for k, (i, j) in enumerate(self.edges):
            for a, Ja in ((i, Ji[k]), (j, Jj[k])):
                if w[k] != 0 and self.var[a] >= 0:
                    s[6 * self.var[a]:6 * self.var[a] + 6] += w[k] * (np.abs(Ja).T @ np.abs(self.Lam[k]) @ np.ones(6))
        return s

    def H_sensitivity(self, P):
        """sum w (|J_a|^T |Lambda| 1 1^T + 1 1^T |Lambda| |J_b|) [n,n]: what an error of size 1 in every entry of every J moves H by, to first order."""
        _, _, w, Ji, Jj = self.linearise(P)
        S = np.zeros((self.n, self.n))
        one = np.ones((6, 6))
        for k, (i, j) in enumerate(self.edges):
            for a, Ja in ((i, Ji[k]), (j, Jj[k])):
                for b, Jb in ((i, Ji[k]), (j, Jj[k])):
                    if w[k] != 0 and self.var[a] >= 0 and self.var[b] >= 0:
                        L = np.abs(self.Lam[k])
                        S[6 * self.var[a]:6 * self.var[a] + 6, 6 * self.var[b]:6 * self.var[b] + 6] += w[k] * (np.abs(Ja).T @ L @ one + one @ L @ np.abs(Jb))
        return S

    def damped(self, H, lam):
        return H + lam * np.diag(np.diag(H))

    def apply(self, P, delta):
        Pn = P.copy()
        for c in range(self.C):
            if self.var[c] >= 0:
                Pn[c] = pose_update(P[c], delta[6 * self.var[c]:6 * self.var[c] + 6])
        return Pn

    def optimize(self, init=None, max_iter=100, lambda0=1e-3, tol_t=1e-9, tol_rot=1e-9, tol_cost=1e-10):
        """-> dict(poses, cost0, cost, iters, status, history [iters,4], weights, chi2, rel [per solved round |c - c'| / c], min_pivot,
        min_qw [the smallest |w| of a residual quaternion met in any linearisation or candidate])."""
        P = initial_poses(self.C, self.edges, self.T, self.anchor) if init is None else np.array(init, np.float64).reshape(-1, 4, 4)
        out = dict(rel=[], min_pivot=np.inf, min_qw=np.inf)
        finite = np.isfinite(P).all() and np.isfinite(self.T).all() and np.isfinite(self.Lam).all()
        c = self.cost(P) if finite else np.nan
        lam, hist, status = lambda0, [], 'max_iter'
        if not np.isfinite(c):
            status = 'nonfinite'
        else:
            on = self.edge_on
            for _ in range(max_iter):
                out['min_qw'] = min(out['min_qw'], np.abs(self.edge_terms(P)[4][on]).min() if on.any() else np.inf)
                H, g, _, _ = self.assemble(P)
                A = self.damped(H, lam)
                d = np.diag(A)
                L = None
                if self.n == 0:
                    L = np.zeros((0, 0))
                elif np.isfinite(A).all() and (d > 0).all():
                    try:
                        L = np.linalg.cholesky(A)
                    except np.linalg.LinAlgError:
                        L = None
                if L is None:
                    hist.append((c, np.nan, lam, DEC_PIVOT))
                    lam *= 10.0
                    if lam > 1e12:
                        status = 'stalled'; break
                    continue
                if self.n:
                    out['min_pivot'] = min(out['min_pivot'], float(np.diag(L).min()))
                delta = np.linalg.solve(A, -g) if self.n else np.zeros(0)
                Pn = self.apply(P, delta)
                terms = self.edge_terms(Pn)
                out['min_qw'] = min(out['min_qw'], np.abs(terms[4][on]).min() if on.any() else np.inf)
                c1 = float(terms[2].sum())
                dd = delta.reshape(-1, 6)
                small = bool((np.linalg.norm(dd[:, :3], axis=1) <= tol_t).all() and (np.linalg.norm(dd[:, 3:], axis=1) <= tol_rot).all())
                if c > 0:
                    out['rel'].append(abs(c - c1) / c)
                if small or abs(c - c1) <= tol_cost * c:
                    hist.append((c, c1, lam, DEC_STOP)); P, c, status = Pn, c1, 'converged'; break
                if c1 < c:
                    hist.append((c, c1, lam, DEC_ACCEPT)); P, c = Pn, c1; lam = max(lam / 10.0, 1e-12)
                else:
                    hist.append((c, c1, lam, DEC_REJECT)); lam *= 10.0
                    if lam > 1e12:
                        status = 'stalled'; break
        _, chi2, _, w, _ = self.edge_terms(P)
        out.update(poses=P, cost0=(np.nan if status == 'nonfinite' else hist[0][0] if hist else c), cost=(np.nan if status == 'nonfinite' else c),
                   iters=len(hist), status=status, history=np.asarray(hist, np.float64).reshape(-1, 4), weights=w, chi2=chi2)
        return out
