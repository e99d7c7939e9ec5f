"""numpy restatement of the dense pair evaluation (include/roreg_hip.h "v6g"; roreg_amd/csrc/icp.hip): what the device must compute.

Coordinates are float32 values widened to float64; T [4,4] float64 with target ~ source R^T + t (cloud 0 the target, cloud 1 the source).
  forward : the v6c search of every source point under (R, t) (tests/_icp_oracle.py transform + nearest: lowest row on an exact tie, a
            correspondence iff d2 <= d d); over the correspondences, x the UNtransformed source point: n01, S01 = sum d2, sum x, sum x x^T;
  backward: the same search of every target point among the source points under Rinv = R^T,
            tinv_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2): n10, S10;
  rmse = sqrt(S / n) (NaN without correspondences), overlap1 = n01 / n_src, overlap0 = n10 / n_tgt (NaN for an empty cloud);
  Lambda = sum G^T G, G = [I | -2 [x]x]: Lambda_tt = n01 I, Lambda_tr = -2 [sum x]x, Lambda_rr = 4 (tr(M) I - M), M = sum x x^T.
A non-finite T: status 'nonfinite', no correspondences.
Every sum is returned as (math.fsum of its terms, bound): |device - fsum| <= n 2^-52 sum |term| + 4 ulp holds for ANY order of summation
(n - 1 roundings of relative size 2^-53 at most, a factor 2 of margin), so nothing here is measured from the code under test."""
import math
from collections import namedtuple

import numpy as np

import _icp_oracle as O

STATUS = ('ok', 'nonfinite')
Eval = namedtuple('Eval', 'n01 n10 overlap0 overlap1 rmse01 rmse10 S01 S10 sx M info info_bound assign01 assign10 status x')
Eval.__doc__ = ('S01, S10: (value, bound); sx: [(value, bound)] * 3; M: {(i, j): (value, bound)}, i <= j; info [6,6] from the fsum moments and '
                'info_bound [6,6] its entrywise bound; x: the corresponding source points [n01,3] in source row order')


def widen(P):
    return np.asarray(P, np.float32).astype(np.float64).reshape(-1, 3)


def bounded_sum(terms):
    """-> (math.fsum(terms), n 2^-52 sum |terms| + 4 ulp of the sum)."""
    terms = [float(v) for v in terms]
    s = math.fsum(terms)
    return s, len(terms) * 2.0 ** -52 * math.fsum(abs(v) for v in terms) + 4.0 * float(np.spacing(abs(s)))


def inverse(R, t):
    """The inverse by transposition, as the device forms it."""
    return np.ascontiguousarray(R.T), np.array([-((R[0, r] * t[0] + R[1, r] * t[1]) + R[2, r] * t[2]) for r in range(3)])


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def information(n, sx, M, factor=2.0):
    """The closed form from the moments (M symmetric [3,3]); factor = 2 is the convention (the quaternion's half angle)."""
    L = np.zeros((6, 6))
    L[:3, :3] = n * np.eye(3)
    L[:3, 3:] = 0.0 - factor * skew(sx)          # (0 - x: a zero entry is +0, as on the device)
    L[3:, :3] = L[:3, 3:].T
    L[3:, 3:] = factor * factor * (np.trace(M) * np.eye(3) - M)
    return L


def information_literal(x, factor=2.0):
    """sum G^T G over the points x [n,3], G = [I | -factor [x]x], formed point by point."""
    L = np.zeros((6, 6))
    for p in x:
        G = np.concatenate([np.eye(3), -factor * skew(p)], 1)
        L += G.T @ G
    return L


def evaluate(Q, P, T, d, nn=O.nearest):
    Q, P = widen(Q), widen(P)
    T = np.array(T, np.float64)
    nan = float('nan')
    zero = (0.0, 0.0)
    if not np.isfinite(T[:3]).all():
        return Eval(0, 0, 0.0 / Q.shape[0] if Q.shape[0] else nan, 0.0 / P.shape[0] if P.shape[0] else nan, nan, nan, zero, zero, [zero] * 3,
                    {(i, j): zero for i in range(3) for j in range(i, 3)}, np.zeros((6, 6)), np.zeros((6, 6)),
                    np.full(P.shape[0], -1, np.int32), np.full(Q.shape[0], -1, np.int32), 'nonfinite', np.zeros((0, 3)))
    R, t = T[:3, :3], T[:3, 3]
    a01, d01 = nn(Q, O.transform(P, R, t), d)
    Ri, ti = inverse(R, t)
    a10, d10 = nn(P, O.transform(Q, Ri, ti), d)
    f, b = a01 >= 0, a10 >= 0
    n01, n10 = int(f.sum()), int(b.sum())
    x = P[f]
    S01, S10 = bounded_sum(d01[f]), bounded_sum(d10[b])
    sx = [bounded_sum(x[:, i]) for i in range(3)]
    M = {(i, j): bounded_sum(x[:, i] * x[:, j]) for i in range(3) for j in range(i, 3)}
    Mv = np.zeros((3, 3)); Mb = np.zeros((3, 3))
    for (i, j), (v, e) in M.items():
        Mv[i, j] = Mv[j, i] = v; Mb[i, j] = Mb[j, i] = e
    info = information(n01, np.array([v for v, _ in sx]), Mv)
    bound = np.zeros((6, 6))
    bound[:3, 3:] = 2.0 * np.abs(skew(np.array([e for _, e in sx])))
    bound[3:, :3] = bound[:3, 3:].T
    bound[3:, 3:] = 4.0 * Mb
    for i in range(3):                    # diagonal of Lambda_rr: the 2 n terms 4 x_j^2, 4 x_k^2 of the two other axes, n01 terms per moment
        j, k = (i + 1) % 3, (i + 2) % 3
        v, e = bounded_sum(np.concatenate([4.0 * x[:, j] * x[:, j], 4.0 * x[:, k] * x[:, k]]))
        info[3 + i, 3 + i] = v; bound[3 + i, 3 + i] = e
    rm = lambda S, n: math.sqrt(S[0] / n) if n else nan
    return Eval(n01, n10, n10 / Q.shape[0] if Q.shape[0] else nan, n01 / P.shape[0] if P.shape[0] else nan, rm(S01, n01), rm(S10, n10), S01, S10, sx, M,
                info, bound, a01, a10, 'ok', x)


def rmse_bound(S, n):
    """What |device rmse - sqrt(S / n)| may be: half the sum's relative bound (the square root halves it), and 4 ulp for the division and the
    square root."""
    want = math.sqrt(S[0] / n)
    return (0.5 * S[1] / S[0] * want * (1.0 + 1e-6) if S[0] > 0 else 0.0) + 4.0 * float(np.spacing(want))


def mean_squared_displacement(x, E):
    """Directly: the mean of |E x - x|^2 over the points x [n,3] under the rigid perturbation E [4,4]."""
    y = x @ E[:3, :3].T + E[:3, 3]
    return float((((y - x) ** 2).sum(1)).mean())
