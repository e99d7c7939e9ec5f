"""High-precision reference of the Kabsch closes (csrc/polar.h, refine_body of csrc/ransac.hip, the fit of csrc/sc2.hip): mpmath at 60
digits.  float64 inputs enter exactly (a float64 is a binary rational; products of two of them are exact at 60 digits), so every figure here
is the exact value of the stated formula to ~1e-58 relative: far below anything a float64 kernel can be compared at."""
import numpy as np
from mpmath import mp, mpf, matrix, svd_r

DIGITS = 60
EPS = 2.0 ** -52


def _mat(H):
    H = np.asarray(H, np.float64)
    return matrix([[mpf(float(v)) for v in row] for row in H])


def to_float(A):
    return np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)], np.float64)


def _cross(A, a, b):
    """the cross product of columns a and b of a 3x3 mp matrix"""
    x, y = [A[i, a] for i in range(3)], [A[i, b] for i in range(3)]
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def polar(H):
    """H [3,3] float64 -> dict: S (three singular values, descending, float), R = U V^T, Rp = U diag(1, 1, det(U V^T)) V^T, det (+1 / -1, of
    U V^T), R2 = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T (the proper rotation of the two leading pairs: what rank 2 leaves defined).  R, Rp,
    R2 are mp matrices; diff() compares a float64 matrix with one of them."""
    with mp.workdps(DIGITS):
        U, S, Vt = svd_r(_mat(H), full_matrices=True, compute_uv=True)
        R = U * Vt
        d = mp.det(R)
        sign = 1 if d > 0 else -1
        D = matrix([[1, 0, 0], [0, 1, 0], [0, 0, sign]])
        Rp = U * D * Vt
        V = Vt.T
        u3, v3 = _cross(U, 0, 1), _cross(V, 0, 1)
        R2 = matrix(3, 3)
        for i in range(3):
            for j in range(3):
                R2[i, j] = U[i, 0] * V[j, 0] + U[i, 1] * V[j, 1] + u3[i] * v3[j]
        return dict(S=np.array([float(S[i]) for i in range(3)]), R=R, Rp=Rp, R2=R2, det=sign)


def diff(R, Rmp):
    """max |R - Rmp| with the subtraction in mpmath -> float"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    with mp.workdps(DIGITS):
        return float(max(abs(mpf(float(R[i, j])) - Rmp[i, j]) for i in range(3) for j in range(3)))


def kappa_uvt(S):
    """the conditioning of U V^T at H: sigma1 / (sigma2 + sigma3) (the polar factor moves by <= 2 |dH| / (sigma2 + sigma3))"""
    return S[0] / (S[1] + S[2]) if S[1] + S[2] > 0 else np.inf


def kappa_proper(S, det):
    """... of the proper rotation: sigma2 - sigma3 takes the sum's place where a reflection is fixed"""
    gap = S[1] + det * S[2]
    return S[0] / gap if gap > 0 else np.inf


def kabsch(k0, k1, w, rows, normalise=True):
    """The weighted Kabsch fit of the correspondences `rows`, k0 ~ R k1 + t, as refine_body states it: w' = w / sum w (normalise=False: w is
    normalised already and enters as it is), c0 = sum w' k0, c1 = sum w' k1, H = sum w' (k0 - c0)(k1 - c1)^T, R = U V^T of H, t = c0 - R c1.
    -> dict of float64 roundings H, c0, c1, R, t, S, det (of U V^T), and the mp values under 'mp' (H, c0, c1, R, t and the proper rotation
    Rp = U diag(1, 1, det) V^T); w None = ones."""
    rows = np.asarray(rows, np.int64)
    k0, k1 = np.asarray(k0, np.float64), np.asarray(k1, np.float64)
    with mp.workdps(DIGITS):
        ws = [mpf(1) if w is None else mpf(float(w[i])) for i in rows]
        if normalise:
            tot = sum(ws)
            ws = [v / tot for v in ws]
        a = [[mpf(float(k0[i, d])) for d in range(3)] for i in rows]
        b = [[mpf(float(k1[i, d])) for d in range(3)] for i in rows]
        c0 = [sum(ws[n] * a[n][d] for n in range(len(rows))) for d in range(3)]
        c1 = [sum(ws[n] * b[n][d] for n in range(len(rows))) for d in range(3)]
        H = matrix(3, 3)
        for n in range(len(rows)):
            da = [ws[n] * (a[n][d] - c0[d]) for d in range(3)]
            db = [b[n][d] - c1[d] for d in range(3)]
            for i in range(3):
                for j in range(3):
                    H[i, j] += da[i] * db[j]
        U, S, Vt = svd_r(H, full_matrices=True, compute_uv=True)
        R = U * Vt
        t = [c0[i] - sum(R[i, j] * c1[j] for j in range(3)) for i in range(3)]
        sign = 1 if mp.det(R) > 0 else -1
        Rp = U * matrix([[1, 0, 0], [0, 1, 0], [0, 0, sign]]) * Vt
        f = lambda v: np.array([float(x) for x in v], np.float64)
        return dict(H=to_float(H), c0=f(c0), c1=f(c1), R=to_float(R), t=f(t), S=f([S[i] for i in range(3)]), det=sign,
                    mp=dict(H=H, c0=c0, c1=c1, R=R, Rp=Rp, t=t))


def vec_diff(v, vmp):
    """|v - vmp| per element, the subtraction in mpmath -> float64 array of v's shape"""
    v = np.asarray(v, np.float64)
    flat = v.reshape(-1)
    ref = [vmp[i, j] for i in range(vmp.rows) for j in range(vmp.cols)] if isinstance(vmp, matrix) else list(vmp)
    with mp.workdps(DIGITS):
        return np.array([float(abs(mpf(float(flat[i])) - ref[i])) for i in range(flat.size)]).reshape(v.shape)
