"""The spatial-compatibility hypothesis generator restated in numpy (include/roreg_hip.h "v6m"): what csrc/sc2.hip is
tested against.  Stands alone: imports nothing of roreg_amd.

Inputs P, Q float64 [M,3] (P = keys0[matches[:,0]], Q = keys1[matches[:,1]]), tau, max_seeds, K.
  1. a_ij = sqrt((dx dx + dy dy) + dz dz) of P_i - P_j, b_ij likewise of Q;  C_ij = [i != j and |a_ij - b_ij| <= tau]
  2. deg_i = sum_j C_ij;  seeds = the S = min(M, max_seeds) rows of greatest degree, ties to the lower index
  3. N2[s, j] = C[s, j] sum_k C[s, k] C[k, j]
  4. set(s) = s, then at most K - 1 of the j with C[s, j] = 1 by greater N2[s, j], ties to the lower j
  5. >= 3 members: the unweighted Kabsch fit P ~ R Q + t over the set, det R = +1 (the sign on the smallest singular direction);
     fewer: R = I, t = P_s - Q_s."""
from collections import namedtuple

import numpy as np

Sc2 = namedtuple('Sc2', 'diff C bits deg seeds N2 cons Trans sigma')
Sc2.__doc__ = ('diff [M,M] = |a - b|, C bool [M,M], bits uint64 [M, ceil(M/64)] (bit j % 64 of word j / 64 = C[i, j]), deg int32 [M], seeds int32 [S], '
               'N2 uint16 [S,M], cons int32 [S,K] (-1 padded), Trans f64 [S,3,4], sigma f64 [S,3] (singular values of the fitted sets, NaN for sets of < 3)')


def pair_distances(X):
    d = X[:, None, :] - X[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def pack_bits(C):
    """bool [M,M] -> uint64 [M, ceil(M/64)], zero padded."""
    M = C.shape[0]
    W = (M + 63) // 64
    padded = np.zeros((M, W * 64), np.uint8)
    padded[:, :M] = C
    return np.ascontiguousarray(np.packbits(padded.reshape(M, W, 64), axis=-1, bitorder='little')).view(np.uint64).reshape(M, W)


def kabsch(p, q):
    """The rotation and translation with p ~ R q + t, det R = +1 -> (R, t, singular values)."""
    cp, cq = p.mean(0), q.mean(0)
    H = (q - cq).T @ (p - cp)
    U, sv, VT = np.linalg.svd(H)
    d = np.sign(np.linalg.det(VT.T @ U.T))
    R = VT.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    return R, cp - R @ cq, sv


def hypotheses(P, Q, tau, max_seeds=1000, K=20):
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3); Q = np.ascontiguousarray(Q, np.float64).reshape(-1, 3)
    M = P.shape[0]
    diff = np.abs(pair_distances(P) - pair_distances(Q))
    C = diff <= tau
    C[np.arange(M), np.arange(M)] = False
    deg = C.sum(1).astype(np.int32)
    S = min(M, int(max_seeds))
    seeds = np.argsort(-deg.astype(np.int64), kind='stable')[:S].astype(np.int32)
    Cf = C.astype(np.float32)                                      # counts <= M < 2^24: exact in float32
    N2 = ((Cf[seeds] @ Cf) * Cf[seeds]).astype(np.uint16).reshape(S, M)
    cons = np.full((S, K), -1, np.int32)
    Trans = np.zeros((S, 3, 4))
    sigma = np.full((S, 3), np.nan)
    for h, s in enumerate(seeds):
        js = np.where(C[s])[0]
        js = js[np.argsort(-N2[h, js].astype(np.int64), kind='stable')][:K - 1]
        members = np.concatenate([[s], js]).astype(np.int64)
        cons[h, :members.shape[0]] = members
        if members.shape[0] >= 3:
            R, t, sigma[h] = kabsch(P[members], Q[members])
        else:
            R, t = np.eye(3), P[s] - Q[s]
        Trans[h, :, :3] = R; Trans[h, :, 3] = t
    return Sc2(diff, C, pack_bits(C), deg, seeds, N2, cons, Trans, sigma)


def threshold_margin(diff, tau):
    """The least distance of an off-diagonal |a_ij - b_ij| from tau (inf for M < 2)."""
    M = diff.shape[0]
    off = ~np.eye(M, dtype=bool)
    return float(np.abs(diff[off] - tau).min()) if M > 1 else float('inf')
