"""Spatial-compatibility estimator: registration from the matched keypoints alone -- no ET network, no equivariant features, no random
numbers (csrc/sc2.hip; no reference counterpart: the reference's estimators are yohoo and yohoc).

    from roreg_amd import sc2
    Trans = sc2.hypotheses(keys0, keys1, matches)                       # [S,3,4] float64, seed order
    res = sc2.register(keys0, keys1, matches, scores, ird=0.1)          # one pair -> Sc2Result
    res = sc2.register([(keys0, keys1, matches, scores), ...], ird=0.1)    # many pairs, the same launches -> [Sc2Result]

Two correct correspondences preserve their mutual distance, so the correspondences compatible with a seed AND with each other are almost free
of outliers; the Kabsch transform of the K best of them is the seed's hypothesis.  The hypotheses are scored over all correspondences and
the winner refined twice by the kernels the other estimators use (hip.ransac_batch).  keys0 / keys1 [*,3] and matches [M,2] (rows of keys0,
rows of keys1; None = the keys are the correspondences, row by row) are host arrays or device tensors; transforms follow the engine's
convention k0 ~ k1 R^T + t.  RegistrationEngine with cfg.ET = 'sc2' is the device-resident form."""
from collections import namedtuple

import numpy as np
import torch

from . import hip

Sc2Result = namedtuple('Sc2Result', 'T row stats n_hyp')
Sc2Result.__doc__ = ('T [4,4] float64 (NaN rotation and translation when there is no correspondence); row: 0-based row of the winning hypothesis '
                     '(seed order; -1 when no hypothesis has an inlier); stats f64 [2,16]: the two refinements\' H (9), c0 (3), c1 (3), sum of '
                     'weights; n_hyp: hypotheses scored')
MAX_SEEDS, K = 1000, 20


def _device(a, dtype, cols):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1, cols)))
    return t.to(device='cuda', dtype=dtype).reshape(-1, cols).contiguous()


def _task(keys0, keys1, matches):
    k0, k1 = _device(keys0, torch.float64, 3), _device(keys1, torch.float64, 3)
    if matches is None:
        if k0.shape[0] != k1.shape[0]:
            raise ValueError('sc2: without matches, keys0 and keys1 must hold one correspondence per row')
        m = torch.arange(k0.shape[0], dtype=torch.int64, device='cuda')
        m = torch.stack([m, m], 1).contiguous()
    else:
        m = _device(matches, torch.int64, 2)
    return k0, k1, m


def hypotheses(keys0, keys1, matches=None, tau=0.1, max_seeds=MAX_SEEDS, k=K):
    """-> Trans [S,3,4] float64 on the device, S = min(M, max_seeds): row h is the hypothesis of the seed of h-th greatest degree."""
    Trans, _ = hip.sc2_hypotheses_batch([_task(keys0, keys1, matches)], tau, max_seeds, k)
    return Trans


def estimate_finish(T_host, st_host, rctx, ird, host_svd=False):
    """The host half of register: T_host [n,4,4], st_host [n,2,16] = the downloaded second refinements and both refinements' statistics.  A rank-deficient
    cross-covariance (<= 2 inliers, coplanar inliers) has no unique U V^T: those pairs are closed by LAPACK like the other estimators' -> T_host."""
    from .test.estimator import _kabsch_host
    T_host = np.array(T_host)
    n = T_host.shape[0]
    deficient = hip.stats_rank_deficient_many(st_host).any(axis=1) if n else np.zeros(0, bool)
    redo = [i for i in range(n) if deficient[i] or host_svd]
    if redo:
        T1s = np.stack([_kabsch_host(st_host[i, 0]) for i in redo])
        st_redo = hip.refine_batch(rctx, redo, T1s, float(ird))[1].cpu().numpy()
        for i, st in zip(redo, st_redo):
            T_host[i] = _kabsch_host(st)
    return T_host


def register(keys0, keys1=None, matches=None, scores=None, ird=0.1, tau=None, max_seeds=MAX_SEEDS, k=K, host_svd=False):
    """One pair (keys0, keys1, matches, scores) -> Sc2Result, or keys0 = a list of such tuples (matches / scores may be None or left out)
    -> [Sc2Result].  scores: the match scores that weigh overlap and refinement (None = ones; a float32 array is summed the way numpy sums
    float32, like the rotation-coherence matcher's); they take no part in generating the hypotheses.  tau: the compatibility threshold
    (None = ird)."""
    single = keys1 is not None
    items = [(keys0, keys1, matches, scores)] if single else [tuple(it) + (None,) * (4 - len(it)) for it in keys0]
    tasks = [_task(a, b, m) for a, b, m, _ in items]
    sc = [None if s is None else (s.cpu().numpy() if torch.is_tensor(s) else np.asarray(s)) for _, _, _, s in items]
    for (_, _, m), s in zip(tasks, sc):
        if s is not None and s.shape != (int(m.shape[0]),):
            raise ValueError('sc2.register: scores must hold one value per correspondence')
    w_f32 = any(s is not None and s.dtype == np.float32 for s in sc)
    weights = [None if s is None else hip.upload(s.astype(np.float64)) for s in sc]
    # the launches RegistrationEngine issues under cfg.ET = 'sc2' (_sc2_tasks, then the estimator tail): no host synchronisation up to here
    Trans, offsets = hip.sc2_hypotheses_batch(tasks, float(ird) if tau is None else float(tau), max_seeds, k)
    rt = [(k0, k1, m, w, Trans[o:o + S], None) for (k0, k1, m), w, (o, S) in zip(tasks, weights, offsets)]
    best, T1, st1, T2, st2, rctx = hip.ransac_batch(rt, float(ird), w_f32=w_f32, keep=True)
    st_host = torch.stack([st1, st2], 1).cpu().numpy()
    T_host = estimate_finish(T2.cpu().numpy(), st_host, rctx, ird, host_svd)
    best = best.cpu().numpy()
    out = []
    for i, (_, _, m) in enumerate(tasks):
        T = T_host[i]
        if int(m.shape[0]) == 0:
            T = np.full((4, 4), np.nan); T[3] = [0.0, 0.0, 0.0, 1.0]
        out.append(Sc2Result(T, int(best[i]) if int(m.shape[0]) else -1, st_host[i], int(rt[i][4].shape[0])))
    return out[0] if single else out
