"""Multiway registration on the device: Levenberg-Marquardt optimisation of a scene's pose graph (csrc/pose_graph.hip, include/roreg_hip.h
"v6h"; no reference counterpart: the reference stops at pairwise transforms).

    from roreg_amd import pose_graph
    r = pose_graph.optimize(n_nodes, edges, transforms, infos)                       # one graph -> PoseGraphResult
    rs = pose_graph.optimize([(n_nodes, edges, transforms, infos), ...], robust_tau=0.1)   # several graphs, the same launches
    T_ij = pose_graph.implied_pairs(r.poses, pairs)                                  # inv(P_i) @ P_j per pair

edges int [E,2], rows (i, j); transforms [E,4,4]: T_k maps cloud j into cloud i (the engine's PairResult transform for (id0 = i, id1 = j));
infos [E,6,6]: the information matrices of dense_eval / evaluate_many.  poses [C,4,4] map every cloud into the world; the anchor keeps its
initial pose (the identity without init=).  The residual is the benchmark's own error measure, RR_cal.computeTransformationErr;
robust_tau (metres) turns on the Geman-McClure kernel that votes wrong pairs down.  RegistrationEngine.optimize_poses is the
device-resident form."""
from collections import namedtuple

import numpy as np
import torch

from . import hip

PoseGraphResult = namedtuple('PoseGraphResult', 'poses reached cost0 cost iters status weights chi2 history')
PoseGraphResult.__doc__ = ("poses [C,4,4] float64; reached bool [C]: the nodes connected to the anchor (the others keep their initial pose); cost0, cost: "
                           "before and after; iters: rounds run; status: 'converged' | 'max_iter' | 'stalled' | 'nonfinite' (poses = the initial ones); "
                           "weights, chi2 [E] at the final poses; history [iters,4] = (c, c', lambda, decision as in hip.PG_DECISION)")

LAMBDA0, TOL_T, TOL_ROT, TOL_COST = 1e-3, 1e-9, 1e-9, 1e-10


def _dev(a, shape, device):
    if torch.is_tensor(a):
        return a.to(device=device, dtype=torch.float64).reshape(shape).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))).to(device)


def results_to_host(dev, graphs):
    """pg_optimize_batch's PgDev -> [PoseGraphResult] (one synchronising copy per table)."""
    poses, cost, iters, status, weights, chi2, history = (v.cpu().numpy() for v in (dev.poses, dev.cost, dev.iters, dev.status, dev.weights, dev.chi2,
                                                                                   dev.history))
    out = []
    for b, g in enumerate(graphs):
        n0, e0, E = dev.node0[b], dev.edge0[b], int(np.asarray(g.edges).reshape(-1, 2).shape[0])
        out.append(PoseGraphResult(poses[n0:n0 + g.n_nodes].copy(), dev.reached[b].copy(), float(cost[b, 0]), float(cost[b, 1]), int(iters[b]),
                                   hip.PG_STATUS[int(status[b])], weights[e0:e0 + E].copy(), chi2[e0:e0 + E].copy(), history[b, :int(iters[b])].copy()))
    return out


def optimize(n_nodes, edges=None, transforms=None, infos=None, init=None, anchor=0, robust_tau=None, max_iter=100, lambda0=LAMBDA0, tol_t=TOL_T,
             tol_rot=TOL_ROT, tol_cost=TOL_COST, device='cuda'):
    """One graph -> PoseGraphResult, or a list of (n_nodes, edges, transforms, infos[, init[, anchor]]) tuples as the first argument ->
    [PoseGraphResult]; the keyword options then hold for every graph of the list."""
    single = edges is not None
    items = [(n_nodes, edges, transforms, infos, init, anchor)] if single else [tuple(it) for it in n_nodes]
    graphs = []
    for it in items:
        C, ed, T, L = it[:4]
        ini = it[4] if len(it) > 4 else init
        anc = it[5] if len(it) > 5 else anchor
        ed = np.asarray(ed, np.int64).reshape(-1, 2)
        E = ed.shape[0]
        graphs.append(hip.PgGraph(int(C), ed, _dev(T, (E, 4, 4), device), _dev(L, (E, 6, 6), device),
                                  None if ini is None else _dev(ini, (int(C), 4, 4), device), int(anc), robust_tau, lambda0, tol_t, tol_rot, tol_cost))
    out = results_to_host(hip.pg_optimize_batch(graphs, max_iter), graphs)
    return out[0] if single else out


def implied_pairs(poses, pairs):
    """The pair transforms a set of world poses implies: inv(P_i) @ P_j for every (i, j) -> [n,4,4] float64 (host)."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.stack([np.linalg.inv(poses[i]) @ poses[j] for i, j in pairs]) if pairs.shape[0] else np.zeros((0, 4, 4))
