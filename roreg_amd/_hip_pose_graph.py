"""ctypes binding of the pose-graph optimiser (csrc/pose_graph.hip; include/roreg_hip.h "v6h"): part of the `roreg_amd.hip` namespace (hip.py
re-exports everything here).  The topology -- reachability from the anchor, the incidence lists, the order in which initial poses are
composed -- is integer work and is done here on the host; every floating-point operation runs on the device."""
from collections import deque, namedtuple

import numpy as np
import torch

from ._abi import _PG_GRAPH
from .hip import HipError, _check, _ptr, _stream, lib, upload

__all__ = ['PG_STATUS', 'PG_DECISION', 'PG_MAX_NODES', 'PG_MAX_EDGES', 'PG_LIN', 'PG_PANEL', 'PG_TILE', 'PgGraph', 'PgDev', 'pg_topology',
           'pg_optimize_batch', 'pg_dense_jacobians']

PG_STATUS = ('converged', 'max_iter', 'stalled', 'nonfinite')
PG_DECISION = ('none', 'accepted', 'rejected', 'rejected_pivot', 'stopped')
PG_MAX_NODES, PG_MAX_EDGES = 256, 65536
PG_LIN = 56                              # doubles per edge record of the first round's table (csrc/pose_graph.hip PG_LIN)
PG_PANEL, PG_TILE = 32, 64               # the Cholesky's panel width and its trailing update's tile (PG_NB, PG_TILE)

PgGraph = namedtuple('PgGraph', 'n_nodes edges transforms infos init anchor tau lambda0 tol_t tol_rot tol_cost',
                     defaults=(None, 0, None, 1e-3, 1e-9, 1e-9, 1e-10))
PgGraph.__doc__ = ('one graph of pg_optimize_batch: n_nodes; edges int [E,2] on the host, rows (i, j); transforms f64 [E,4,4] and infos f64 [E,6,6] '
                   'device tensors; init f64 [n_nodes,4,4] device tensor or None (compose the transforms along a breadth-first walk from the '
                   'anchor); tau: the robust kernel\'s scale in metres or None')
PgDev = namedtuple('PgDev', 'poses cost iters status weights chi2 history reached node0 edge0 act0 pieces')
PgDev.__doc__ = ('device tensors over the whole batch: poses f64 [C_total,4,4], cost f64 [G,2] = (start, final), iters / status int32 [G], weights / '
                 'chi2 f64 [E_total], history f64 [G,max_iter,4]; host: reached [bool [C]] per graph and the graphs\' first node / edge / optimised '
                 'node in the batch tables; pieces = None or (lin [E_total,56], H [flat], g [6 A_total], delta [6 A_total]) of the first round')


def pg_topology(n_nodes, edges, anchor):
    """-> (reached bool [C], var int32 [C], inc [C lists of edge numbers, ascending], walk int32 [A,2]).  Breadth-first from the anchor; a
    node's incident edges are visited in ascending edge number, and a node is entered by the first edge that reaches it."""
    C = int(n_nodes)
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    if not 1 <= C <= PG_MAX_NODES:
        raise HipError(f'pose graph: {C} nodes; a graph has 1 to {PG_MAX_NODES}')
    if edges.shape[0] > PG_MAX_EDGES:
        raise HipError(f'pose graph: {edges.shape[0]} edges; a graph has at most {PG_MAX_EDGES}')
    if not 0 <= int(anchor) < C:
        raise HipError(f'pose graph: anchor {anchor} is not a node')
    if edges.size and (edges.min() < 0 or edges.max() >= C or (edges[:, 0] == edges[:, 1]).any()):
        raise HipError('pose graph: an edge names a node outside the graph or joins a node to itself')
    inc = [[] for _ in range(C)]
    for k, (i, j) in enumerate(edges.tolist()):
        inc[i].append(k); inc[j].append(k)
    reached = np.zeros(C, bool); reached[anchor] = True
    walk, queue = [], deque([int(anchor)])
    while queue:
        u = queue.popleft()
        for k in inc[u]:
            v = int(edges[k, 0] + edges[k, 1]) - u
            if not reached[v]:
                reached[v] = True
                walk.append((v, k)); queue.append(v)
    var = np.full(C, -1, np.int32)
    act = np.flatnonzero(reached & (np.arange(C) != anchor))
    var[act] = np.arange(act.shape[0], dtype=np.int32)
    return reached, var, inc, np.asarray(walk, np.int32).reshape(-1, 2)


def _i32(values):
    return upload(np.ascontiguousarray(np.asarray(values, np.int32).reshape(-1))) if len(values) else None


def pg_optimize_batch(graphs, max_iter=100, want_pieces=False):
    """graphs: [PgGraph] -> PgDev.  All max_iter rounds of every graph are enqueued in this call and nothing returns to the host.  Either
    every graph brings initial poses or none does.  A graph's bits depend neither on the batch nor on its place in it."""
    graphs = [g if isinstance(g, PgGraph) else PgGraph(*g) for g in graphs]
    G, max_iter = len(graphs), int(max_iter)
    if max_iter < 0:
        raise HipError('pg_optimize_batch: max_iter must be >= 0')
    if G == 0:
        raise HipError('pg_optimize_batch: no graph')
    has_init = graphs[0].init is not None
    if any((g.init is not None) != has_init for g in graphs):
        raise HipError('pg_optimize_batch: either every graph brings initial poses or none does')
    table = np.zeros(G, _PG_GRAPH)
    reached_all, var_all, inc_ptr, inc_edge, act_graph, act_node, walk_all, ei, ej, eg = [], [], [0], [], [], [], [], [], [], []
    node0 = edge0 = act0 = h0 = 0
    dev = graphs[0].transforms.device
    for b, g in enumerate(graphs):
        edges = np.asarray(g.edges, np.int64).reshape(-1, 2)
        E, C = edges.shape[0], int(g.n_nodes)
        reached, var, inc, walk = pg_topology(C, edges, g.anchor)
        if tuple(g.transforms.shape) != (E, 4, 4) or tuple(g.infos.shape) != (E, 6, 6):
            raise HipError('pg_optimize_batch: transforms must be [E,4,4] and infos [E,6,6]')
        _ptr(g.transforms, torch.float64); _ptr(g.infos, torch.float64)
        if has_init:
            _ptr(g.init, torch.float64)
            if tuple(g.init.shape) != (C, 4, 4):
                raise HipError('pg_optimize_batch: init must be [n_nodes,4,4]')
        tau = 0.0 if g.tau is None else float(g.tau)
        if g.tau is not None and not tau > 0.0:
            raise HipError('pg_optimize_batch: robust_tau must be positive (None = no robust kernel)')
        n_act = int((var >= 0).sum())
        table[b] = (node0, C, edge0, E, act0, n_act, int(g.anchor), 0, h0, tau, float(g.lambda0), float(g.tol_t), float(g.tol_rot),
                    float(g.tol_cost), 0.0)
        reached_all.append(reached); var_all.append(var)
        for c in range(C):
            inc_edge.extend(edge0 + k for k in inc[c]); inc_ptr.append(len(inc_edge))
        act = np.flatnonzero(var >= 0)
        act_graph.extend([b] * n_act); act_node.extend(act.tolist())
        walk[:, 1] += edge0
        walk_all.append(walk)
        ei.extend(edges[:, 0].tolist()); ej.extend(edges[:, 1].tolist()); eg.extend([b] * E)
        node0 += C; edge0 += E; act0 += n_act; h0 += (6 * n_act) ** 2
    Ct, Et, At = node0, edge0, act0
    ws_n = lib().roreg_pg_workspace(table.ctypes.data, G)
    if ws_n == 0:
        raise HipError(f'pg_optimize_batch: a graph exceeds {PG_MAX_NODES} nodes or {PG_MAX_EDGES} edges')
    tdev = upload(table.view(np.uint8).reshape(G, _PG_GRAPH.itemsize))
    T = torch.cat([g.transforms.reshape(-1, 16) for g in graphs]).contiguous()
    Lam = torch.cat([g.infos.reshape(-1, 36) for g in graphs]).contiguous()
    poses = (torch.cat([g.init.reshape(-1, 16) for g in graphs]).contiguous().clone() if has_init
             else torch.empty((Ct, 16), dtype=torch.float64, device=dev))
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    cost, weights, chi2, history = f64(G, 2), f64(max(Et, 1)), f64(max(Et, 1)), f64(G, max(max_iter, 1), 4)
    iters = torch.empty(G, dtype=torch.int32, device=dev); status = torch.empty_like(iters)
    lin = H = gd = None
    if want_pieces:
        lin, H, gd = f64(max(Et, 1), PG_LIN), f64(max(h0, 1)), f64(2, max(6 * At, 1))
    ws = torch.empty(max(ws_n, 8), dtype=torch.uint8, device=dev)
    walk_np = np.concatenate(walk_all) if walk_all else np.zeros((0, 2), np.int32)
    tabs = [_i32(ei), _i32(ej), _i32(eg)]
    vdev, pdev, iedev = _i32(np.concatenate(var_all)), _i32(inc_ptr), _i32(inc_edge)
    agdev, andev, wdev = _i32(act_graph), _i32(act_node), _i32(walk_np.reshape(-1))
    _check(lib().roreg_pg_optimize_batch(table.ctypes.data, _ptr(tdev), G, _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), _ptr(T) if Et else None,
                                         _ptr(Lam) if Et else None, _ptr(vdev), _ptr(pdev), _ptr(iedev), _ptr(agdev), _ptr(andev), _ptr(wdev),
                                         int(has_init), max_iter, _ptr(poses), _ptr(cost), _ptr(iters), _ptr(status), _ptr(weights), _ptr(chi2),
                                         _ptr(history), _ptr(lin), _ptr(H), _ptr(gd), _ptr(ws), ws_n, _stream()), 'roreg_pg_optimize_batch')
    pieces = (lin[:Et], H[:h0], gd[0, :6 * At], gd[1, :6 * At]) if want_pieces else None
    return PgDev(poses.view(Ct, 4, 4), cost, iters, status, weights[:Et], chi2[:Et], history[:, :max_iter], reached_all,
                 table['node0'].tolist(), table['edge0'].tolist(), table['act0'].tolist(), pieces)


def pg_dense_jacobians(lin):
    """The first round's edge records (numpy [E,56]) -> (e [E,6], chi2 [E], w [E], J_i [E,6,6], J_j [E,6,6])."""
    lin = np.asarray(lin, np.float64).reshape(-1, PG_LIN)
    E = lin.shape[0]
    RE, Q, A, B, D = (lin[:, o:o + 9].reshape(E, 3, 3) for o in (8, 17, 26, 35, 44))
    Jj = np.zeros((E, 6, 6)); Ji = np.zeros((E, 6, 6))
    Jj[:, :3, :3] = RE; Jj[:, 3:, 3:] = Q
    Ji[:, :3, :3] = -A; Ji[:, :3, 3:] = -B; Ji[:, 3:, 3:] = -D
    return lin[:, :6], lin[:, 6], lin[:, 7], Ji, Jj
