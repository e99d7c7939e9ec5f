"""Seeded pose graphs shared by tests/test_pose_graph_oracle.py (CPU) and tests/test_hip_pose_graph.py (GPU).  Every family is named for
the condition it has to meet; the CPU file asserts those conditions on the oracle's own run, so that the GPU file may rely on them."""
import numpy as np

from _pose_graph_oracle import exp_so3, rigid_inv, topology

# C / E of the families whose device run has to match the oracle's round for round (a ring plus random closures; edge noise 5 mm / 0.5 deg)
MATCHED = ((3, 3), (12, 21), (33, 72), (43, 122))
# one node's block (6 unknowns) below / across / above the sizes at which the solve kernel's loops change their trip count: the 32-wide
# Cholesky panel (n = 24, 30 | 36), the 64-row trailing tile behind the first panel (n - 32 = 58 | 64, 70: n = 90, 96, 102) and the 128-row LDS
# stage of the panel below the diagonal block (n - 32 = 124 | 130, 136: n = 156, 162, 168).  n = 6 (C - 1).
SOLVE_EDGES = {'panel_below': 5, 'panel_last_inside': 6, 'panel_above': 7, 'tile_below': 16, 'tile_at': 17, 'tile_above': 18,
               'stage_below': 27, 'stage_above': 28, 'stage_above2': 29}
OUTLIERS = {(12, 21): 2, (43, 122): 6}
TAU = 0.1


def rot(axis, deg):
    axis = np.asarray(axis, np.float64)
    return exp_so3(axis / np.linalg.norm(axis) * np.deg2rad(deg))


def pose(R, t):
    P = np.eye(4); P[:3, :3] = R; P[:3, 3] = t
    return P


def random_pose(rng, max_deg, max_t):
    return pose(rot(rng.standard_normal(3), rng.uniform(0, max_deg)), rng.uniform(-max_t, max_t, 3))


def information(rng, m=1500):
    """The information matrix of m correspondences at random source points (dense_eval's definition: sum G^T G, G = [I | -2 [x]x])."""
    x = rng.uniform(-1.5, 1.5, (m, 3))
    L = np.zeros((6, 6))
    L[:3, :3] = m * np.eye(3)
    s = x.sum(0)
    K = -2.0 * np.array([[0, -s[2], s[1]], [s[2], 0, -s[0]], [-s[1], s[0], 0]])
    L[:3, 3:] = K; L[3:, :3] = K.T
    M = x.T @ x
    L[3:, 3:] = 4.0 * (np.trace(M) * np.eye(3) - M)
    return L


def ring_graph(seed, C, E, noise_t=0.005, noise_deg=0.5, n_outliers=0, flip=True):
    """-> dict(C, edges [E,2], T [E,4,4], Lam [E,6,6], truth [C,4,4] with truth[0] = I, outliers [indices]).  Ring 0-1-..-(C-1)-0 (for C = 2 the one
    edge) plus random closures up to E edges; about half of the edges are stored in the opposite orientation."""
    rng = np.random.default_rng(seed)
    truth = np.stack([np.eye(4)] + [random_pose(rng, 120.0, 2.0) for _ in range(C - 1)])
    pairs = [(c, (c + 1) % C) for c in range(C if C > 2 else 1)]
    while len(pairs) < E:
        i, j = rng.integers(0, C, 2)
        if i != j and abs(i - j) not in (1, C - 1):
            pairs.append((int(i), int(j)))
    edges, T, Lam = [], [], []
    for i, j in pairs:
        if flip and rng.random() < 0.5:
            i, j = j, i
        noise = pose(rot(rng.standard_normal(3), noise_deg * rng.uniform(0.2, 1.0)), rng.standard_normal(3) * noise_t / np.sqrt(3.0)) if noise_t or noise_deg else np.eye(4)
        edges.append((i, j)); T.append(rigid_inv(truth[i]) @ truth[j] @ noise); Lam.append(information(rng))
    out_idx = []
    if n_outliers:
        # gross edges are closures that the breadth-first walk from node 0 does not compose the initial poses along: a wrong edge in that
        # spanning tree is satisfied exactly by the start, and no local method can tell it from a right one
        used = {k for _, k in topology(C, edges, 0)[1]}
        out_idx = sorted(rng.choice([k for k in range(C, E) if k not in used], n_outliers, replace=False).tolist())
        for k in out_idx:
            T[k] = T[k] @ pose(rot(rng.standard_normal(3), np.rad2deg(0.5)), 0.5 * np.array([1.0, 0, 0]))
    return dict(C=C, edges=np.asarray(edges, np.int64), T=np.stack(T), Lam=np.stack(Lam), truth=truth, outliers=out_idx)


def matched(C, E, seed=0):
    return ring_graph(1000 + 37 * C + seed, C, E)


def with_outliers(C, E):
    return ring_graph(2000 + C, C, E, n_outliers=OUTLIERS[(C, E)])


def solve_edge(C):
    return ring_graph(3000 + C, C, 2 * C if C > 4 else C)


def perturbed(truth, seed, deg, t, anchor=0):
    """truth with every pose but the anchor's moved by exactly deg degrees about a random axis and t metres in a random direction."""
    rng = np.random.default_rng(seed)
    out = truth.copy()
    for c in range(truth.shape[0]):
        if c != anchor:
            d = rng.standard_normal(3)
            out[c] = truth[c] @ pose(rot(rng.standard_normal(3), deg), d / np.linalg.norm(d) * t)
    return out


def far_start(seed=53):
    """C = 12 / E = 21, started 2 rad / 0.5 m off: the run must contain rejected rounds (most seeds have none: the quaternion residual saturates; 53 has three)."""
    g = ring_graph(4000 + seed, 12, 21)
    g['init'] = perturbed(g['truth'], 4100 + seed, np.rad2deg(2.0), 0.5)
    return g


def tree(seed, C):
    """A random tree, noise free: every node hangs off an earlier one."""
    rng = np.random.default_rng(seed)
    truth = np.stack([np.eye(4)] + [random_pose(rng, 120.0, 2.0) for _ in range(C - 1)])
    edges = [(int(rng.integers(0, c)), c) if rng.random() < 0.5 else (c, int(rng.integers(0, c))) for c in range(1, C)]
    T = np.stack([rigid_inv(truth[i]) @ truth[j] for i, j in edges])
    return dict(C=C, edges=np.asarray(edges, np.int64), T=T, Lam=np.stack([information(rng) for _ in edges]), truth=truth, outliers=[])


def noise_free_loop(seed, C, E):
    g = ring_graph(seed, C, E, noise_t=0.0, noise_deg=0.0)
    g['init'] = perturbed(g['truth'], seed + 1, 5.0, 0.1)
    return g
