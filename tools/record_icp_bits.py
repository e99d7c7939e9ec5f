"""Record what the dense-ICP family (csrc/icp.hip) returns, bit for bit, so that a restructuring of its kernels can be shown to change nothing.

    python tools/record_icp_bits.py [--out tests/golden/icp_parent_bits.npz]

Runs a fixed case set on the GPU and writes every returned tensor: floats as their integer bit patterns, assignments as they are, and the
hash of the commit whose kernels produced them.  No inputs are stored: they come from the seeded case functions of tests/_icp_cases.py
and tests/_icp_plane_cases.py (the evaluation runs on the chunk pairs, as tests/_dense_eval_cases.py's chunk family does).  Runs in a git
checkout only, and refuses while roreg_amd/csrc or include differ from HEAD: the library must be that commit's.
tests/test_hip_icp_edges.py::test_refactor_keeps_the_parents_bits recomputes run_cases() and compares with np.array_equal.

The case set (the smallest shapes at which the shared skeleton can go wrong):
  chunk       -- C.chunk_pairs() in one batch (sources of 1 .. 3073 points across the 64 / 256 / 1024 / 2048 / 3072 boundaries, targets of
                 1 .. 1025), point and plane method, and the same batch reversed;
  solve       -- C.solve_family() at max_iter = 1 with the statistics: both determinant signs, rank rejections, sixteen decades of H;
  wall        -- the C.WALL_SEEDS pairs: the determinant fix in mid-run;
  rank        -- the plane method on one, two and three exact planes and on the walls (tests/test_hip_icp_plane.py's rank family);
  degenerate  -- a non-finite T0 and an empty source, both methods;
  eval        -- hip.icp_eval_batch on the chunk pairs with both assignment directions."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'icp_parent_bits.npz')
_BITS = {np.dtype(np.float64): np.int64, np.dtype(np.float32): np.int32}


def _host(t):
    """device tensor -> numpy array, a float array as its integer bit pattern (NaN payloads and signed zeros compare as bits)"""
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(_BITS[a.dtype]) if a.dtype in _BITS else a


def run_cases():
    """-> {name: array}: every tensor the case set returns, from the library that roreg_amd.hip loads."""
    import torch

    import _icp_cases as C
    import _icp_plane_cases as PC
    from roreg_amd import hip
    out, grids = {}, {}

    def grid(p, d):
        key = (p.ctypes.data, p.shape[0], d)
        if key not in grids:
            grids[key] = (hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d), p)       # (p kept: its address is the key)
        return grids[key][0]

    dev = lambda T: torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()

    def put(name, res, fields):
        for f, v in zip(fields, res):
            if isinstance(v, list):            # assignments: one ragged list per batch, stored end to end
                out[f'{name}/{f}'] = np.concatenate([_host(a) for a in v]) if v else np.zeros(0, np.int32)
            else:
                out[f'{name}/{f}'] = _host(v)

    icp_fields = ('T', 'iters', 'inliers', 'rmse', 'status', 'assign', 'stats')

    def both_methods(name, cases, d, radius, max_iter, stats=True):
        """cases [(target, source, T0)] as one batch of the point method and one of the plane method (normals on the target's grid)"""
        point = [(grid(q, d), grid(p, d), dev(T0)) for q, p, T0 in cases]
        put(f'{name}/point', hip.icp_batch(point, d, max_iter=max_iter, want_assign=True, want_stats=stats), icp_fields)
        normals = {}
        for g, _, _ in point:
            if id(g) not in normals:
                normals[id(g)] = hip.icp_normals(g, radius)
        plane = [(g, s, normals[id(g)], T0) for g, s, T0 in point]
        put(f'{name}/plane', hip.icp_plane_batch(plane, d, max_iter=max_iter, want_assign=True, want_stats=stats), icp_fields)

    chunk = [(q, p, T0) for _, q, p, T0 in C.chunk_pairs()]
    both_methods('chunk', chunk, C.CHUNK_DIST, PC.CHUNK_RADIUS, C.CHUNK_ITER)
    both_methods('chunk_reversed', chunk[::-1], C.CHUNK_DIST, PC.CHUNK_RADIUS, C.CHUNK_ITER)

    solve = [(hip.IcpGrid(torch.from_numpy(c['Q']).cuda(), C.SOLVE_DIST, box=np.stack([c['Q'].min(0), c['Q'].max(0)]).astype(np.float64)),
              hip.IcpGrid(torch.from_numpy(c['P']).cuda(), C.SOLVE_DIST, box=np.stack([c['P'].min(0), c['P'].max(0)]).astype(np.float64)), dev(c['T0']))
             for c in C.solve_family()[0]]
    put('solve/point', hip.icp_batch(solve, C.SOLVE_DIST, max_iter=1, want_stats=True), icp_fields[:5] + ('stats',))

    walls = [C.wall_pair(seed) for seed in C.WALL_SEEDS]
    both_methods('wall', [(q, p, T0) for q, p, _, T0 in walls], C.WALL_DIST, PC.RANK_RADIUS, C.WALL_ITER)
    for n in PC.RANK_PLANES:                   # (one batch each, as the rank test runs them)
        tgt, src, _, T0 = PC.planes_pair(n)
        both_methods(f'planes{n}', [(tgt, src, T0)], PC.RANK_DIST, PC.RANK_RADIUS, PC.RANK_ITER)

    _, q, p, T0 = C.chunk_pairs()[C.CHUNK_SRC_N.index(1025)]
    Tn = T0.copy(); Tn[1, 2] = np.nan
    # (no statistics: a pair that never iterates leaves its row of them unwritten)
    both_methods('degenerate', [(q, p, Tn), (q, p[:0], T0), (q, p, T0)], C.CHUNK_DIST, PC.CHUNK_RADIUS, C.CHUNK_ITER, stats=False)

    ev = [(grid(q, C.CHUNK_DIST), grid(p, C.CHUNK_DIST), dev(T0)) for q, p, T0 in chunk]
    put('eval', hip.icp_eval_batch(ev, C.CHUNK_DIST, want_assign=True), ('stats', 'info', 'status', 'assign01', 'assign10'))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=FIXTURE)
    a = ap.parse_args()
    git = lambda *args: subprocess.run(('git', '-C', ROOT) + args, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    commit = git('rev-parse', 'HEAD').stdout.strip()
    if len(commit) != 40 or git('diff', '--quiet', 'HEAD', '--', 'roreg_amd/csrc', 'include').returncode != 0:
        sys.exit('record_icp_bits: not a git checkout, or roreg_amd/csrc or include differ from HEAD -- the fixture is recorded from committed kernels only')
    arrays = run_cases()
    np.savez_compressed(a.out, commit=np.array(commit), **arrays)
    print(f'{a.out}: {len(arrays)} arrays, {sum(v.nbytes for v in arrays.values())} bytes before compression, {os.path.getsize(a.out)} bytes; commit {commit}')


if __name__ == '__main__':
    main()
