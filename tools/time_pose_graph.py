"""Time the pose-graph optimiser (csrc/pose_graph.hip, v6h) at the benchmark's shape: 8 graphs of 37-66 nodes and about 200 edges each, one
call for all of them.  Per run: the call's time between stream events, the rounds each graph ran, and the solve launches' share of it (the
library's event brackets, slot 'pg_solve', taken in a run of their own so that they do not sit inside the timed call); beside those the
numpy oracle's time on the same graphs (tests/_pose_graph_oracle.py, one graph after the other on the host).

    python tools/time_pose_graph.py --out profiles/pose_graph_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

NODES = (37, 41, 46, 50, 54, 58, 62, 66)          # 433 clouds in 8 scenes: the benchmark's scene sizes run from 37 to 66


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--edges', type=int, default=200)
    ap.add_argument('--tau', type=float, default=None)
    ap.add_argument('--max_iter', type=int, default=100)
    ap.add_argument('--no_oracle', action='store_true')
    a = ap.parse_args()
    import torch
    import _pose_graph_cases as K
    import _pose_graph_oracle as O
    from roreg_amd import hip
    graphs = [K.ring_graph(500 + C, C, a.edges) for C in NODES]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()
    batch = [hip.PgGraph(g['C'], g['edges'], dev(g['T']), dev(g['Lam']), None, 0, a.tau) for g in graphs]
    lines = [f'pose-graph optimisation, {len(graphs)} graphs in one call: nodes {list(NODES)}, {a.edges} edges each, tau {a.tau}, max_iter {a.max_iter}',
             f'device: {torch.cuda.get_device_name(0)}']
    hip.pg_optimize_batch(batch, a.max_iter)                      # warm-up: module load, staging ring
    torch.cuda.synchronize()
    times = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = hip.pg_optimize_batch(batch, a.max_iter)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    iters, status = r.iters.cpu().numpy(), r.status.cpu().numpy()
    lines.append(f'call time between stream events over {a.runs} runs: median {np.median(times):.3f} ms (min {min(times):.3f}, max {max(times):.3f}); '
                 f'{3 * a.max_iter + 2} launches enqueued per call')
    lines.append(f'rounds run per graph: {iters.tolist()}, status {[hip.PG_STATUS[s] for s in status]}')
    hip.profile_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hip.pg_optimize_batch(batch, a.max_iter)
    e1.record()
    torch.cuda.synchronize()
    ms, n = hip.profile_read('pg_solve')
    hip.profile_enable(False)
    lines.append(f'solve launches in a bracketed run: {ms:.3f} ms in {n} launches of a {e0.elapsed_time(e1):.3f} ms call = {ms / e0.elapsed_time(e1):.2f} of it '
                 f'(the launches after the last graph has finished return at once and are counted)')
    if not a.no_oracle:
        t0 = time.perf_counter()
        refs = [O.Graph(g['C'], g['edges'], g['T'], g['Lam'], tau=a.tau).optimize(max_iter=a.max_iter) for g in graphs]
        t1 = time.perf_counter()
        poses = r.poses.cpu().numpy()
        worst = max(np.abs(poses[r.node0[b]:r.node0[b] + g['C']] - ref['poses']).max() for b, (g, ref) in enumerate(zip(graphs, refs)))
        lines.append(f'numpy oracle on the host, the same graphs one after the other: {(t1 - t0) * 1e3:.0f} ms, rounds {[ref["iters"] for ref in refs]}; '
                     f'max |pose - oracle| {worst:.2e}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
