"""Time the dense ICP refinement (RegistrationEngine.icp_many) on a scene-like batch, on the GPU, against the same inputs through a
scipy k-d tree ICP on the host.

    python tools/time_icp.py [--pairs 60] [--clouds 20] [--sizes 50000,300000] [--max_dist 0.07] [--max_iter 30] [--reps 5]
                             [--host_pairs 3] [--out profiles/icp_timing.txt]

The batch: `clouds` dense clouds of one synthetic room (roreg_amd.synth.make_dense_pair views under seeded poses), `pairs` pairs among
them with start transforms 3 degrees / 5 cm off the ground truth.  How many points a real 3DMatch fragment has is not known here, so two
sizes are timed.  Device times are stream events around icp_many (grids built beforehand, and once more inside a timed window of their
own); the search kernel's share comes from the library's event brackets (hip.profile_read('icp_search')) in a separate pass.  The host
figure runs the first `host_pairs` pairs through cKDTree.query(workers=16) + the same update and is scaled per pair."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_batch(n_clouds, n_pairs, n, seed=0):
    """-> (clouds [float32 [n,3]], pairs [(i, j, T0)]): view k of one room is views[k % 2] of make_dense_pair(seed + k // 2) moved by a seeded pose."""
    import _icp_oracle as O
    from roreg_amd import synth
    rng = np.random.default_rng(seed)
    clouds, poses = [], []
    for k in range(0, n_clouds, 2):
        p0, p1, Tg = synth.make_dense_pair(seed + k, n)
        clouds += [p0, p1]
        poses += [np.eye(4), Tg]                         # world <- cloud
    pairs = []
    for q in range(n_pairs):
        k = 2 * (q % (n_clouds // 2))
        a, b = (k, k + 1) if (q // (n_clouds // 2)) % 2 == 0 else (k + 1, k)
        Tg = np.linalg.inv(poses[a]) @ poses[b]
        pairs.append((a, b, O.perturb(Tg, 3.0, 0.05, int(rng.integers(1 << 30)))))
    return clouds[:n_clouds], pairs


def host_icp(p0, p1, T0, d, max_iter, workers):
    import _icp_oracle as O
    from scipy.spatial import cKDTree
    Q = p0.astype(np.float64)
    tree = cKDTree(Q)

    def nn(Q_, Pt, d_):
        dist, idx = tree.query(Pt, k=1, distance_upper_bound=d_, workers=workers)
        ok = idx < Q.shape[0]
        return np.where(ok, idx, -1).astype(np.int32), np.where(ok, dist * dist, np.inf)
    return O.icp(p0, p1, T0, d, max_iter=max_iter, nn=nn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=60)
    ap.add_argument('--clouds', type=int, default=20)
    ap.add_argument('--sizes', default='50000,300000')
    ap.add_argument('--max_dist', type=float, default=0.07)
    ap.add_argument('--max_iter', type=int, default=30)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host_pairs', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'time_icp.py measures on the GPU; there is no host fallback'
    from roreg_amd import hip
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    eng = RegistrationEngine(default_config(), None, None)
    lines = [f'dense ICP timing: {a.pairs} pairs among {a.clouds} clouds, max_dist {a.max_dist}, max_iter {a.max_iter}, starts 3 degrees / 5 cm off; '
             f'device {torch.cuda.get_device_name(0)}',
             'the point count of a real 3DMatch fragment is not known on this machine: two sizes']
    for n in [int(v) for v in a.sizes.split(',')]:
        clouds, pairs = make_batch(a.clouds, a.pairs, n)
        states = [eng.attach_points(CloudState(before=None), c) for c in clouds]
        T0 = hip.upload(np.stack([T for _, _, T in pairs]))
        items = [(states[i], states[j], T0[q]) for q, (i, j, _) in enumerate(pairs)]
        ev = lambda: torch.cuda.Event(enable_timing=True)
        out = eng.icp_many(items, a.max_dist, a.max_iter)                   # warm-up: code objects, grids, allocator
        torch.cuda.synchronize()
        t_build = []
        for _ in range(a.reps):                                             # grid builds on their own (once per cloud and radius in a scene)
            e0, e1 = ev(), ev()
            e0.record()
            for s in states:
                hip.IcpGrid(s.points, a.max_dist, box=s.points_box)
            e1.record(); torch.cuda.synchronize()
            t_build.append(e0.elapsed_time(e1))
        t_run = []
        for _ in range(a.reps):
            e0, e1 = ev(), ev()
            e0.record()
            out = eng.icp_many(items, a.max_dist, a.max_iter)
            e1.record(); torch.cuda.synchronize()
            t_run.append(e0.elapsed_time(e1))
        iters = out[1].cpu().numpy(); inl = out[2].cpu().numpy(); status = out[4].cpu().numpy()
        hip.profile_enable(True)                                            # a pass of its own: the brackets add events to the stream
        eng.icp_many(items, a.max_dist, a.max_iter)
        torch.cuda.synchronize()
        ms_search, n_br = hip.profile_read('icp_search')
        e0, e1 = ev(), ev()
        e0.record(); eng.icp_many(items, a.max_dist, a.max_iter); e1.record(); torch.cuda.synchronize()
        ms_prof = e0.elapsed_time(e1)
        ms_search, n_br = hip.profile_read('icp_search')[0] - ms_search, hip.profile_read('icp_search')[1] - n_br
        hip.profile_enable(False)
        med = float(np.median(t_run))
        queries = float((iters.astype(np.int64) * n).sum())
        lines += [f'\n{n} points per cloud',
                  f'  grid build, {a.clouds} clouds          : median {np.median(t_build):.3f} ms (min {min(t_build):.3f}, max {max(t_build):.3f}) = {np.median(t_build) / a.clouds:.3f} ms per cloud',
                  f'  icp_many, {a.pairs} pairs             : median {med:.3f} ms (min {min(t_run):.3f}, max {max(t_run):.3f}) over {a.reps} runs = {med / a.pairs:.4f} ms per pair',
                  f'  iterations run                  : mean {iters.mean():.1f}, min {iters.min()}, max {iters.max()}; inliers mean {inl.mean():.0f}; '
                  f'status counts {np.bincount(status, minlength=4).tolist()} {list(hip.ICP_STATUS)}',
                  f'  point queries                   : {queries:.3e} per run = {queries / (med * 1e-3):.3e} per second',
                  f'  search kernel share             : {ms_search:.3f} ms in {n_br} launches of a {ms_prof:.3f} ms run with the brackets on = {100 * ms_search / ms_prof:.1f} %']
        t0 = time.perf_counter()
        hres = [host_icp(clouds[i], clouds[j], T, a.max_dist, a.max_iter, a.workers) for i, j, T in pairs[:a.host_pairs]]
        host_ms = (time.perf_counter() - t0) * 1e3 / max(a.host_pairs, 1)
        Tdev = out[0].cpu().numpy()
        diff = max(float(np.abs(Tdev[q] - r.T).max()) for q, r in enumerate(hres)) if hres else float('nan')
        lines += [f'  host, cKDTree(workers={a.workers}) ICP  : {host_ms:.1f} ms per pair (mean of the first {a.host_pairs} pairs, tree build included; iterations '
                  f'{[r.iters for r in hres]}); max |T_device - T_host| = {diff:.2e}',
                  f'  host / device per pair          : {host_ms / (med / a.pairs):.0f} x']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
