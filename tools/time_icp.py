"""Time the dense ICP refinement (RegistrationEngine.icp_many) on a scene-like batch, on the GPU, against the same inputs through a
scipy k-d tree ICP on the host.

    python tools/time_icp.py [--pairs 60] [--clouds 20] [--sizes 50000,300000] [--max_dist 0.07] [--max_iter 30] [--reps 5]
                             [--method point|plane|gicp|point,plane,gicp] [--loss none,huber,tukey [--loss_scale 0.03]] [--normal_radius 0.14]
                             [--host_pairs 3] [--voxel 0.025,0.05]
                             [--eval] [--out profiles/icp_timing.txt]

The batch: `clouds` dense clouds of one synthetic room (roreg_amd.synth.make_dense_pair views under seeded poses), `pairs` pairs among
them with start transforms 3 degrees / 5 cm off the ground truth.  How many points a real 3DMatch fragment has is not known here, so two
sizes are timed.  Device times are stream events around icp_many (grids built beforehand, and once more inside a timed window of their
own); the search kernel's share comes from the library's event brackets (hip.profile_read('icp_search')) in a separate pass.  The host
figure runs the first `host_pairs` pairs through cKDTree.query(workers=16) + the same update and is scaled per pair (point method only, and
only where scipy is installed).  --method plane times the point-to-plane form on the same batch: the one-time normal estimation per cloud in a
window of its own, the shares of the search and of the plane pass from their brackets (the rest is the solve, the first launches and the
gaps between launches), and every method's distance from the ground truth.  --method gicp times the plane-to-plane form
likewise (its pass is read from the same bracket, 'icp_plane'; its normals window covers every cloud, and every cloud is a source somewhere).  --voxel 0.025,0.05 adds, in the same job and per voxel size: the
voxel-grid downsampling's call time per cloud (hip.voxel_downsample, host clock around the call and a device synchronise: the call reads
(m, flags) back), m / n, the numpy oracle's time for one such cloud on the host, and every method's icp_many on the clouds downsampled at
attach_points -- ms per pair, iterations, distance from the ground truth -- beside the full-cloud figures above it.  --eval adds the
read-only pair evaluation (RegistrationEngine.evaluate_many: both directions, overlap, RMSE, information matrix) on the same batch under its
start transforms, beside the nearest thing the iteration offers: two icp_many(max_iter=1) calls, one forward and one with the clouds swapped
under the inverse transforms; the two are timed alternately, --reps times each.  --loss none,huber,tukey times the plane and gicp methods once per
entry of the list on the same batch (none: the unweighted entries; a loss: the weighted kernels at --loss_scale), each with its own bracket
shares and distance from the ground truth."""
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


def ground_truth(n_clouds, n_pairs, n, seed=0):
    """The ground-truth transform of every pair of make_batch, in its order."""
    from roreg_amd import synth
    poses = []
    for k in range(0, n_clouds, 2):
        poses += [np.eye(4), synth.dense_gt()]
    out = []
    for q in range(n_pairs):
        k = 2 * (q % (n_clouds // 2))
        a, b = (k, k + 1) if (q // (n_clouds // 2)) % 2 == 0 else (k + 1, k)
        out.append(np.linalg.inv(poses[a]) @ poses[b])
    return out


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
    ap.add_argument('--method', default='point', help="'point', 'plane', 'gicp' or a comma list of them: every method is timed on the same batch")
    ap.add_argument('--loss', default='none', help="plane and gicp methods: a comma list of 'none' and robust losses (huber, cauchy, gm, tukey), each timed in turn")
    ap.add_argument('--loss_scale', type=float, default=0.03, help='the scale of every loss of --loss, in metres')
    ap.add_argument('--normal_radius', type=float, default=None, help='plane and gicp methods: radius of the normal estimation (default 2 max_dist)')
    ap.add_argument('--voxel', default='', help="voxel sizes, e.g. '0.025,0.05': downsampling time per cloud and the ICP on the downsampled clouds")
    ap.add_argument('--eval', action='store_true', help='time evaluate_many beside two icp_many(max_iter=1) calls (forward, and swapped under the inverse)')
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
    import _icp_oracle as O
    methods = a.method.split(',')
    assert all(m in ('point', 'plane', 'gicp') for m in methods), a.method
    losses = [None if v == 'none' else v for v in a.loss.split(',')]
    assert all(v is None or v in hip.ICP_LOSSES for v in losses), a.loss
    runs = [(m, v) for m in methods for v in (losses if m in ('plane', 'gicp') else [None])]          # (the point method has no loss)
    radius = 2.0 * a.max_dist if a.normal_radius is None else a.normal_radius
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for n in [int(v) for v in a.sizes.split(',')]:
        clouds, pairs = make_batch(a.clouds, a.pairs, n)
        gts = ground_truth(a.clouds, a.pairs, n)
        states = [eng.attach_points(CloudState(before=None), c) for c in clouds]
        T0 = hip.upload(np.stack([T for _, _, T in pairs]))
        items = [(states[i], states[j], T0[q]) for q, (i, j, _) in enumerate(pairs)]
        eng.icp_many(items, a.max_dist, a.max_iter)                         # warm-up: code objects, grids, allocator
        torch.cuda.synchronize()
        t_build = []
        for _ in range(a.reps):                                             # grid builds on their own (once per cloud and radius in a scene)
            e0, e1 = ev(), ev()
            e0.record()
            for s in states:
                hip.IcpGrid(s.points, a.max_dist, box=s.points_box)
            e1.record(); torch.cuda.synchronize()
            t_build.append(e0.elapsed_time(e1))
        lines += [f'\n{n} points per cloud',
                  f'  grid build, {a.clouds} clouds          : median {np.median(t_build):.3f} ms (min {min(t_build):.3f}, max {max(t_build):.3f}) = {np.median(t_build) / a.clouds:.3f} ms per cloud']
        for method, loss in runs:
            kw = dict(method=method, normal_radius=radius) if method in ('plane', 'gicp') else {}
            if loss is not None:
                kw.update(loss=loss, loss_scale=a.loss_scale)
            run = lambda: eng.icp_many(items, a.max_dist, a.max_iter, **kw)
            out = run()                                                     # warm-up of this method (plane, gicp: the normals are cached from here on)
            torch.cuda.synchronize()
            lines += [f'  method {method}' + (f' (normal radius {radius}, min_neighbors 6)' if method in ('plane', 'gicp') else '')
                      + (f', loss {loss} at scale {a.loss_scale}' if loss is not None else '')]
            if method in ('plane', 'gicp') and loss == losses[0]:           # (once per method: the normals do not depend on the loss)                                 # (every cloud of the batch is a target and a source: both sides' tables are in this window)
                t_nrm = []
                for _ in range(a.reps):                                     # the normal estimation on its own (once per cloud and radius in a scene)
                    e0, e1 = ev(), ev()
                    e0.record()
                    for s in states:
                        hip.icp_normals(eng.icp_grid(s, a.max_dist), radius, 6)
                    e1.record(); torch.cuda.synchronize()
                    t_nrm.append(e0.elapsed_time(e1))
                valid = float(np.mean([float((eng.icp_normals(s, a.max_dist, radius)[:, :3] != 0).any(1).double().mean()) for s in states]))
                lines += [f'    normals, {a.clouds} clouds           : median {np.median(t_nrm):.3f} ms (min {min(t_nrm):.3f}, max {max(t_nrm):.3f}) = '
                          f'{np.median(t_nrm) / a.clouds:.3f} ms per cloud; {100 * valid:.2f} % of the points get a normal']
            t_run = []
            for _ in range(a.reps):
                e0, e1 = ev(), ev()
                e0.record()
                out = run()
                e1.record(); torch.cuda.synchronize()
                t_run.append(e0.elapsed_time(e1))
            iters = out[1].cpu().numpy(); inl = out[2].cpu().numpy(); status = out[4].cpu().numpy()
            slots = ('icp_search', 'icp_plane') if method in ('plane', 'gicp') else ('icp_search',)      # ('icp_plane': the second pass of either normal-based method)
            hip.profile_enable(True)                                        # a pass of its own: the brackets add events to the stream
            run()
            torch.cuda.synchronize()
            before = {k: hip.profile_read(k) for k in slots}
            e0, e1 = ev(), ev()
            e0.record(); run(); e1.record(); torch.cuda.synchronize()
            ms_prof = e0.elapsed_time(e1)
            share = {k: (hip.profile_read(k)[0] - before[k][0], hip.profile_read(k)[1] - before[k][1]) for k in slots}
            hip.profile_enable(False)
            med = float(np.median(t_run))
            queries = float((iters.astype(np.int64) * n).sum())
            Tdev = out[0].cpu().numpy()
            err = np.array([O.pose_error(Tdev[q], gts[q]) for q in range(len(pairs))])
            lines += [f'    icp_many, {a.pairs} pairs           : median {med:.3f} ms (min {min(t_run):.3f}, max {max(t_run):.3f}) over {a.reps} runs = {med / a.pairs:.4f} ms per pair',
                      f'    iterations run                : mean {iters.mean():.1f}, min {iters.min()}, max {iters.max()}; inliers mean {inl.mean():.0f}; '
                      f'status counts {np.bincount(status, minlength=4).tolist()} {list(hip.ICP_STATUS)}',
                      f'    from the ground truth         : rotation median {np.median(err[:, 0]):.4f} deg (max {err[:, 0].max():.4f}), translation median '
                      f'{np.median(err[:, 1]) * 1e3:.3f} mm (max {err[:, 1].max() * 1e3:.3f})',
                      f'    point queries                 : {queries:.3e} per run = {queries / (med * 1e-3):.3e} per second']
            rest = ms_prof
            for k in slots:
                rest -= share[k][0]
                lines += [f'    {k + " share":<30}: {share[k][0]:.3f} ms in {share[k][1]} launches of a {ms_prof:.3f} ms run with the brackets on = {100 * share[k][0] / ms_prof:.1f} %']
            lines += [f'    solve, first launches and gaps: {rest:.3f} ms = {100 * rest / ms_prof:.1f} %']
            if method == 'point' and a.host_pairs > 0:
                try:
                    import scipy.spatial                                    # noqa: F401
                except ImportError:
                    lines += ['    host, cKDTree ICP             : scipy is not installed here']
                    continue
                t0 = time.perf_counter()
                hres = [host_icp(clouds[i], clouds[j], T, a.max_dist, a.max_iter, a.workers) for i, j, T in pairs[:a.host_pairs]]
                host_ms = (time.perf_counter() - t0) * 1e3 / max(a.host_pairs, 1)
                diff = max(float(np.abs(Tdev[q] - r.T).max()) for q, r in enumerate(hres)) if hres else float('nan')
                lines += [f'    host, cKDTree(workers={a.workers}) ICP: {host_ms:.1f} ms per pair (mean of the first {a.host_pairs} pairs, tree build included; iterations '
                          f'{[r.iters for r in hres]}); max |T_device - T_host| = {diff:.2e}',
                          f'    host / device per pair        : {host_ms / (med / a.pairs):.0f} x']
        if a.eval:
            Tinv = hip.upload(np.stack([np.linalg.inv(T) for _, _, T in pairs]))
            swapped = [(states[j], states[i], Tinv[q]) for q, (i, j, _) in enumerate(pairs)]
            run_eval = lambda: eng.evaluate_many(items, a.max_dist)
            run_icp1 = lambda: (eng.icp_many(items, a.max_dist, 1), eng.icp_many(swapped, a.max_dist, 1))
            st = run_eval()[0]; one = run_icp1()                            # warm-up
            torch.cuda.synchronize()
            same = bool(torch.equal(st[:, 0].to(torch.int32), one[0][2]))
            t_eval, t_icp1 = [], []
            for _ in range(a.reps):                                         # alternately: both see the same clocks and cache state
                for run, acc in ((run_eval, t_eval), (run_icp1, t_icp1)):
                    e0, e1 = ev(), ev()
                    e0.record(); run(); e1.record(); torch.cuda.synchronize()
                    acc.append(e0.elapsed_time(e1))
            me, mi = float(np.median(t_eval)), float(np.median(t_icp1))
            lines += [f'  pair evaluation (both directions, 11 sums, information matrix), {a.pairs} pairs, alternating, {a.reps} runs each',
                      f'    evaluate_many                 : median {me:.3f} ms (min {min(t_eval):.3f}, max {max(t_eval):.3f}) = {me / a.pairs:.4f} ms per pair; '
                      f'overlap1 mean {float(st[:, 3].mean()):.3f}; n01 equals the forward icp_many inliers: {same}',
                      f'    2 x icp_many(max_iter=1)      : median {mi:.3f} ms (min {min(t_icp1):.3f}, max {max(t_icp1):.3f}) = {mi / a.pairs:.4f} ms per pair',
                      f'    evaluate_many / the two calls : {me / mi:.3f}']
        for v in [float(x) for x in a.voxel.split(',') if x]:
            import _voxel_oracle as VO
            for s_ in states:                                               # warm-up: code object, allocator
                hip.voxel_downsample(s_.points, v)
            torch.cuda.synchronize()
            t_vox = []
            for _ in range(max(a.reps, 5)):
                t0 = time.perf_counter()
                ms = [int(hip.voxel_downsample(s_.points, v).first.shape[0]) for s_ in states]
                torch.cuda.synchronize()
                t_vox.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            VO.downsample(clouds[0], v)
            t_np = (time.perf_counter() - t0) * 1e3
            lines += [f'  voxel {v}',
                      f'    downsample, {a.clouds} clouds        : median {np.median(t_vox):.3f} ms (min {min(t_vox):.3f}, max {max(t_vox):.3f}) over {len(t_vox)} runs = '
                      f'{np.median(t_vox) / a.clouds:.3f} ms per cloud (call time with a synchronise); m / n = {np.mean(ms) / n:.4f} (m mean {np.mean(ms):.0f})',
                      f'    numpy oracle on the host      : {t_np:.1f} ms for one cloud (np.unique + np.add.at, one thread)']
            vstates = [eng.attach_points(CloudState(before=None), c, voxel=v) for c in clouds]
            vitems = [(vstates[i], vstates[j], T0[q]) for q, (i, j, _) in enumerate(pairs)]
            for method in methods:
                kw = dict(method=method, normal_radius=radius) if method in ('plane', 'gicp') else {}
                run = lambda: eng.icp_many(vitems, a.max_dist, a.max_iter, **kw)
                out = run()                                                 # warm-up: grids (and normals) of the downsampled clouds
                torch.cuda.synchronize()
                t_run = []
                for _ in range(a.reps):
                    e0, e1 = ev(), ev()
                    e0.record()
                    out = run()
                    e1.record(); torch.cuda.synchronize()
                    t_run.append(e0.elapsed_time(e1))
                iters = out[1].cpu().numpy(); inl = out[2].cpu().numpy(); status = out[4].cpu().numpy()
                Tdev = out[0].cpu().numpy()
                err = np.array([O.pose_error(Tdev[q], gts[q]) for q in range(len(pairs))])
                med = float(np.median(t_run))
                lines += [f'    method {method}, icp_many on the downsampled clouds: median {med:.3f} ms (min {min(t_run):.3f}, max {max(t_run):.3f}) over {a.reps} runs = '
                          f'{med / a.pairs:.4f} ms per pair; iterations mean {iters.mean():.1f}, min {iters.min()}, max {iters.max()}; inliers mean {inl.mean():.0f}; '
                          f'status counts {np.bincount(status, minlength=4).tolist()}',
                          f'      from the ground truth       : rotation median {np.median(err[:, 0]):.4f} deg (max {err[:, 0].max():.4f}), translation median '
                          f'{np.median(err[:, 1]) * 1e3:.3f} mm (max {err[:, 1].max() * 1e3:.3f})']
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
