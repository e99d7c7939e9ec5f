"""Timing of the grid k-nearest-neighbour kernel and what is built on it (csrc/grid_knn.hip) on one cloud of
synth.make_dense_pair(0, n=300000), whole and voxel-downsampled at 0.025: device events around each call, 2 warm-up rounds, the median of 10.

    python tools/time_knn.py [--out profiles/grid_knn_timing.txt] [--n 300000] [--voxel 0.025]

Timed: hip.grid_knn at k 8 / 16 / 32 and radius 0.05 / 0.125 (the grid is built for the radius, outside the timing; the fraction of rows whose ball
holds at least k and the mean ball are printed beside it), neighbors.knn(radius=None) with its rounds, outliers.statistical(nb_neighbors=16) end to end.
Yardsticks, in the same process: hip.icp_normals on the same grid and radius (it walks the same balls twice: the floor the candidate traffic
sets) and hip.knn_search(points, points, k), the brute-force scan that was the only k-NN before (3 repetitions: it is slow), with its workspace."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from roreg_amd import hip, neighbors, outliers, synth, voxel          # noqa: E402

KS, RADII = (8, 16, 32), (0.05, 0.125)


def timed(fn, warm=2, reps=10):
    """median milliseconds between device events around fn()"""
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def run(name, pts, say, brute):
    n = int(pts.shape[0])
    say(f'\n== {name}: {n} points')
    say(f'{"call":<44}{"ms":>10}{"x normals":>11}   notes')
    for r in RADII:
        grid = hip.IcpGrid(pts, r)
        t_n = timed(lambda: hip.icp_normals(grid, r))
        say(f'{f"icp_normals r={r}":<44}{t_n:>10.3f}{1.0:>11.2f}   the same grid, the same balls, two walks')
        for k in KS:
            t = timed(lambda: hip.grid_knn(grid, k, r, want_mean=True))
            count = hip.grid_knn(grid, k, r)[2]
            say(f'{f"grid_knn k={k} r={r}":<44}{t:>10.3f}{t / t_n:>11.2f}   mean ball {float(count.double().mean()):.1f}, '
                f'{100.0 * float((count >= k).double().mean()):.1f} % of the rows hold k')
    info = {}
    t = timed(lambda: neighbors.device_knn(pts, 16, info=info))
    say(f'{"neighbors.knn k=16 radius=None":<44}{t:>10.3f}{"":>11}   {info["rounds"]} rounds at radii {[round(v, 4) for v in info["radii"]]}')
    t = timed(lambda: outliers.device_statistical(pts, 16, 2.0))
    kept = int(outliers.device_statistical(pts, 16, 2.0).mask.sum())
    say(f'{"outliers.statistical nb_neighbors=16":<44}{t:>10.3f}{"":>11}   end to end (grids, rounds, threshold, compaction); keeps {kept} of {n}')
    if brute:
        for k in (8, 16):
            ws = hip.lib().roreg_knn_search_workspace(n, n)
            t = timed(lambda: hip.knn_search(pts, pts, k), warm=1, reps=3)
            say(f'{f"knn_search k={k} (brute force, {n} x {n})":<44}{t:>10.3f}{"":>11}   workspace {ws / 2 ** 20:.1f} MiB; float32 distances, the row itself listed')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=300000)
    ap.add_argument('--voxel', type=float, default=0.025)
    ap.add_argument('--brute_whole', action='store_true', help='also time the brute-force scan on the whole cloud (about five times the work of the downsampled one)')
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/time_knn.py on {torch.cuda.get_device_name(0)}: synth.make_dense_pair(0, n={a.n})[0]; device events, 2 warm-up rounds, median of 10')
    pts = torch.from_numpy(np.ascontiguousarray(synth.make_dense_pair(0, n=a.n)[0], np.float32)).cuda()
    down = voxel.device_downsample(pts, a.voxel)[0]
    run(f'voxel {a.voxel}', down, say, True)
    run('whole cloud', pts, say, a.brute_whole)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
