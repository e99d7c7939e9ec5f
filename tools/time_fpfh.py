"""Time the FPFH stages (csrc/fpfh.hip) on one dense cloud, on the GPU.

    python tools/time_fpfh.py [--n 300000] [--voxel 0.025] [--normal_radius 0.05] [--radius 0.125] [--reps 20] [--out profiles/fpfh_timing.txt]

The cloud: view 0 of roreg_amd.synth.make_dense_pair(0, n) downsampled at `voxel` on the device; its pair for the two nearest-neighbour
searches is view 1 treated alike.  Device times are stream events around each binding call (the permutation / scaling passes and the
workspace allocation of a call are inside its window), after two warm-up rounds, `reps` rounds with the stages in turn; the figure is the
median, the spread is min .. max.  hip.icp_normals on the same grid at the FPFH radius is the yardstick: a kernel that walks the same balls
(twice).  No parent and no reference to race: nothing here is a bar."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=300000)
    ap.add_argument('--voxel', type=float, default=0.025)
    ap.add_argument('--normal_radius', type=float, default=0.05)
    ap.add_argument('--radius', type=float, default=0.125)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fpfh_timing.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_fpfh.py needs the GPU: there is no host fallback'
    from roreg_amd import fpfh, hip, icp, synth, voxel
    p0, p1, _ = synth.make_dense_pair(0, n=args.n)
    clouds = [voxel.device_downsample(icp.device_points(p), args.voxel)[0] for p in (p0, p1)]
    pts = clouds[0]
    grid = hip.IcpGrid(pts, args.radius)
    table = hip.icp_normals(grid, args.normal_radius)
    c = pts.double().mean(0).cpu().numpy()
    descs = [fpfh.describe(p, args.radius, normal_radius=args.normal_radius) for p in clouds]
    rows = [d.valid.nonzero().reshape(-1).contiguous() for d in descs]
    stages = {
        'icp_normals (radius %g: the yardstick)' % args.radius: lambda s: hip.icp_normals(grid, args.radius),
        'icp_normals (radius %g: the normals used)' % args.normal_radius: lambda s: hip.icp_normals(grid, args.normal_radius),
        'fpfh_orient': lambda s: s.__setitem__('o', hip.fpfh_orient(grid, table, c)),
        'fpfh_spfh': lambda s: s.__setitem__('cm', hip.fpfh_spfh(grid, s['o'], args.radius)),
        'fpfh_features': lambda s: s.__setitem__('f', hip.fpfh_features(grid, s['cm'][0], s['cm'][1], args.radius)),
        'nn_search 0 -> 1 (F = 33: the generic kernel)': lambda s: hip.nn_search(descs[0].features, descs[1].features, src_rows=rows[0], tgt_rows=rows[1]),
        'nn_search 1 -> 0': lambda s: hip.nn_search(descs[1].features, descs[0].features, src_rows=rows[1], tgt_rows=rows[0]),
    }
    state, times = {}, {k: [] for k in stages}
    for rep in range(args.reps + 2):
        for name, fn in stages.items():
            ms, _ = timed(lambda: fn(state))
            if rep >= 2:
                times[name].append(ms)
    m = state['cm'][1]
    lines = [f'# {torch.cuda.get_device_name(0)}; synth.make_dense_pair(0, n={args.n}) view 0 at voxel {args.voxel}: {pts.shape[0]} points '
             f'(view 1: {clouds[1].shape[0]}), grid cell edge {grid.edge:g}, dims {grid.dims}',
             f'# normal radius {args.normal_radius}, FPFH radius {args.radius}; pairs counted per point: mean {float(m.float().mean()):.1f}, max {int(m.max())}; '
             f'valid rows {int(descs[0].valid.sum())} / {int(descs[1].valid.sum())}',
             f'# device events around each call, 2 warm-up rounds, {args.reps} rounds: median (min .. max) ms', '']
    for name, t in times.items():
        lines.append(f'{name:<52s} {np.median(t):9.3f}   ({min(t):.3f} .. {max(t):.3f})')
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
