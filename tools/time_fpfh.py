"""Time the FPFH stages (csrc/fpfh.hip) on one dense cloud, on the GPU.

    python tools/time_fpfh.py [--n 300000] [--voxel 0.025] [--normal_radius 0.05] [--radius 0.125] [--reps 20] [--out profiles/fpfh_timing.txt]
    python tools/time_fpfh.py --match [--reps 10] [--out profiles/fpfh_match_timing.txt]       # the matcher alone: see match_section

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


def match_section(args):
    """fpfh.match(method='scan') against method='mfma' (csrc/fpfh_match.hip) on the dense pair's descriptors and on the 6,000-row pair of the tests
    (tests/_fpfh_cases.py terrain pair 0 at voxel 0.05): after one warm-up call of each, the two alternate `reps` times on the same process and
    device; device events around each call (row selection, launches, the count's read-back and the cut are inside the window, alike for both);
    median (min .. max).  Then pass A / pass B of one call from the library's event slots, the candidate counts of a 512 x 512 sub-block, and a
    sweep over the side length (the first L valid rows of both sides, median of 3) for the crossover fpfh.match(method='auto') uses."""
    from roreg_amd import fpfh, hip, synth
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _fpfh_cases as K
    lines = [f'# {torch.cuda.get_device_name(0)}; fpfh.match(d0, d1, method=...), device events around each call, 1 warm-up, {args.reps} alternating rounds: '
             f'median (min .. max) ms', '']

    def race(d0, d1, reps):
        t = {'scan': [], 'mfma': []}
        for rep in range(reps + 1):
            for method in t:
                ms, m = timed(lambda: fpfh.match(d0, d1, method=method))
                if rep:
                    t[method].append(ms)
        return t, int(m.shape[0])

    def first_rows(d, L):
        keep = d.valid.bool() & (torch.cumsum(d.valid.long(), 0) <= L)
        return fpfh.FpfhCloud(d.points, d.normals, d.features, keep.to(torch.uint8))

    def passes(d0, d1):
        hip.profile_enable(True)
        fpfh.match(d0, d1, method='mfma')
        a, b = hip.fpfh_match_pass_times()
        hip.profile_enable(False)
        return a, b

    def candidates(d0, d1):
        r0, r1 = (d.valid.nonzero().reshape(-1)[:512].contiguous() for d in (d0, d1))
        dbg = hip.fpfh_match(d0.features, d1.features, r0, r1, debug=True)[5]
        return (f'candidates in the 512 x 512 block of the first valid rows: per row mean {dbg["cnt0"].mean():.2f}, max {int(dbg["cnt0"].max())}; '
                f'per column mean {dbg["cnt1"].mean():.2f}, max {int(dbg["cnt1"].max())}')

    p0, p1, _ = synth.make_dense_pair(0, n=args.n)
    dense = [fpfh.describe(p, args.radius, normal_radius=args.normal_radius, voxel=args.voxel) for p in (p0, p1)]
    q0, q1, _ = K.terrain_pair(0)
    small = [fpfh.describe(p, K.TERRAIN_R, voxel=K.TERRAIN_VOXEL) for p in (q0, q1)]
    for name, (d0, d1) in ((f'synth.make_dense_pair(0, n={args.n}) at voxel {args.voxel}', dense), ('terrain pair 0 at voxel 0.05 (the tests\' shape)', small)):
        t, n_matches = race(d0, d1, args.reps)
        a, b = passes(d0, d1)
        sc, mf = np.median(t['scan']), np.median(t['mfma'])
        lines += [f'{name}: {int(d0.valid.sum())} x {int(d1.valid.sum())} valid rows, {n_matches} mutual matches',
                  f'  scan {sc:10.3f}   ({min(t["scan"]):.3f} .. {max(t["scan"]):.3f})',
                  f'  mfma {mf:10.3f}   ({min(t["mfma"]):.3f} .. {max(t["mfma"]):.3f})      scan / mfma = {sc / mf:.1f}',
                  f'  one mfma call: pass A {a:.3f} ms, pass B {b:.3f} ms', '  ' + candidates(d0, d1), '']
    lines += ['sweep over the side length L (the first L valid rows of both sides of the dense pair), median of 3 ms:', f'  {"L":>7s} {"scan":>10s} {"mfma":>10s}  scan / mfma']
    most = min(int(d.valid.sum()) for d in dense)
    for L in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072):
        L = min(L, most)
        t, _ = race(first_rows(dense[0], L), first_rows(dense[1], L), 3)
        sc, mf = np.median(t['scan']), np.median(t['mfma'])
        lines.append(f'  {L:7d} {sc:10.3f} {mf:10.3f}  {sc / mf:8.2f}')
        if L == most:
            break
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--match', action='store_true', help='time the matcher (scan against mfma) instead of the descriptor stages')
    ap.add_argument('--n', type=int, default=300000)
    ap.add_argument('--voxel', type=float, default=0.025)
    ap.add_argument('--normal_radius', type=float, default=0.05)
    ap.add_argument('--radius', type=float, default=0.125)
    ap.add_argument('--reps', type=int, default=None, help='default 20 (10 with --match)')
    ap.add_argument('--out', default=None, help='default profiles/fpfh_timing.txt (profiles/fpfh_match_timing.txt with --match)')
    args = ap.parse_args()
    args.reps = (10 if args.match else 20) if args.reps is None else args.reps
    args.out = os.path.join(ROOT, 'profiles', 'fpfh_match_timing.txt' if args.match else 'fpfh_timing.txt') if args.out is None else args.out
    assert torch.cuda.is_available(), 'time_fpfh.py needs the GPU: there is no host fallback'
    if args.match:
        return match_section(args)
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
