"""Timing of the DBSCAN kernels (csrc/cluster.hip) on one cloud of synth.make_dense_pair(0, n=300000), whole and
voxel-downsampled at 0.025, at eps 0.05 and min_points 1 and 6.

    python tools/time_cluster.py [--out profiles/cluster_timing.txt] [--n 300000] [--voxel 0.025] [--eps 0.05] [--no_trace]

The whole call (hip.grid_dbscan on a grid built for eps outside the timing): device events, 2 warm-up rounds, the median of 10.  Beside it the
yardstick for the two walking passes: hip.grid_knn(grid, 1, eps), the radius filter's kernel, which walks the same balls once.  Each launch of
the call: from a `rocprofv3 --kernel-trace` run of its own (a fresh child process that only repeats the calls, started before this process
opens the device), the median of the same 10 repetitions."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_POINTS = (1, 6)
WARM, REPS = 2, 10
TAIL = ('cluster_shorten_kernel', 'cluster_hook_kernel', 'cluster_settle_kernel', 'cluster_flag_kernel', 'icp_scan_sums_kernel', 'icp_scan_top_kernel',
        'icp_scan_apply_kernel', 'cluster_label_kernel')


def launches(min_points):
    """the kernels of one call, in launch order (at min_points = 1 the count launch does the link launch's work)"""
    return ('cluster_count_kernel',) + (() if min_points == 1 else ('cluster_link_kernel',)) + TAIL


def clouds(n, voxel_edge):
    import torch
    from roreg_amd import synth, voxel
    pts = torch.from_numpy(np.ascontiguousarray(synth.make_dense_pair(0, n=n)[0], np.float32)).cuda()
    return ((f'voxel {voxel_edge}', voxel.device_downsample(pts, voxel_edge)[0]), ('whole cloud', pts))


def timed(fn):
    """median milliseconds between device events around fn()"""
    import torch
    for _ in range(WARM):
        fn()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def trace_child(a):
    """what the traced process runs: per cloud and min_points, WARM + REPS calls and nothing else between them"""
    import torch
    from roreg_amd import hip
    for _, pts in clouds(a.n, a.voxel):
        grid = hip.IcpGrid(pts, a.eps)
        for mp in MIN_POINTS:
            torch.cuda.synchronize()
            for _ in range(WARM + REPS):
                hip.grid_dbscan(grid, a.eps, mp)
            torch.cuda.synchronize()


def traced_launches(a):
    """-> {(cloud index, min_points): {launch: median microseconds}} from a rocprofv3 --kernel-trace run of trace_child, or a string saying why not"""
    prof = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(prof):
        return 'rocprofv3 was not found'
    out = tempfile.mkdtemp(prefix='cluster_trace_')
    try:
        cmd = [prof, '--kernel-trace', '--output-format', 'csv', '-d', out, '--', sys.executable, os.path.abspath(__file__), '--trace_child', '--n', str(a.n),
               '--voxel', str(a.voxel), '--eps', str(a.eps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        files = glob.glob(os.path.join(out, '**', '*kernel_trace.csv'), recursive=True)
        if p.returncode != 0 or not files:
            return f'the traced run ended with status {p.returncode} and {len(files)} trace files: {(p.stdout + p.stderr)[-400:]}'
        rows = []
        for f in files:
            with open(f, newline='') as fh:
                rows += [(int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(fh)]
    finally:
        shutil.rmtree(out, ignore_errors=True)
    rows.sort()
    names = [r[2] for r in rows]
    starts = [i for i, nm in enumerate(names) if 'cluster_count_kernel' in nm]
    per = WARM + REPS
    if len(starts) != 2 * len(MIN_POINTS) * per:
        return f'{len(starts)} calls in the trace, {2 * len(MIN_POINTS) * per} expected'
    res = {}
    for c, i in enumerate(starts):
        key = (c // (per * len(MIN_POINTS)), MIN_POINTS[(c // per) % len(MIN_POINTS)])
        want_all = launches(key[1])
        call = rows[i:i + len(want_all)]
        if len(call) != len(want_all) or any(want not in got[2] for want, got in zip(want_all, call)):
            return f'call {c} of the trace is not the launches of one call: {[r[2][:40] for r in call]}'
        if c % per < WARM:
            continue
        for want, got in zip(want_all, call):
            res.setdefault(key, {}).setdefault(want, []).append((got[1] - got[0]) / 1e3)
        res[key].setdefault('first start to last end', []).append((call[-1][1] - call[0][0]) / 1e3)
    return {k: {nm: float(np.median(v)) for nm, v in d.items()} for k, d in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=300000)
    ap.add_argument('--voxel', type=float, default=0.025)
    ap.add_argument('--eps', type=float, default=0.05)
    ap.add_argument('--no_trace', action='store_true', help='skip the rocprofv3 run (the whole-call table only)')
    ap.add_argument('--trace_child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a)
    trace = 'skipped (--no_trace)' if a.no_trace else traced_launches(a)           # (before this process opens the device)
    import torch
    from roreg_amd import hip
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/time_cluster.py on {torch.cuda.get_device_name(0)}: synth.make_dense_pair(0, n={a.n})[0], eps {a.eps}; device events, {WARM} warm-up rounds, '
        f'median of {REPS}; launches from a rocprofv3 --kernel-trace run of its own')
    for c, (name, pts) in enumerate(clouds(a.n, a.voxel)):
        n = int(pts.shape[0])
        grid = hip.IcpGrid(pts, a.eps)
        t_walk = timed(lambda: hip.grid_knn(grid, 1, a.eps))
        ball = float(hip.grid_knn(grid, 1, a.eps)[2].double().mean()) + 1.0
        say(f'\n== {name}: {n} points, mean ball {ball:.1f} rows (itself included)')
        say(f'{"call":<44}{"ms":>10}{"x walk":>9}   notes')
        say(f'{f"grid_knn k=1 r={a.eps} (the radius filter)":<44}{t_walk:>10.3f}{1.0:>9.2f}   the same grid, the same balls, one walk')
        for mp in MIN_POINTS:
            t = timed(lambda: hip.grid_dbscan(grid, a.eps, mp))
            labels, core, nc, sizes = hip.grid_dbscan(grid, a.eps, mp)
            say(f'{f"grid_dbscan eps={a.eps} min_points={mp}":<44}{t:>10.3f}{t / t_walk:>9.2f}   {int(nc.item())} clusters, the largest {int(sizes.max())} rows, '
                f'{int(core.sum())} core, {int(((labels >= 0) & (core == 0)).sum())} border, {int((labels < 0).sum())} noise')
            if isinstance(trace, dict):
                d = trace[(c, mp)]
                for nm in launches(mp) + ('first start to last end',):
                    say(f'{"    " + nm:<44}{d[nm] / 1e3:>10.3f}{d[nm] / 1e3 / t_walk:>9.2f}')
    if not isinstance(trace, dict):
        say(f'\nlaunches: {trace}')
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
