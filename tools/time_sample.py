"""Timing of the farthest-point sampling kernel (csrc/sample.hip) on view 0 of synth.make_dense_pair(0, n=300000), whole
and voxel-downsampled, in every tier that holds the cloud; beside it the same selection written as k iterations of torch operators on the
device (the only formulation there was before the kernel), a batch of 64 clouds in one launch beside 64 single calls, the per-step launch form beside the
persistent one on 1 to 16 large clouds (the crossover behind hip.fps_auto_steps), and fpfh.match on 5000 sampled rows a side beside all rows.

    python tools/time_sample.py [--out profiles/fps_timing.txt] [--n 300000] [--batch 64]

Device events, 2 warm-up rounds, the median of 10.  No counters and no split of a step into its update and its reduction: not measured."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 2, 10
KS = (1000, 5000)
VOXELS = (None, 0.025, 0.05, 0.1)                                # None: the whole cloud; the coarser grids give clouds the lower tiers hold
MATCH_ROWS = 5000


def timed(fn, warm=WARM, reps=REPS):
    """median milliseconds between device events around fn()"""
    import torch
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


def torch_fps(pts, k, start=0):
    """the selection as k iterations of torch operators (float64, the kernel's d2, no FMA: separate multiplies and adds) -> rows int64 [k]"""
    import torch
    p = pts.double()
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    D = torch.full((p.shape[0],), float('inf'), dtype=torch.float64, device=p.device)
    rows = torch.empty(k, dtype=torch.int64, device=p.device)
    c = torch.tensor(start, device=p.device)
    for s in range(k):
        rows[s] = c
        dx, dy, dz = x - x[c], y - y[c], z - z[c]
        D = torch.minimum(D, (dx * dx + dy * dy) + dz * dz)
        D[c] = -1.0                                              # taken
        c = torch.argmax(D)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=300000)
    ap.add_argument('--batch', type=int, default=64)
    a = ap.parse_args()
    import torch
    from roreg_amd import fpfh, hip, sample, synth, voxel
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/time_sample.py on {torch.cuda.get_device_name(0)}: synth.make_dense_pair(0, n={a.n})[0]; device events, {WARM} warm-up rounds, median of {REPS}; '
        f'tiers: lds = n <= {hip.FPS_TIER_EDGES[0]}, reg = n <= {hip.FPS_TIER_EDGES[1]}, mem = any n')
    p0, p1, _ = synth.make_dense_pair(0, n=a.n)
    raw = torch.from_numpy(np.ascontiguousarray(p0, np.float32)).cuda()
    clouds = [(('whole cloud' if v is None else f'voxel {v}'), raw if v is None else voxel.device_downsample(raw, v)[0]) for v in VOXELS]

    say('\n== one cloud, one workgroup: hip.fps, and the torch-operator loop that gives the same rows')
    say(f'{"cloud":<14}{"n":>8}{"k":>6}{"tier":>6}{"ms":>11}{"us / step":>11}{"torch ms":>11}{"torch / hip":>12}   rows')
    for name, pts in clouds:
        n = int(pts.shape[0])
        for k in KS:
            k = min(k, n)
            t_torch = timed(lambda: torch_fps(pts, k), 1, 3)
            want = torch_fps(pts, k)
            for tier in hip.FPS_TIERS[hip.fps_tier(n):] + ('steps',):
                kw = dict(method='steps') if tier == 'steps' else dict(tier=tier, method='persistent')
                t = timed(lambda: hip.fps(pts, k, **kw))
                rows, _, count = hip.fps(pts, k, **kw)
                same = int(count) == k and torch.equal(rows.long(), want)
                say(f'{name:<14}{n:>8}{k:>6}{tier:>6}{t:>11.3f}{t * 1e3 / k:>11.2f}{t_torch:>11.2f}{t_torch / t:>12.1f}   {"the same" if same else "DIFFERENT"}')

    say(f'\n== {a.batch} clouds: one hip.fps_batch launch beside {a.batch} hip.fps calls (one workgroup per cloud: a batch shares the compute units)')
    say(f'{"cloud":<14}{"n":>8}{"k":>6}{"tier":>6}{"batch ms":>11}{"singles ms":>12}{"singles / batch":>17}')
    for name, pts in (clouds[3], clouds[1]):
        n, k = int(pts.shape[0]), 1000
        many = [(pts + 0.001 * q).contiguous() for q in range(a.batch)]
        t_b = timed(lambda: hip.fps_batch([(m, k) for m in many], method='persistent'))
        t_s = timed(lambda: [hip.fps(m, k, method='persistent') for m in many], 1, 5)
        say(f'{name:<14}{n:>8}{k:>6}{hip.FPS_TIERS[hip.fps_tier(n)]:>6}{t_b:>11.3f}{t_s:>12.3f}{t_s / t_b:>17.1f}')

    say(f'\n== few large clouds: the persistent form (one launch, one workgroup a cloud) beside the per-step form (k + 1 launches a cloud, one after the '
        f'other); method auto takes the per-step form while clouds x {hip.FPS_STEPS_ROWS} <= n')
    say(f'{"cloud":<14}{"n":>8}{"k":>6}{"clouds":>8}{"persistent ms":>15}{"steps ms":>11}{"persistent / steps":>20}')
    for name, pts in (clouds[2], clouds[1], clouds[0]):
        n, k = int(pts.shape[0]), 1000
        for T in (1, 2, 4, 8, 16):
            many = [(pts + 0.001 * q).contiguous() for q in range(T)]
            t_p = timed(lambda: hip.fps_batch([(m, k) for m in many], method='persistent'), 1, 5)
            t_s = timed(lambda: hip.fps_batch([(m, k) for m in many], method='steps'), 1, 5)
            say(f'{name:<14}{n:>8}{k:>6}{T:>8}{t_p:>15.3f}{t_s:>11.3f}{t_p / t_s:>20.2f}')

    say(f'\n== fpfh.match (method mfma) of the pair at voxel 0.025 (radius 0.125, normal radius 0.05): every valid row beside {MATCH_ROWS} sampled rows a side')
    d = [fpfh.describe(p, 0.125, normal_radius=0.05, voxel=0.025) for p in (p0, p1)]
    t_fps = timed(lambda: sample.device_farthest([x.points for x in d], MATCH_ROWS))
    rows = [r[0] for r in sample.device_farthest([x.points for x in d], MATCH_ROWS)]
    t_all = timed(lambda: fpfh.match(d[0], d[1], method='mfma'))
    t_kp = timed(lambda: fpfh.match(d[0], d[1], method='mfma', rows0=rows[0], rows1=rows[1]))
    m_all, m_kp = fpfh.match(d[0], d[1], method='mfma'), fpfh.match(d[0], d[1], method='mfma', rows0=rows[0], rows1=rows[1])
    say(f'{"rows":<34}{"ms":>10}   matches')
    say(f'{f"{int(d[0].valid.sum())} x {int(d[1].valid.sum())} (all valid rows)":<34}{t_all:>10.3f}   {int(m_all.shape[0])}')
    say(f'{f"{MATCH_ROWS} x {MATCH_ROWS} (sampled)":<34}{t_kp:>10.3f}   {int(m_kp.shape[0])}')
    say(f'{"sampling both clouds, one launch":<34}{t_fps:>10.3f}   ({int(d[0].points.shape[0])} and {int(d[1].points.shape[0])} points, k = {MATCH_ROWS}, method auto)')
    say('(fpfh.match includes its own read-backs: the valid rows and the count)')
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
