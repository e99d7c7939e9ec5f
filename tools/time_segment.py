"""Timing of the plane segmentation kernels (csrc/plane.hip) on view 0 of synth.make_dense_pair(0, n=300000), whole and
voxel-downsampled at 0.025 and 0.05, at 256, 1024 and 4096 hypotheses a round and 6 planes; beside it the same selection written with torch
operators on the device (the draws on the host from the live count, the support as chunked float64 products, argmax, masked assignment), which
must give the same labels.  The scoring pass alone (hip.plane_score) on round 0's triples is timed too.

    python tools/time_segment.py [--out profiles/segment_timing.txt] [--n 300000]

Device events, 2 warm-up rounds, the median of 10 (the torch form: 1 and 3).  No counters, no split of a round into its launches, no other
dist, no cloud above 300,000 rows: not measured."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

WARM, REPS = 2, 10
VOXELS = (None, 0.025, 0.05)
HYPS = (256, 1024, 4096)
PLANES, DIST, SEED = 6, 0.01, 1
TORCH_CHUNK_BYTES = 1 << 28                                       # one float64 [chunk, L] temporary of the torch form


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


def torch_planes(pts, dist, n_hyp, max_planes, min_inliers, seed):
    """the segmentation with torch operators (float64, the kernel's operation order, separate multiplies and adds) -> labels int32 [n]"""
    import torch
    import _plane_oracle as PO
    X = pts.double()
    labels = torch.full((X.shape[0],), -1, dtype=torch.int32, device=X.device)
    alive = torch.isfinite(X).all(1)
    d2 = float(dist) * float(dist)
    for r in range(max_planes):
        live = torch.nonzero(alive & (labels < 0)).reshape(-1)
        L = int(live.shape[0])
        if L < 3:
            break
        idx = torch.from_numpy(PO.draws(seed, r, n_hyp, L)).to(X.device)
        distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
        Y = X[live]
        A, B, C = Y[idx[:, 0]], Y[idx[:, 1]], Y[idx[:, 2]]
        e1, e2 = B - A, C - A
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        q = (nx * nx + ny * ny) + nz * nz
        valid = distinct & (q != 0) & torch.isfinite(q)
        thr = d2 * q
        x, y, z = Y[:, 0].contiguous(), Y[:, 1].contiguous(), Y[:, 2].contiguous()
        chunk = max(1, TORCH_CHUNK_BYTES // (8 * L))
        cnt = torch.empty(n_hyp, dtype=torch.int64, device=X.device)

        def inside(h0, h1):
            s = (nx[h0:h1, None] * (x[None, :] - A[h0:h1, 0:1]) + ny[h0:h1, None] * (y[None, :] - A[h0:h1, 1:2])) + nz[h0:h1, None] * (z[None, :] - A[h0:h1, 2:3])
            return s * s <= thr[h0:h1, None]

        for h0 in range(0, n_hyp, chunk):
            cnt[h0:h0 + chunk] = inside(h0, min(h0 + chunk, n_hyp)).sum(1)
        cnt = torch.where(valid, cnt, torch.full_like(cnt, -1))
        key = cnt * n_hyp + (n_hyp - 1 - torch.arange(n_hyp, device=X.device))          # (count descending, h ascending)
        h = int(torch.argmax(key))
        if int(cnt[h]) < min_inliers:
            break
        labels[live[inside(h, h + 1)[0]]] = r
    return labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--n', type=int, default=300000)
    a = ap.parse_args()
    import torch
    from roreg_amd import hip, synth, voxel
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'tools/time_segment.py on {torch.cuda.get_device_name(0)}: synth.make_dense_pair(0, n={a.n})[0], dist {DIST}, {PLANES} planes, seed {SEED}; device events, '
        f'{WARM} warm-up rounds, median of {REPS} (torch form: 1 and 3)')
    p0 = synth.make_dense_pair(0, n=a.n)[0]
    raw = torch.from_numpy(np.ascontiguousarray(p0, np.float32)).cuda()
    clouds = [(('whole cloud' if v is None else f'voxel {v}'), raw if v is None else voxel.device_downsample(raw, v)[0]) for v in VOXELS]
    say(f'\n{"cloud":<14}{"n":>8}{"H":>6}{"planes":>8}{"segment ms":>12}{"ms / round":>12}{"score ms":>10}{"G tests/s":>11}{"torch ms":>11}{"torch / hip":>12}   labels')
    for name, pts in clouds:
        n = int(pts.shape[0])
        min_inliers = max(3, n // 100)
        for H in HYPS:
            run = lambda: hip.plane_segment(pts, DIST, H, PLANES, min_inliers, SEED)
            t = timed(run)
            labels, n_planes, counts, triples, raw_planes, fit, rms = run()
            k = int(n_planes)
            t_torch = timed(lambda: torch_planes(pts, DIST, H, PLANES, min_inliers, SEED), 1, 3)
            same = torch.equal(labels, torch_planes(pts, DIST, H, PLANES, min_inliers, SEED))
            import _plane_oracle as PO
            trip = torch.from_numpy(PO.draws(SEED, 0, H, n).astype(np.int32)).cuda()          # round 0's draws: every row is live in this cloud
            t_score = timed(lambda: hip.plane_score(pts, trip, DIST))
            say(f'{name:<14}{n:>8}{H:>6}{k:>8}{t:>12.3f}{t / PLANES:>12.3f}{t_score:>10.3f}{n * H / t_score / 1e6:>11.1f}{t_torch:>11.2f}{t_torch / t:>12.1f}   '
                f'{"the same" if same else "DIFFERENT"}')
    say('(segment ms: all 6 rounds of hip.plane_segment, 12 launches a round, nothing read back; score ms: hip.plane_score, the check launch and the scoring pass over '
        'all rows; G tests/s: rows x hypotheses of that pass per second; the torch form reads the live count and the winner back every round)')
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
