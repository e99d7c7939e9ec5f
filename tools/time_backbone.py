"""Times the device FCGF backbone (roreg_amd/backbone/fcgf.py, csrc/sparse_conv.hip) on one cloud: synth.make_dense_pair(seed, 300000) at a
2.5 cm voxel over the 60 icosahedral rotations, full-width ResUNetBN2C with seeded weights.

    python tools/time_backbone.py [--seed 7] [--points 300000] [--voxel 0.025] [--out profiles/fcgf_backbone_timing.txt]

Reports the voxel counts per level, every launch of one forward pass of `--layer_batch` rotations (HIP events around each call; FLOPs = 2 Cin
Cout x the map's entries that exist) with its achieved rate, and the whole cloud's wall time (rotation on the host, voxelisation, network,
nearest-neighbour lookup of 5000 keypoints, download) at rot_batch = 1, 12 and 60."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roreg_amd import hip, synth, testset                   # noqa: E402
from roreg_amd.backbone import fcgf                         # noqa: E402
from roreg_amd.group import tables                          # noqa: E402

# v_mfma_f32_32x32x2_f32 issues 1/16 of the fp16 MFMA's products per cycle; profiles/r02_mfma_peak.txt measured 1648 TFLOP/s for fp16 (random operands)
F32_MFMA_PEAK_TFLOPS = 1648.7 / 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--points', type=int, default=300000)
    ap.add_argument('--voxel', type=float, default=0.025)
    ap.add_argument('--layer_batch', type=int, default=12)
    ap.add_argument('--batches', default='1,12,60')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    pts = synth.make_dense_pair(args.seed, args.points)[0].astype(np.float64)
    kps = pts[np.random.default_rng(1).choice(pts.shape[0], 5000, replace=False)]
    model = fcgf.ResUNetBN2C(1, 32, normalize_feature=True, conv1_kernel_size=5)
    synth.seeded_state_dict(model, 5)
    model = model.cuda().eval()
    R = tables().R
    say(f'FCGF backbone (ResUNetBN2C, conv1 kernel 5, seeded weights), synth.make_dense_pair({args.seed}, {args.points})[0] at voxel {args.voxel}, '
        f'{torch.cuda.get_device_name(0)}')

    # ---- one forward pass of layer_batch rotations, every launch between two events ----
    vox = [testset._voxelise((pts @ R[g].T).astype(np.float32), args.voxel) for g in range(args.layer_batch)]
    c4, cuts = testset._batch_coords([c for _, c in vox])
    say(f'voxels of rotation 0: {int(cuts[1])}; of {args.layer_batch} rotations as one sparse tensor: {c4.shape[0]}')
    model(c4, cuts)                                          # warm-up
    records, real = [], {n: getattr(hip, n) for n in ('sparse_stride_map', 'sparse_kernel_map', 'sparse_conv', 'sparse_l2norm')}

    def timed(name):
        def call(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); r = real[name](*a, **kw); e1.record(); torch.cuda.synchronize()
            flops, what = 0, name
            if name == 'sparse_conv':
                W, M = a[1], a[2]
                W = W[None] if W.dim() == 2 else W
                flops = 2 * W.shape[1] * W.shape[2] * int((M >= 0).sum())
                what = f'conv {W.shape[1]:3d} -> {W.shape[2]:3d}, K {W.shape[0]:3d}, rows {M.shape[0]}'
            elif name == 'sparse_kernel_map':
                what = f'kernel map k {a[2]}, step {a[3]:2d}, rows {a[1].shape[0]}'
            elif name == 'sparse_stride_map':
                what = f'stride map ts {a[2]}, rows {a[0].shape[0]} -> {r.coords.shape[0]}'
            records.append((what, e0.elapsed_time(e1), flops))
            return r
        return call

    for n in real:
        setattr(hip, n, timed(n))
    try:
        model(c4, cuts)
    finally:
        for n, f in real.items():
            setattr(hip, n, f)
    say(f'\nper launch, one forward pass of {args.layer_batch} rotations (each launch synchronised: the sum is above the pass\'s own time):')
    for what, ms, flops in records:
        say(f'  {what:48s} {ms:9.3f} ms' + (f'  {flops / 1e9:9.2f} GFLOP  {flops / ms / 1e9:7.2f} TFLOP/s' if flops else ''))
    conv_ms = sum(ms for w, ms, f in records if f); conv_fl = sum(f for _, _, f in records)
    map_ms = sum(ms for w, ms, f in records if not f)
    say(f'  convolutions: {conv_fl / 1e9:.1f} GFLOP in {conv_ms:.1f} ms = {conv_fl / conv_ms / 1e9:.2f} TFLOP/s '
        f'({100 * conv_fl / conv_ms / 1e9 / F32_MFMA_PEAK_TFLOPS:.1f} % of the f32-input MFMA peak, {F32_MFMA_PEAK_TFLOPS:.0f} TFLOP/s); maps and the rest: {map_ms:.1f} ms')
    say(f'  per rotation: {conv_fl / args.layer_batch / 1e9:.1f} GFLOP; per cloud (60 rotations): {conv_fl / args.layer_batch * 60 / 1e12:.2f} TFLOP')
    block2_tr = sum(f for _, _, f in records[-5:-3])         # the last launches: ..., block2_tr.conv1, block2_tr.conv2, conv1_tr, final, l2norm
    say(f'  block2_tr (two 64 -> 64 convolutions at full resolution): {100 * block2_tr / conv_fl:.0f} % of the FLOPs')

    # ---- the whole cloud ----
    say('\nwhole cloud, 60 rotations, 5000 keypoints (host rotation + upload + voxelisation + network + nearest neighbour + download), wall time:')
    for rb in (int(b) for b in args.batches.split(',')):
        ts = []
        for _ in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f = testset.extract_group_features(model, pts, kps, args.voxel, rb)
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        say(f'  rot_batch {rb:2d}: {min(ts):7.3f} s (runs: {", ".join(f"{t:.3f}" for t in ts)}), peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, '
            f'features {f.shape} finite: {bool(np.isfinite(f).all())}')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
