"""Times the raw-cloud route on a synthetic scene of dense clouds (synth.make_dense_pair), full-width FCGF backbone and GF / ET networks with
seeded weights, 5000 keypoints per cloud:

    python tools/time_raw_scene.py [--seed 7] [--points 300000] [--clouds 4] [--voxel 0.025] [--rot_batch 12] [--out profiles/raw_scene_timing.txt]

Per cloud, wall time (synchronised, two repeats after one warm-up pass each) of
  (a) the file route's work without the file: testset.extract_group_features (features assembled by torch, downloaded) + the upload
      RegistrationEngine.extract_many does with a host array;
  (b) testset.group_features_device (assembled by hip.group_feature_assemble, left on the device);
and (c) the whole scene through register.Registrar.scene, split with engine.phase_ms into backbone (the source's calls, timed around
source[i]), extractor (phase 'extract' less the backbone) and the per-pair stages; peak device memory; and the shard plan's cloud_cost =
seconds per cloud through source + extractor over seconds per pair."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roreg_amd import synth, testset                         # noqa: E402
from roreg_amd.backbone import fcgf                          # noqa: E402
from roreg_amd.engine import RegistrationEngine              # noqa: E402
from roreg_amd.network import name2network                   # noqa: E402
from roreg_amd.parses.parses_test import default_config      # noqa: E402
from roreg_amd.register import Registrar                     # noqa: E402


class TimedSource(testset.GroupFeatureSource):
    """The source with a synchronised clock around every cloud."""
    seconds = 0.0

    def __getitem__(self, i):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        f = super().__getitem__(i)
        torch.cuda.synchronize(); self.seconds += time.perf_counter() - t0
        return f


class TimedRegistrar(Registrar):
    def source(self, clouds, keypoints, keep_points=False):
        return TimedSource(self.backbone, lambda i: clouds[i], lambda i: keypoints[i], self.voxel_size, self.rot_batch, self.engine.feat_dtype,
                           keep_points=keep_points, ids=range(len(clouds)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--points', type=int, default=300000)
    ap.add_argument('--clouds', type=int, default=4)
    ap.add_argument('--keypoints', type=int, default=5000)
    ap.add_argument('--voxel', type=float, default=0.025)
    ap.add_argument('--rot_batch', type=int, default=12)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    clouds = [c.astype(np.float64) for q in range((args.clouds + 1) // 2) for c in synth.make_dense_pair(args.seed + q, args.points)[:2]][:args.clouds]
    kps = [c[np.random.default_rng(1 + q).choice(c.shape[0], args.keypoints, replace=False)] for q, c in enumerate(clouds)]
    pairs = [(a, b) for a in range(len(clouds)) for b in range(a + 1, len(clouds))]
    model = fcgf.ResUNetBN2C(1, 32, normalize_feature=True, conv1_kernel_size=5)
    synth.seeded_state_dict(model, 5)
    model = model.cuda().eval()
    cfg = default_config(keynum=args.keypoints, ET='yohoo', SO3_related_files=None)
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    engine = RegistrationEngine(cfg, gf, et)
    say(f'raw-cloud route, {len(clouds)} clouds of synth.make_dense_pair({args.seed}.., {args.points}) at voxel {args.voxel}, rot_batch {args.rot_batch}, '
        f'{args.keypoints} keypoints, {len(pairs)} pairs, full-width FCGF + GF + ET with seeded weights, {torch.cuda.get_device_name(0)}')

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def route_a(q):
        f = testset.extract_group_features(model, clouds[q], kps[q], args.voxel, args.rot_batch)
        return torch.from_numpy(f).to('cuda', torch.float32).to(engine.feat_dtype)               # extract_many's upload of a host array

    def route_b(q):
        return testset.group_features_device(model, clouds[q], kps[q], args.voxel, args.rot_batch, engine.feat_dtype)

    say('\nper cloud, wall time in seconds (one warm-up pass over the clouds, then two repeats):')
    per_route = {}
    for name, fn in (('(a) extract_group_features + upload', route_a), ('(b) group_features_device', route_b)):
        for q in range(len(clouds)):
            fn(q)
        reps = []
        for _ in range(2):
            ts = [timed(lambda q=q: fn(q))[0] for q in range(len(clouds))]
            reps.append(sum(ts) / len(ts))
        per_route[name] = reps
        say(f'  {name:40s} {min(reps):7.4f}  (repeats: {", ".join(f"{t:.4f}" for t in reps)}; spread {abs(reps[0] - reps[1]):.4f})')
    a, b = per_route['(a) extract_group_features + upload'], per_route['(b) group_features_device']
    spread = max(abs(a[0] - a[1]), abs(b[0] - b[1]))
    same = torch.equal(route_a(0).view(torch.int32 if engine.feat_dtype == torch.float32 else torch.int16),
                       route_b(0).view(torch.int32 if engine.feat_dtype == torch.float32 else torch.int16))
    say(f'  (b) - (a) = {min(b) - min(a):+.4f} s per cloud (spread of the repeats: {spread:.4f} s); the two features are bitwise equal: {same}')
    if min(b) - min(a) > spread:
        say('  NOTE: (b) is slower than (a) by more than the spread of the repeats')

    say(f'\n(c) the whole scene through Registrar.scene (seeded; {len(pairs)} pairs), synchronised phases of engine.phase_ms, seconds:')
    reg = TimedRegistrar(engine, model, args.voxel, args.rot_batch, args.keypoints)
    reg.scene(clouds, pairs, keypoints=kps, seed=3)                                                # warm-up
    rows = []
    for _ in range(2):
        torch.cuda.reset_peak_memory_stats()
        engine.phase_ms = {}
        wall, res = timed(lambda: reg.scene(clouds, pairs, keypoints=kps, seed=3))
        ph = {k: v / 1e3 for k, v in engine.phase_ms.items()}
        engine.phase_ms = None
        backbone = reg.last_source.seconds
        extractor = ph.get('extract', 0.0) - backbone
        per_pair = sum(v for k, v in ph.items() if k != 'extract')
        rows.append((wall, backbone, extractor, per_pair, torch.cuda.max_memory_allocated() / 2 ** 30))
        say(f'  wall {wall:7.3f}: backbone {backbone:7.3f} ({backbone / len(clouds):.4f} per cloud), extractor {extractor:7.4f} ({extractor / len(clouds):.4f} per cloud), '
            f'per-pair stages {per_pair:7.4f} ({per_pair / len(pairs):.5f} per pair: ' + ', '.join(f'{k} {v:.4f}' for k, v in ph.items() if k != 'extract') +
            f'); peak device memory {rows[-1][4]:.1f} GiB; backbone runs per cloud {sorted(set(reg.last_source.runs.values()))}; '
            f'matches per pair {[r.n_match for r in res]}')
    best = min(rows)
    cloud_s, pair_s = (best[1] + best[2]) / len(clouds), best[3] / len(pairs)
    say(f'\ncloud_cost = seconds per cloud through source + extractor / seconds per pair = {cloud_s:.4f} / {pair_s:.5f} = {cloud_s / pair_s:.0f}')
    say(f'  (the per-pair figure comes from a scene of {len(pairs)} pairs and carries the scene\'s fixed host synchronisations; shard_scenes\' own fit on '
        f'full scenes is 0.29 ms per pair, which would give {cloud_s / 0.29e-3:.0f}.  The ratio shapes the shard plan only: no result depends on it.)')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
