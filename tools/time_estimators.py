"""The three estimators side by side on one GPU: pairs/s of the engine under --ET yohoo, yohoc and sc2 on the kitchen-shaped synthetic scene
(bench.py's BASELINE configs[1] shape: 60 clouds, 449 pairs, 5000 keypoints, mutual matcher), the sc2 kernels' times per pair from events,
and RR / RRE / RTE of the three on synth.make_scene_device scenes at overlap 0.6 and 0.2.

    python tools/time_estimators.py [--kpts 5000] [--passes 2] [--repeats 2] [--out profiles/sc2_estimator_timing.txt]

The estimators alternate (yohoo, yohoc, sc2, yohoo, ...) after one warm-up round each, so a drift of the box shows in every column alike."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from roreg_amd import hip, synth                                          # noqa: E402
from roreg_amd.engine import RegistrationEngine                            # noqa: E402
from roreg_amd.network import name2network                                 # noqa: E402
from roreg_amd.parses.parses_test import default_config                    # noqa: E402
from roreg_amd.register import pair_seeds                                  # noqa: E402
from roreg_amd.utils.r_eval import compute_R_diff                          # noqa: E402

ESTIMATORS = ('yohoo', 'yohoc', 'sc2')


def engines(kpts, gemm):
    out = {}
    gf = name2network['GF_test'](default_config()); synth.seeded_state_dict(gf, 101)
    for ET in ESTIMATORS:
        cfg = default_config(keynum=kpts, max_iter=1000, ET=ET)
        et = None
        if ET == 'yohoo':
            et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
        out[ET] = RegistrationEngine(cfg, gf, et); out[ET].set_gemm_mode(gemm)
    return out


def accuracy(res, poses):
    """(RR, mean RRE, mean RTE over the successes) with the evaluator's pointdsc criterion: RRE < 15 degrees and RTE < 0.3 m"""
    rre, rte = [], []
    for r in res:
        gt = synth.pose_transform(poses, r.id0, r.id1)
        if np.isfinite(r.trans).all():
            rre.append(compute_R_diff(r.trans[:3, :3], gt[:3, :3])); rte.append(float(np.linalg.norm(r.trans[:3, 3] - gt[:3, 3])))
        else:
            rre.append(np.inf); rte.append(np.inf)
    rre, rte = np.array(rre), np.array(rte)
    ok = (rre < 15) & (rte < 0.3)
    return float(ok.mean()), float(rre[ok].mean()) if ok.any() else float('nan'), float(rte[ok].mean()) if ok.any() else float('nan')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kpts', type=int, default=5000)
    ap.add_argument('--passes', type=int, default=2, help='pipelined passes over the scene per timed run')
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--gemm', default=hip.GEMM_MODE)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = []

    def say(s=''):
        print(s, flush=True); lines.append(s)
    n_clouds, n_pairs = synth.THREEDMATCH_CLOUDS[0], synth.THREEDMATCH_PAIRS[0]
    feats, keys, poses = synth.make_scene_device(500, n_clouds, args.kpts, 0.6)
    pairs = [(str(a), str(b)) for a, b in synth.scene_pair_list(n_clouds, n_pairs, 900, locality=8.0)]
    seeds = pair_seeds(0, pairs)
    eng = engines(args.kpts, args.gemm)
    job = (feats, keys, pairs, dict(pair_seeds=seeds))
    say(f'# kitchen-shaped synthetic scene: {n_clouds} clouds, {n_pairs} pairs, {args.kpts} keypoints, overlap 0.6, mutual matcher, max_iter 1000, gemm {args.gemm}')
    say(f'# {torch.cuda.get_device_name(0)}; each run = {args.passes} pipelined passes (run_scenes); estimators alternate after one warm-up run each')
    for ET in ESTIMATORS:
        eng[ET].run_scenes([job] * args.passes)
    rate = {ET: [] for ET in ESTIMATORS}
    last = {}
    for rep in range(args.repeats):
        for ET in ESTIMATORS:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            last[ET] = eng[ET].run_scenes([job] * args.passes)[-1]
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            rate[ET].append(n_pairs * args.passes / dt)
    say()
    say('estimator   pairs/s per repeat          RR      RRE [deg]  RTE [m]   mean recalltime')
    for ET in ESTIMATORS:
        rr, rre, rte = accuracy(last[ET], poses)
        say(f'{ET:10s}  {"  ".join(f"{v:8.1f}" for v in rate[ET]):28s}  {rr:6.4f}  {rre:9.4f}  {rte:8.5f}  {np.mean([r.recalltime for r in last[ET]]):8.1f}')
    # the sc2 kernels alone, from events, on the scene's own match lists
    res = eng['sc2'].run_scene(feats, keys, pairs, pair_seeds=seeds, keep_matches=True)
    tasks = [(keys[int(r.id0)], keys[int(r.id1)], r.matches) for r in res]
    M = np.array([int(r.n_match) for r in res])
    ird = float(eng['sc2'].cfg.ransac_ird)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ms = []
    for rep in range(args.repeats + 1):
        ev[0].record()
        Trans, offsets = hip.sc2_hypotheses_batch(tasks, ird, 1000, 20)
        ev[1].record()
        hip.ransac_batch([(k0, k1, m, None, Trans[o:o + S], None) for (k0, k1, m), (o, S) in zip(tasks, offsets)], ird)
        ev[2].record()
        torch.cuda.synchronize()
        ms.append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    say()
    say(f'sc2 on the scene\'s {len(tasks)} match lists (M min / mean / max = {M.min()} / {M.mean():.0f} / {M.max()}; first run = warm-up), ms per pair from events:')
    for rep, (a, b) in enumerate(ms):
        say(f'  run {rep}: hypotheses (6 launches per group: gather, compatibility, degree, rank, second order, fit) {a / len(tasks):7.4f}   '
            f'scoring + 2 refinements (hip.ransac_batch) {b / len(tasks):7.4f}')
    del feats, keys, tasks, res, last, job
    # accuracy at two overlaps on a 16-cloud scene
    say()
    say('accuracy on synth.make_scene_device(seed, 16 clouds, 60 pairs): RR / RRE [deg] / RTE [m] (pointdsc criterion, means over the successes)')
    for overlap in (0.6, 0.2):
        f2, k2, p2 = synth.make_scene_device(1400, 16, args.kpts, overlap)
        pr = [(str(a), str(b)) for a, b in synth.scene_pair_list(16, 60, 4242)]
        sd = pair_seeds(1, pr)
        for ET in ESTIMATORS:
            rr, rre, rte = accuracy(eng[ET].run_scene(f2, k2, pr, pair_seeds=sd), p2)
            say(f'  overlap {overlap}: {ET:6s} {rr:6.4f} / {rre:7.4f} / {rte:7.5f}')
        del f2, k2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
