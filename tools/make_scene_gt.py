"""Ground-truth files of a scene from its dense clouds and poses, computed on the GPU (RegistrationEngine.overlap_matrix,
roreg_amd.dense_eval): gt.log (the pairs whose overlap exceeds --overlap, 3DMatch's 30 %), gt.info (their information matrices, the ones
RR_cal.computeTransformationErr consumes) and gtLo.log (the pairs between --low_overlap and --overlap, 3DLoMatch's 10-30 %).

    python tools/make_scene_gt.py --clouds scene/cloud_*.npy --poses scene/poses.npy --out scene/gt_dir --max_dist 0.05 [--voxel 0.025]
                                  [--overlap 0.3] [--low_overlap 0.1] [--force]

clouds: one .npy of [n,3] per cloud, in cloud order (the shell's sorted expansion); poses: .npy [C,4,4], world <- cloud.  A pair (i, j),
i < j, carries T = inv(pose_i) @ pose_j (x_i = R x_j + t, the datasets' get_transform) and its overlap is the smaller of the two directed
overlaps: the share of cloud j's points with a point of cloud i within max_dist, and the reverse.  Existing files are not overwritten
without --force."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def select_pairs(overlap, high, low):
    """overlap [C,C] directed -> (pairs above `high`, pairs in [low, high]), i < j, by min(overlap[i, j], overlap[j, i]); NaN selects nothing."""
    C = overlap.shape[0]
    hi, lo = [], []
    for i in range(C):
        for j in range(i + 1, C):
            o = min(overlap[i, j], overlap[j, i])
            if o > high:
                hi.append((i, j))
            elif low <= o <= high:
                lo.append((i, j))
    return hi, lo


def write_log(path, pairs, n_clouds, poses):
    from roreg_amd.test.estimator import pre_log_entry
    with open(path, 'w') as f:
        for i, j in pairs:
            f.write(pre_log_entry(i, j, n_clouds, np.linalg.inv(poses[i]) @ poses[j]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', nargs='+', required=True)
    ap.add_argument('--poses', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--max_dist', type=float, required=True)
    ap.add_argument('--voxel', type=float, default=None)
    ap.add_argument('--overlap', type=float, default=0.3)
    ap.add_argument('--low_overlap', type=float, default=0.1)
    ap.add_argument('--force', action='store_true')
    a = ap.parse_args()
    names = [os.path.join(a.out, f) for f in ('gt.log', 'gt.info', 'gtLo.log')]
    present = [f for f in names if os.path.exists(f)]
    if present and not a.force:
        sys.exit(f'make_scene_gt: {", ".join(present)} exist; --force overwrites')
    import torch
    assert torch.cuda.is_available(), 'make_scene_gt.py computes on the GPU; there is no host fallback'
    from roreg_amd.engine import CloudState, RegistrationEngine
    from roreg_amd.parses.parses_test import default_config
    from roreg_amd.utils import RR_cal
    poses = np.load(a.poses).astype(np.float64).reshape(-1, 4, 4)
    assert poses.shape[0] == len(a.clouds), 'one pose per cloud'
    eng = RegistrationEngine(default_config(), None, None)
    states = [eng.attach_points(CloudState(before=None), np.load(f), voxel=a.voxel) for f in a.clouds]
    counts, overlap = eng.overlap_matrix(states, poses, a.max_dist)
    hi, lo = select_pairs(overlap, a.overlap, a.low_overlap)
    T = [torch.from_numpy(np.linalg.inv(poses[i]) @ poses[j]).cuda() for i, j in hi]
    info = eng.evaluate_many([(states[i], states[j], Tk) for (i, j), Tk in zip(hi, T)], a.max_dist)[1].cpu().numpy()
    os.makedirs(a.out, exist_ok=True)
    write_log(names[0], hi, len(states), poses)
    RR_cal.write_trajectory_info(names[1], hi, len(states), info)
    write_log(names[2], lo, len(states), poses)
    print(f'{len(states)} clouds, max_dist {a.max_dist}: {len(hi)} pairs above {a.overlap}, {len(lo)} in [{a.low_overlap}, {a.overlap}] -> {a.out}')


if __name__ == '__main__':
    main()
