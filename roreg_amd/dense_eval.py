"""Read-only evaluation of a dense pair under a given transform, on the device (csrc/icp.hip, include/roreg_hip.h "v6g"; no reference
counterpart: the reference reads a benchmark's gt.info, it never computes one).

    from roreg_amd import dense_eval
    e = dense_eval.evaluate(points0, points1, T, max_dist=0.05)             # one pair -> PairEval
    es = dense_eval.evaluate([(points0, points1, T), ...], max_dist=0.05)   # many pairs, the same two launches -> [PairEval]
    e, mask0, mask1 = dense_eval.evaluate(points0, points1, T, max_dist=0.05, overlap_masks=True)

points0 is the target (cloud 0), points1 the source (cloud 1), T [4,4] float64 in the engine's convention k0 ~ k1 R^T + t.  overlap1 = the
share of cloud 1's points with a point of cloud 0 within max_dist under T (n01 of them, root mean square distance rmse01); overlap0, n10,
rmse10 the other way round under the inverse; info = the 6x6 information matrix of the forward correspondences in Redwood's order and
scaling, the one RR_cal.computeTransformationErr divides by its [0,0] entry (RR_cal.write_trajectory_info writes a gt.info from them).
RegistrationEngine.evaluate_many / overlap_matrix are the device-resident forms."""
from collections import namedtuple

import numpy as np

from . import hip
from . import voxel as voxel_grid
from .icp import device_points, device_transform

PairEval = namedtuple('PairEval', 'n01 n10 overlap0 overlap1 rmse01 rmse10 info status')
PairEval.__doc__ = ("n01, n10: correspondences source -> target and target -> source; overlap0 = n10 / n_tgt, overlap1 = n01 / n_src (NaN for an empty "
                    "cloud); rmse01, rmse10 (NaN without correspondences); info [6,6] float64; status: 'ok' | 'nonfinite' (T not finite: counts 0, info 0)")


def results_to_host(stats, info, status):
    """icp_eval_batch's device tensors -> [PairEval] (one synchronising copy each)."""
    stats, info, status = (v.cpu().numpy() for v in (stats, info, status))
    return [PairEval(int(s[0]), int(s[1]), float(s[2]), float(s[3]), float(s[4]), float(s[5]), info[i].copy(), hip.ICP_EVAL_STATUS[int(status[i])])
            for i, s in enumerate(stats)]


def evaluate(points0, points1=None, T=None, max_dist=None, voxel=None, voxel_mode='centroid', device='cuda', overlap_masks=False):
    """One pair (points0, points1, T) -> PairEval, or a list of such triples as the first argument -> [PairEval].  An array that appears in
    several pairs (the same object) is uploaded and gridded once.  voxel=: every distinct array is voxel-grid downsampled once, where it is
    uploaded (roreg_amd.voxel); counts and overlaps are then the downsampled clouds'.  overlap_masks=True: every result becomes (PairEval,
    mask0 bool [n_tgt], mask1 bool [n_src]): the points of either cloud that have a point of the other within max_dist."""
    if max_dist is None:
        raise ValueError('evaluate: max_dist is required')
    if voxel is not None:
        voxel_grid.check_args(voxel, voxel_mode, 'evaluate')
    single = points1 is not None
    items = [(points0, points1, T)] if single else list(points0)
    grids = {}

    def grid(p):
        g = grids.get(id(p))
        if g is None:
            pts = device_points(p, device)
            if voxel is not None:
                pts = voxel_grid.device_downsample(pts, voxel, voxel_mode)[0]
            g = grids[id(p)] = hip.IcpGrid(pts, max_dist)
        return g

    pairs = [(grid(p0), grid(p1), device_transform(Tp, device)) for p0, p1, Tp in items]
    res = hip.icp_eval_batch(pairs, max_dist, want_assign=overlap_masks)
    out = results_to_host(*res[:3])
    if overlap_masks:
        out = [(e, a10.cpu().numpy() >= 0, a01.cpu().numpy() >= 0) for e, a01, a10 in zip(out, res[3], res[4])]
    return out[0] if single else out
