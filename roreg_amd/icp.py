"""Dense point-to-point ICP refinement of registered pairs on the device (csrc/icp.hip; no reference counterpart: the reference ends at the
keypoint transform, and its users refine on the host with a k-d tree).

    from roreg_amd import icp
    res = icp.refine(points0, points1, T0, max_dist=0.07)            # one pair -> IcpResult
    res = icp.refine([(points0, points1, T0), ...], max_dist=0.07)   # many pairs, the same launches -> [IcpResult]

points0 is the target (cloud 0), points1 the source (cloud 1), T0 [4,4] float64 in the engine's convention k0 ~ k1 R^T + t.  Coordinates are
rounded to float32 once, at upload; all arithmetic is float64.  RegistrationEngine.icp_many is the device-resident form (grids cached per
cloud, results left on the device)."""
from collections import namedtuple

import numpy as np
import torch

from . import hip

IcpResult = namedtuple('IcpResult', 'T iters inliers rmse status')
IcpResult.__doc__ = ('T [4,4] float64; iters: searches executed; inliers, rmse: of the last executed search; '
                     "status: 'converged' | 'max_iter' | 'no_support' (T0 kept) | 'nonfinite' (T0 returned unchanged)")

TOL_DEG, TOL_T = 1e-4, 1e-6


def device_points(pts, device='cuda'):
    """host array or tensor [n,3] -> contiguous float32 device tensor (the one rounding of the coordinates)."""
    if torch.is_tensor(pts):
        t = pts.to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(pts).reshape(-1, 3), np.float32)).to(device)
    return t.reshape(-1, 3).contiguous()


def device_transform(T, device='cuda'):
    if torch.is_tensor(T):
        return T.to(device=device, dtype=torch.float64).reshape(4, 4).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(T, np.float64).reshape(4, 4))).to(device)


def results_to_host(T, iters, inliers, rmse, status):
    """icp_batch's device tensors -> [IcpResult] (one synchronising copy each)."""
    T, iters, inliers, rmse, status = (v.cpu().numpy() for v in (T, iters, inliers, rmse, status))
    return [IcpResult(T[i].copy(), int(iters[i]), int(inliers[i]), float(rmse[i]), hip.ICP_STATUS[int(status[i])]) for i in range(T.shape[0])]


def refine(points0, points1=None, T0=None, max_dist=None, max_iter=30, tol_deg=TOL_DEG, tol_t=TOL_T, device='cuda'):
    """One pair (points0, points1, T0) -> IcpResult, or a list of such triples as the first argument -> [IcpResult].  An array that
    appears in several pairs (the same object) is uploaded and gridded once."""
    if max_dist is None:
        raise ValueError('refine: max_dist is required')
    single = points1 is not None
    items = [(points0, points1, T0)] if single else list(points0)
    grids = {}

    def grid(p):
        g = grids.get(id(p))
        if g is None:
            g = grids[id(p)] = hip.IcpGrid(device_points(p, device), max_dist)
        return g

    pairs = [(grid(p0), grid(p1), device_transform(T, device)) for p0, p1, T in items]
    out = results_to_host(*hip.icp_batch(pairs, max_dist, max_iter, tol_deg, tol_t))
    return out[0] if single else out
