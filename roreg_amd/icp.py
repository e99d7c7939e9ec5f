"""Dense ICP refinement of registered pairs on the device, point-to-point, point-to-plane or plane-to-plane (csrc/icp.hip; no reference counterpart: the
reference ends at the keypoint transform, and its users refine on the host with a k-d tree).

    from roreg_amd import icp
    res = icp.refine(points0, points1, T0, max_dist=0.07)            # one pair -> IcpResult
    res = icp.refine([(points0, points1, T0), ...], max_dist=0.07)   # many pairs, the same launches -> [IcpResult]
    res = icp.refine(points0, points1, T0, max_dist=0.07, method='plane')      # against the target's surface normals (radius 2 max_dist)
    res = icp.refine(points0, points1, T0, max_dist=0.07, method='gicp')       # generalized ICP: both clouds' normals weight every residual
    normals, valid, counts = icp.estimate_normals(points0, radius=0.14)
    res = icp.refine(points0, points1, T0, max_dist=0.07, voxel=0.025)         # both clouds voxel-grid downsampled on the device first
    res = icp.refine(points0, points1, T0, max_dist=0.15, method='plane', loss='tukey', loss_scale=0.03)   # robust: residuals beyond 3 cm get weight 0
    res = icp.refine(points0, points1, T0, max_dist=0.07, voxel=0.025, outliers=dict(kind='statistical', nb_neighbors=16, std_ratio=1.0))   # isolated points dropped first

points0 is the target (cloud 0), points1 the source (cloud 1), T0 [4,4] float64 in the engine's convention k0 ~ k1 R^T + t.  Coordinates are
rounded to float32 once, at upload; all arithmetic is float64.  RegistrationEngine.icp_many is the device-resident form (grids cached per
cloud, results left on the device)."""
from collections import namedtuple

import numpy as np
import torch

from . import hip
from . import outliers as outlier_filter
from . import voxel as voxel_grid

IcpResult = namedtuple('IcpResult', 'T iters inliers rmse status')
IcpResult.__doc__ = ('T [4,4] float64; iters: searches executed; inliers, rmse: of the last executed search (method=\'plane\': the correspondences '
                     'with a valid target normal and their root mean square plane residual; method=\'gicp\': the distance inliers n and '
                     'sqrt(sum d^T M d / n), the residual WHITENED by M = (C_q + R C_p R^T)^-1 -- not a distance: dense_eval gives the Euclidean figure); '
                     "status: 'converged' | 'max_iter' | 'no_support' (T0 kept) | 'nonfinite' (T0 returned unchanged).  Under a robust loss (loss=) inliers "
                     'and rmse are still the UNWEIGHTED count and root mean square of every correspondence inside the distance gate -- comparable across '
                     "losses, outliers included --, and 'no_support' is also what weights that are all zero (a scale far below the residuals) end in")
METHODS = ('point', 'plane', 'gicp')

TOL_DEG, TOL_T = 1e-4, 1e-6
GICP_EPSILON = 1e-3          # the covariance along the normal, relative to the two directions in the surface


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


def check_loss(method, loss, loss_scale, what='refine'):
    """The loss arguments of refine and RegistrationEngine.icp_many -> {} (no loss) or hip.icp_plane_batch's / hip.icp_gicp_batch's keywords."""
    if loss is None:
        if loss_scale is not None:
            raise ValueError(f'{what}: loss_scale without a loss')
        return {}
    if loss not in hip.ICP_LOSSES:
        raise ValueError(f'{what}: loss must be one of {hip.ICP_LOSSES} or None, got {loss!r}')
    if method not in ('plane', 'gicp'):
        raise ValueError(f"{what}: a loss needs method='plane' or 'gicp' (the weighted point-to-point fit is not built), got method={method!r}")
    if loss_scale is None or isinstance(loss_scale, (str, bytes)) or not (float(loss_scale) > 0.0 and np.isfinite(float(loss_scale))):
        raise ValueError(f'{what}: loss {loss!r} needs a positive, finite loss_scale (in the unit of the coordinates), got {loss_scale!r}')
    return dict(loss=loss, scale=float(loss_scale))


def run_batch(method, items, grid, normals, normal_radius, max_dist, *params, gicp_epsilon=GICP_EPSILON, loss=None, loss_scale=None):
    """The method dispatch of refine and RegistrationEngine.icp_many (`method` checked by the caller).  items [(target, source, T0 device
    tensor)]; grid(cloud) -> its IcpGrid; normals(cloud, radius) -> its normal table, radius 2 max_dist unless normal_radius says otherwise
    ('gicp' asks for the source's too; the callers' caches give a cloud that is a target here and a source there its table once);
    params: max_iter, tol_deg, tol_t -> the device tensors of hip.icp_batch / hip.icp_plane_batch / hip.icp_gicp_batch.  loss, loss_scale:
    a robust loss for every pair ('plane' and 'gicp' only; check_loss); without one the calls are what they were."""
    robust = check_loss(method, loss, loss_scale, 'icp')
    if method in ('plane', 'gicp'):
        radius = 2.0 * float(max_dist) if normal_radius is None else float(normal_radius)
    if method == 'gicp':
        return hip.icp_gicp_batch([(grid(a), grid(b), normals(a, radius), normals(b, radius), T, gicp_epsilon) for a, b, T in items], max_dist, *params, **robust)
    if method == 'plane':
        return hip.icp_plane_batch([(grid(a), grid(b), normals(a, radius), T) for a, b, T in items], max_dist, *params, **robust)
    return hip.icp_batch([(grid(a), grid(b), T) for a, b, T in items], max_dist, *params)


def estimate_normals(points, radius, min_neighbors=6, device='cuda', voxel=None, outliers=None):
    """Surface normals of a cloud [n,3] from the points within `radius` of each point -> (normals float64 [n,3], valid bool [n], counts
    int64 [n]) on the host; an invalid row (fewer than min_neighbors points in its ball, itself included, or a collinear ball) is zero.
    voxel=: the normals of the cloud downsampled to its voxel centroids (roreg_amd.voxel), and as a fourth value the lowest original row
    of every voxel (int32 [m]).  outliers=dict(kind='statistical' | 'radius' | 'cluster', ...) (roreg_amd.outliers): the cloud is filtered after the
    downsampling, the normals are those of the kept points, and the fourth value is the original row of every kept point (under voxel=: the
    lowest original row of its voxel)."""
    if voxel is not None:
        voxel_grid.check_args(voxel, what='estimate_normals')
    outliers = outlier_filter.check_args(outliers, 'estimate_normals')
    pts = device_points(points, device)
    if voxel is not None:
        pts, vd = voxel_grid.device_downsample(pts, voxel)
    rows = None if voxel is None else vd.first
    if outliers is not None:
        pts, kept = outlier_filter.device_apply(pts, outliers)
        rows = kept if rows is None else rows.index_select(0, kept)
    table = hip.icp_normals(hip.IcpGrid(pts, radius), radius, min_neighbors).cpu().numpy()
    normals = np.ascontiguousarray(table[:, :3])
    out = (normals, (normals != 0).any(1), table[:, 3].astype(np.int64))
    return out if rows is None else out + (rows.cpu().numpy(),)


def refine(points0, points1=None, T0=None, max_dist=None, max_iter=30, tol_deg=TOL_DEG, tol_t=TOL_T, device='cuda', method='point', normal_radius=None,
           min_neighbors=6, voxel=None, voxel_mode='centroid', gicp_epsilon=GICP_EPSILON, loss=None, loss_scale=None, outliers=None):
    """One pair (points0, points1, T0) -> IcpResult, or a list of such triples as the first argument -> [IcpResult].  An array that
    appears in several pairs (the same object) is uploaded and gridded once.  method='plane': point-to-plane against the target's normals,
    estimated once per distinct target array from the points within normal_radius (default 2 max_dist).  method='gicp': plane-to-plane
    (generalized ICP): the normals of both clouds, once per distinct array, give every point the covariance I - (1 - gicp_epsilon) n n^T and
    every residual the weight (C_q + R C_p R^T)^-1; rmse is then the whitened residual (IcpResult).  voxel=: every distinct array is
    voxel-grid downsampled once, where it is uploaded (voxel_mode 'centroid' or 'first', roreg_amd.voxel); grids and normals are built on
    the downsampled clouds, and inliers and rmse are the downsampled source's.  loss= ('huber', 'cauchy', 'gm', 'tukey': hip.ICP_LOSSES) with
    loss_scale=k (metres): iteratively re-weighted least squares under method 'plane' or 'gicp' -- inside the distance gate every
    correspondence enters the normal equations with the loss's weight of its residual / k (the plane residual; under 'gicp' sqrt(2 gicp_epsilon
    d^T M d), the same distance where the normals agree), so that geometry only one scan saw stops pulling the solution; inliers and rmse stay
    unweighted.  A loss with method='point', an unknown loss, a missing, non-positive or non-finite loss_scale: ValueError.
    outliers=dict(kind='statistical', nb_neighbors=, std_ratio=) or dict(kind='radius', radius=, min_neighbors=) (roreg_amd.outliers): every
    distinct array is filtered once, after voxel= and before its grid and normals are built; inliers and rmse are the kept source's."""
    if max_dist is None:
        raise ValueError('refine: max_dist is required')
    if method not in METHODS:
        raise ValueError(f'refine: method must be one of {METHODS}, got {method!r}')
    check_loss(method, loss, loss_scale)
    if voxel is not None:
        voxel_grid.check_args(voxel, voxel_mode, 'refine')
    outliers = outlier_filter.check_args(outliers, 'refine')
    single = points1 is not None
    items = [(points0, points1, T0)] if single else list(points0)
    grids = {}

    def grid(p):
        g = grids.get(id(p))
        if g is None:
            pts = device_points(p, device)
            if voxel is not None:
                pts = voxel_grid.device_downsample(pts, voxel, voxel_mode)[0]
            pts = outlier_filter.device_apply(pts, outliers)[0]
            g = grids[id(p)] = hip.IcpGrid(pts, max_dist)
        return g

    normals = {}

    def table(p, radius):
        t = normals.get(id(p))
        if t is None:
            t = normals[id(p)] = hip.icp_normals(grid(p), radius, min_neighbors)
        return t

    out = results_to_host(*run_batch(method, [(p0, p1, device_transform(T, device)) for p0, p1, T in items], grid, table, normal_radius, max_dist, max_iter,
                                     tol_deg, tol_t, gicp_epsilon=gicp_epsilon, loss=loss, loss_scale=loss_scale))
    return out[0] if single else out
