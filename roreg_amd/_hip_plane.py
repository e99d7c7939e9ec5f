"""ctypes binding of the plane segmentation kernels (csrc/plane.hip; include/roreg_hip.h "v6t"): part of the `roreg_amd.hip` namespace (hip.py
re-exports everything here).  No reference counterpart; tests/_plane_oracle.py restates the definition in numpy."""
import math

import numpy as np
import torch

from .hip import _check, _ptr, _stream, lib

__all__ = ['PLANE_MAX_N', 'PLANE_MAX_HYP', 'PLANE_MAX_PLANES', 'PLANE_THREADS', 'PLANE_TILE', 'PLANE_HYP_CHUNK', 'plane_check_args', 'plane_score', 'plane_segment']

PLANE_MAX_N = 1 << 30                  # csrc/plane.hip PLANE_MAX_N
PLANE_MAX_HYP = 65536                  # == ROREG_PLANE_MAX_HYP
PLANE_MAX_PLANES = 64                  # == ROREG_PLANE_MAX_PLANES
PLANE_THREADS = 256                    # == ROREG_PLANE_THREADS: lanes of a scoring workgroup
PLANE_TILE = 1024                      # == ROREG_PLANE_TILE: live points a scoring workgroup keeps in registers
PLANE_HYP_CHUNK = 128                  # == ROREG_PLANE_HYP_CHUNK: hypothesis records it stages in LDS at a time


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _cloud(points, what):
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_cuda or not points.is_contiguous():
        raise ValueError(f'{what}: points must be a contiguous float32 [n,3] device tensor')
    n = int(points.shape[0])
    if n > PLANE_MAX_N:
        raise ValueError(f'{what}: {n} rows are more than the kernel numbers (2^30)')
    return n


def _dist(dist, what):
    ok = not isinstance(dist, (bool, str, bytes)) and isinstance(dist, (int, float, np.integer, np.floating))
    if not ok or not (float(dist) > 0.0 and math.isfinite(float(dist))):
        raise ValueError(f'{what}: dist must be a positive finite number, got {dist!r}')
    return float(dist)


def plane_check_args(dist, n_hyp, max_planes, min_inliers, seed, what='plane_segment'):
    """ValueError for what no cloud could make valid (no device call) -> (dist, n_hyp, max_planes, min_inliers, seed) as the kernel takes them."""
    dist = _dist(dist, what)
    if not _is_int(n_hyp) or not 1 <= int(n_hyp) <= PLANE_MAX_HYP:
        raise ValueError(f'{what}: n_hyp must be an integer in [1, {PLANE_MAX_HYP}], got {n_hyp!r}')
    if not _is_int(max_planes) or not 0 <= int(max_planes) <= PLANE_MAX_PLANES:
        raise ValueError(f'{what}: max_planes must be an integer in [0, {PLANE_MAX_PLANES}], got {max_planes!r}')
    if not _is_int(min_inliers) or not 3 <= int(min_inliers) < 2 ** 31:
        raise ValueError(f'{what}: min_inliers must be an integer >= 3, got {min_inliers!r}')
    if not _is_int(seed) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f'{what}: seed must be an integer in [0, 2^64), got {seed!r}')
    return dist, int(n_hyp), int(max_planes), int(min_inliers), int(seed)


def plane_score(points, triples, dist):
    """points float32 [n,3], triples int32 [H,3] (original rows), device tensors -> counts int32 [H] on the device: the number of non-dead rows
    within `dist` of the plane through each triple, as include/roreg_hip.h "v6t" defines the test (inclusive, float64, no square root); -1 for
    a triple with a repeated row, a row outside [0, n), a dead row or three collinear points.  Nothing is read back.  ValueError before any
    device call: a bad shape or dtype, dist not positive and finite, more than PLANE_MAX_HYP triples."""
    n = _cloud(points, 'plane_score')
    if (not isinstance(triples, torch.Tensor) or triples.dtype != torch.int32 or triples.dim() != 2 or triples.shape[1] != 3 or not triples.is_cuda
            or not triples.is_contiguous()):
        raise ValueError('plane_score: triples must be a contiguous int32 [H,3] device tensor')
    H = int(triples.shape[0])
    if H > PLANE_MAX_HYP:
        raise ValueError(f'plane_score: {H} triples are more than {PLANE_MAX_HYP}')
    dist = _dist(dist, 'plane_score')
    counts = torch.empty(H, dtype=torch.int32, device=points.device)
    if H:
        _check(lib().roreg_plane_score(_ptr(points) if n else None, n, _ptr(triples), H, dist, _ptr(counts), _stream()), 'roreg_plane_score')
    return counts


def plane_segment(points, dist, n_hyp=1024, max_planes=1, min_inliers=3, seed=0):
    """points float32 [n,3] device tensor -> (labels int32 [n], n_planes int32 [1], counts int32 [K], triples int32 [K,3], raw float64 [K,4],
    fit float64 [K,4], rms float64 [K]) device tensors, K = max_planes: RANSAC plane segmentation as include/roreg_hip.h "v6t" defines it.  Round
    r draws n_hyp triples of live rows, counts the live rows within `dist` of each plane, and gives the rows of the plane of greatest count
    (the lowest hypothesis among equals) label r, unless that count is below min_inliers, which ends the segmentation.  raw is the winning
    triple's unnormalised plane, fit the least-squares plane through its inliers (unit normal, offset), rms their root-mean-square distance to it.
    Behind n_planes: counts 0, triples -1, raw / fit / rms 0.  labels, n_planes, counts, triples and raw are the same bytes on every run.  Every
    round is enqueued at once; nothing is read back.  ValueError before any device call: a bad shape or dtype, dist not positive and finite,
    n_hyp outside [1, PLANE_MAX_HYP], max_planes outside [0, PLANE_MAX_PLANES], min_inliers < 3, seed outside [0, 2^64)."""
    n = _cloud(points, 'plane_segment')
    dist, H, K, min_inliers, seed = plane_check_args(dist, n_hyp, max_planes, min_inliers, seed)
    dev = points.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    n_planes = torch.empty(1, dtype=torch.int32, device=dev)
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    triples = torch.empty((K, 3), dtype=torch.int32, device=dev)
    raw, fit = (torch.empty((K, 4), dtype=torch.float64, device=dev) for _ in range(2))
    rms = torch.empty(K, dtype=torch.float64, device=dev)
    ws_n = lib().roreg_plane_workspace(n, H) if n >= 3 and K else 0
    ws = torch.empty(ws_n, dtype=torch.uint8, device=dev) if ws_n else None
    _check(lib().roreg_plane_segment(_ptr(points) if n else None, n, dist, H, K, min_inliers, seed, _ptr(labels) if n else None, _ptr(n_planes),
                                     _ptr(counts) if K else None, _ptr(triples) if K else None, _ptr(raw) if K else None, _ptr(fit) if K else None,
                                     _ptr(rms) if K else None, _ptr(ws), ws_n, _stream()), 'roreg_plane_segment')
    return labels, n_planes, counts, triples, raw, fit, rms
