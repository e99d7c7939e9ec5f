"""Raw scans in, registrations out, in one process: the public front of the pipeline for clouds that have no feature files.

    from roreg_amd.register import Registrar
    reg = Registrar(engine, backbone)                        # a RegistrationEngine and the device FCGF network (backbone/fcgf.py, eval mode)
    r = reg.pair(points0, points1, seed=0)                   # -> PairResult: r.trans [4,4] f64 (k0 ~ k1 R^T + t), r.keypoints0 / r.keypoints1
    rs = reg.scene([pts_a, pts_b, pts_c], [(0, 1), (1, 2)], seed=0, icp=dict(max_dist=0.07))       # -> [PairResult], r.trans_icp refined

A cloud's group feature is computed from its points on the device (testset.GroupFeatureSource: the backbone on the 60 rotated copies, assembled
by hip.group_feature_assemble in the engine's storage type) when the engine's extractor asks for it, once per cloud, and never leaves the
device; everything behind it is RegistrationEngine.run_scene as the file-backed drivers call it.

Keypoints default to the reference's fallback (dataops/dataset.py get_kps): a shuffle of the cloud's row numbers, the first n_keypoints of it
(every row if the cloud has fewer).  With seed= they are drawn from a RandomState(seed) of the call's own, cloud after cloud in the order
given, and the pairs draw from per-pair streams derived from the seed (run_scene's pair_seeds): the call is then a function of its arguments
and leaves numpy's process-global generator alone.  Without a seed both use the global generator, as the reference does.
keypoint_method='farthest' takes the first n_keypoints rows of the cloud's farthest-point sampling from row 0 instead (roreg_amd/sample.py, on
the device, all clouds in one launch): keypoints that cover a raw scan evenly where the shuffle follows the sensor's density, and no random
numbers."""
import zlib

import numpy as np

from .testset import GroupFeatureSource


def draw_keypoint_rows(n_rows, n_keypoints=5000, rng=None):
    """get_kps's fallback: np.arange(n_rows) shuffled, cut to the first n_keypoints.  rng: a RandomState, or None = numpy's global generator."""
    rows = np.arange(int(n_rows))
    (np.random if rng is None else rng).shuffle(rows)
    return rows[0:int(n_keypoints)]


def pair_seeds(seed, pairs):
    """One generator seed per pair, a function of (seed, id0, id1) alone (the multi-GPU driver's rule, with an empty scene name)."""
    return [(int(seed) + zlib.crc32(f':{a}:{b}'.encode())) % (2 ** 32) for a, b in pairs]


KEYPOINT_METHODS = ('shuffle', 'farthest')


class Registrar:
    def __init__(self, engine, backbone, voxel_size=0.025, rot_batch=12, n_keypoints=5000, keypoint_method='shuffle'):
        if keypoint_method not in KEYPOINT_METHODS:
            raise ValueError(f'Registrar: keypoint_method must be one of {KEYPOINT_METHODS}, got {keypoint_method!r}')
        self.engine, self.backbone, self.keypoint_method = engine, backbone, keypoint_method
        self.voxel_size, self.rot_batch, self.n_keypoints = float(voxel_size), int(rot_batch), int(n_keypoints)

    def keypoints_of(self, clouds, keypoints=None, seed=None):
        """clouds [[n,3]]; keypoints: None, or per cloud None / an [N,3] array that bypasses the draw -> [keypoints [N,3] float64]."""
        rng = None if seed is None else np.random.RandomState(int(seed))
        out = []
        sampled = {}
        if self.keypoint_method == 'farthest':
            from . import sample
            todo = [q for q in range(len(clouds)) if keypoints is None or keypoints[q] is None]
            res = sample.farthest_many([np.asarray(clouds[q]) for q in todo], self.n_keypoints)
            sampled = {q: r.rows.cpu().numpy() for q, r in zip(todo, res)}
        for q, pts in enumerate(clouds):
            given = None if keypoints is None else keypoints[q]
            if given is not None:
                out.append(np.asarray(given, np.float64).reshape(-1, 3))
            elif q in sampled:
                out.append(np.asarray(np.asarray(pts)[sampled[q]], np.float64))
            else:
                pts = np.asarray(pts)
                out.append(np.asarray(pts[draw_keypoint_rows(pts.shape[0], self.n_keypoints, rng)], np.float64))
        return out

    def source(self, clouds, keypoints, keep_points=False):
        return GroupFeatureSource(self.backbone, lambda i: clouds[i], lambda i: keypoints[i], self.voxel_size, self.rot_batch,
                                  self.engine.feat_dtype, keep_points=keep_points, ids=range(len(clouds)))

    def scene(self, clouds, pairs, keypoints=None, seed=None, icp=None, **run_kw):
        """clouds: a list of [n,3] arrays; pairs: [(i, j)] indices into it (cloud i the target, j the source) -> [PairResult] in pair order, each
        with keypoints0 / keypoints1 (the keypoints used) and, with icp=dict(RegistrationEngine.icp_many's arguments), trans_icp and its fields.
        run_kw: further keyword arguments of run_scene (keynum, max_iter, keep_matches, ...)."""
        kps = self.keypoints_of(clouds, keypoints, seed)
        pair_ids = [(str(int(a)), str(int(b))) for a, b in pairs]
        src = self.source(clouds, kps, keep_points=icp is not None)
        if seed is not None:
            run_kw.setdefault('pair_seeds', pair_seeds(seed, pair_ids))
        if icp is not None:
            run_kw.update(points=src, icp=dict(icp))
        res = self.engine.run_scene(src, dict(enumerate(kps)), pair_ids, **run_kw)
        for r in res:
            r.keypoints0, r.keypoints1 = kps[int(r.id0)], kps[int(r.id1)]
        self.last_source = src
        return res

    def pair(self, points0, points1, keypoints0=None, keypoints1=None, seed=None, icp=None, **run_kw):
        """points0 the target, points1 the source -> PairResult (trans maps cloud 1 onto cloud 0)."""
        return self.scene([points0, points1], [(0, 1)], [keypoints0, keypoints1], seed, icp, **run_kw)[0]
