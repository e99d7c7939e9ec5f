"""Row N3 of the scope table: the step immediately upstream of the path -- assembling the [N,32,60] group feature of a cloud's
keypoints from a point-wise backbone evaluated on the 60 icosahedrally rotated copies of the cloud (testset.py:124-181).

The point-wise backbone is a plug-in:

    backbone(xyz [n,3] float32 ndarray) -> (xyz_down [m,3] float32, feats [m,F] float32)     (host arrays or device tensors)

The reference's own backbone, the sparse-conv FCGF network, runs on the device here (roreg_amd/backbone/fcgf.py): FCGFBackbone(model,
voxel_size) wraps it as such a plug-in, one rotation per call, and extract_group_features runs `rot_batch` rotations as one sparse tensor.
    python -m roreg_amd.testset --dataset D --model CKPT --voxel_size V       mirrors the reference's testset.py for a dataset directory.
group_features_device is extract_group_features left on the device (assembled by hip.group_feature_assemble, float32 or bfloat16, no download);
GroupFeatureSource serves it lazily as the engine's `feats` (roreg_amd/register.py, run_distributed --from_points).

For every group element g the cloud and its keypoints are rotated by R_g, the backbone runs on the rotated cloud, and each
rotated keypoint takes the feature of its nearest down-sampled point (knn_module.KNN(1), testset.py:170-172) -- that lookup is
roreg_nn_search with F=3.  Output layout = the hot path's input contract: float32 [N, F, 60], group index fastest."""
import numpy as np
import torch

from . import hip
from .group import tables
from .utils.utils import make_non_exists_dir


def assemble_group_features(backbone, points, keypoints, group_dir=None):
    """points [n,3], keypoints [N,3] (float64 like dataset.get_pc / get_kps) -> float32 [N,F,60] (host ndarray)."""
    T = tables(group_dir)
    pts = np.asarray(points, np.float64)
    kps = np.asarray(keypoints, np.float64)
    # the 60 rotated keypoint sets in ONE upload (host float64 products rounded to float32 exactly as testset.py:80-81 does; 3.6 MB at 5000
    # keypoints); the group feature is assembled in place on the device and downloaded once
    kps_all = hip.upload(np.stack([(kps @ T.R[g].T).astype(np.float32) for g in range(60)]))            # [60,N,3]
    out = None
    for g in range(60):
        xyz_g = (pts @ T.R[g].T).astype(np.float32)                      # testset.py:43
        xyz_down, feats = backbone(xyz_g)                                 # the plug-in decides where its outputs live; device tensors are used as they are
        xyz_down = torch.as_tensor(xyz_down, dtype=torch.float32).to('cuda', non_blocking=True).contiguous()
        feats = torch.as_tensor(feats, dtype=torch.float32).to('cuda', non_blocking=True)
        if out is None:
            out = torch.empty((kps.shape[0], feats.shape[1], 60), dtype=torch.float32, device='cuda')
        nn = hip.nn_search(kps_all[g], xyz_down)                          # nearest down-sampled point of every keypoint (KNN(1), testset.py:170-172)
        out[:, :, g] = feats[nn]                                          # [N,F] into group column g
    return out.cpu().numpy()                                              # [N,F,60]


def _voxelise(xyz_g, voxel_size):
    """One rotated cloud (host float32 [n,3]) -> (xyz_down [m,3] = the lowest original row of every voxel, in ascending row; coords int32 [m,3] =
    floor(x / voxel)) on the device: testset.py:45-53's sparse_quantize(xyz / voxel, return_index=True) and np.floor(xyz / voxel)."""
    from . import voxel
    xyz_down, vd = voxel.device_downsample(hip.upload(np.ascontiguousarray(xyz_g, np.float32)), voxel_size, mode='first')
    return xyz_down, vd.coords


def _batch_coords(coords_list):
    """Per-item coords int32 [m_i,3] -> (int32 [sum m_i, 4] rows (item, x, y, z), cuts int32 [items + 1] on the host)."""
    cuts = np.concatenate([[0], np.cumsum([int(c.shape[0]) for c in coords_list])]).astype(np.int32)
    rows = [torch.cat([torch.full((int(c.shape[0]), 1), i, dtype=torch.int32, device=c.device), c], 1) for i, c in enumerate(coords_list)]
    return torch.cat(rows, 0).contiguous(), cuts


class FCGFBackbone:
    """The device FCGF network (roreg_amd.backbone.fcgf.ResUNetBN2C, on the device, in eval mode) as a plug-in backbone: one rotation per call."""

    def __init__(self, model, voxel_size=0.025):
        self.model, self.voxel_size = model, float(voxel_size)

    def __call__(self, xyz):
        xyz_down, coords = _voxelise(xyz, self.voxel_size)
        c4, cuts = _batch_coords([coords])
        return xyz_down, self.model(c4, cuts)


def _rotation_batches(model, points, keypoints, voxel_size, rot_batch, group_dir):
    """The body extract_group_features and group_features_device share: per batch of `rot_batch` rotations (the last one may be short)
    -> (g0, feats float32 [M,F] on the device, cuts int32 [R + 1] on the host, [nn int64 [N] per rotation: the item-local nearest down-sampled
    row of every keypoint]).  The rotations are host float64 products rounded to float32, exactly as assemble_group_features."""
    T = tables(group_dir)
    pts = np.asarray(points, np.float64)
    kps = np.asarray(keypoints, np.float64)
    rot_batch = max(1, min(60, int(rot_batch)))
    kps_all = hip.upload(np.stack([(kps @ T.R[g].T).astype(np.float32) for g in range(60)]))            # [60,N,3]
    for g0 in range(0, 60, rot_batch):
        gs = range(g0, min(60, g0 + rot_batch))
        vox = [_voxelise((pts @ T.R[g].T).astype(np.float32), voxel_size) for g in gs]                 # host rotation exactly as assemble_group_features
        c4, cuts = _batch_coords([c for _, c in vox])
        feats = model(c4, cuts)
        yield g0, feats, cuts, [hip.nn_search(kps_all[g], vox[i][0]) for i, g in enumerate(gs)]


def extract_group_features(model, points, keypoints, voxel_size=0.025, rot_batch=12, group_dir=None):
    """assemble_group_features(FCGFBackbone(model, voxel_size), points, keypoints) with `rot_batch` rotations run through the network as one
    sparse tensor (one item per rotation): the same [N,F,60] array bit for bit, since an item's features do not depend on its batch."""
    out = None
    for g0, feats, cuts, nns in _rotation_batches(model, points, keypoints, voxel_size, rot_batch, group_dir):
        if out is None:
            out = torch.empty((int(nns[0].shape[0]), feats.shape[1], 60), dtype=torch.float32, device='cuda')
        for i, nn in enumerate(nns):
            out[:, :, g0 + i] = feats[int(cuts[i]):int(cuts[i + 1])][nn]
    return out.cpu().numpy()


def group_features_device(model, points, keypoints, voxel_size=0.025, rot_batch=12, dtype=torch.float32, group_dir=None):
    """extract_group_features left on the device: the [N,F,60] group feature as a device tensor, float32 (the bits of extract_group_features) or
    bfloat16 (those bits rounded to nearest even: the engine's other storage type), written once -- one hip.group_feature_assemble launch per
    batch of rotations instead of an indexed gather and a strided scatter per rotation, and no download."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f'group_features_device: dtype must be torch.float32 or torch.bfloat16, got {dtype}')
    out = info = None
    for g0, feats, cuts, nns in _rotation_batches(model, points, keypoints, voxel_size, rot_batch, group_dir):
        if out is None:
            out = torch.empty((int(nns[0].shape[0]), feats.shape[1], 60), dtype=dtype, device=feats.device)
            info = torch.zeros(1, dtype=torch.int32, device=feats.device)
        hip.group_feature_assemble(feats, hip.upload(cuts), torch.stack(nns), g0, out, info=info)
    hip.check_group_feature_info(info)                                    # (one read-back per cloud, behind the last batch)
    return out


class GroupFeatureSource:
    """{cloud id: [N,F,60] device tensor} computed from raw points when asked: the `feats` of RegistrationEngine.run_scene / distributed.run_plan
    for clouds that have no feature files.  source[i] runs group_features_device on get_points(i) / get_keypoints(i) (both called with the int
    cloud id) and counts the run in source.runs[i]; the engine asks for a cloud once per extraction and keeps what it got, so nothing is held here.
    dtype: the engine's storage type (engine.feat_dtype) lets extract_many take the tensor as it is; float32 is converted there to the same bits.
    rows(i) / like(i) give a cloud's row count / a storage-less stand-in of its feature without running the network (the keypoints are read
    once and kept: they are small).  keep_points=True: the source also serves as run_scene's `points=` -- a cloud's points, read for its
    feature, are kept until get(i) hands them to the ICP stage (read once, not once per consumer).  on_feature(i, tensor), optional, sees every
    computed feature (the driver's --save_group_features).  `computed` tells distributed.run_plan that source[i] is expensive: a cut scene's
    receivers then get `before` shipped beside `eqv` instead of evaluating source[i] again."""
    computed = True

    def __init__(self, model, get_points, get_keypoints, voxel_size=0.025, rot_batch=12, dtype=torch.float32, group_dir=None, keep_points=False,
                 on_feature=None, ids=None):
        self.model, self.get_points, self.get_keypoints = model, get_points, get_keypoints
        self.voxel_size, self.rot_batch, self.dtype, self.group_dir = float(voxel_size), int(rot_batch), dtype, group_dir
        self.keep_points, self.on_feature = bool(keep_points), on_feature
        self.ids = None if ids is None else {int(i) for i in ids}
        self.runs = {}                                                    # cloud id -> backbone runs (60 rotations each)
        self._kps, self._pts = {}, {}

    def __contains__(self, i):
        return self.ids is None or int(i) in self.ids

    def keypoints(self, i):
        i = int(i)
        if i not in self._kps:
            self._kps[i] = np.asarray(self.get_keypoints(i))
        return self._kps[i]

    def rows(self, i):
        return int(self.keypoints(i).shape[0])

    def like(self, i, channels=32):
        return torch.empty((self.rows(i), channels, 60), dtype=self.dtype, device='meta')

    def __getitem__(self, i):
        i = int(i)
        if i not in self:
            raise KeyError(i)
        pts = self._pts.pop(i) if i in self._pts else np.asarray(self.get_points(i))
        if self.keep_points:
            self._pts[i] = pts
        f = group_features_device(self.model, pts, self.keypoints(i), self.voxel_size, self.rot_batch, self.dtype, self.group_dir)
        self.runs[i] = self.runs.get(i, 0) + 1
        if self.on_feature is not None:
            self.on_feature(i, f)
        return f

    def get(self, i, default=None):
        """The dense points of cloud i (run_scene's `points=` mapping; int ids only, so that `points.get(i, points.get(str(i)))` reads once)."""
        if isinstance(i, str) or i not in self:
            return default
        i = int(i)
        return self._pts.pop(i) if i in self._pts else np.asarray(self.get_points(i))


def write_group_features(backbone, dataset, output_cache_fn, backbone_name='FCGF', group_dir=None, voxel_size=0.025, rot_batch=12):
    """Writes {output_cache_fn}/{dataset.name}/{backbone}_Input_Group_feature/{pc}.npy for every cloud of a scene.  backbone: a plug-in callable,
    or the device FCGF network itself (a torch module: the batched path, with voxel_size and rot_batch)."""
    out = f'{output_cache_fn}/{dataset.name}/{backbone_name}_Input_Group_feature'
    make_non_exists_dir(out)
    for pc_id in dataset.pc_ids:
        if isinstance(backbone, torch.nn.Module):
            f = extract_group_features(backbone, dataset.get_pc(pc_id), dataset.get_kps(pc_id), voxel_size, rot_batch, group_dir)
        else:
            f = assemble_group_features(backbone, dataset.get_pc(pc_id), dataset.get_kps(pc_id), group_dir)
        np.save(f'{out}/{pc_id}.npy', f)


def main(argv=None):
    """The reference's testset.py for a dataset directory: FCGF group features of every cloud of every scene, under
    {outdir}/{dataset}/{scene}/FCGF_Input_Group_feature/{pc}.npy."""
    import argparse
    from .backbone import fcgf
    from .dataops.dataset import get_dataset_name
    basedir = './data'
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument('--model', default='./checkpoints/FCGF/backbone/best_val_checkpoint.pth', help='FCGF checkpoint (config + state_dict)')
    ap.add_argument('--outdir', default=f'{basedir}/YOHO_FCGF/Testset')
    ap.add_argument('--voxel_size', default=0.025, type=float)
    ap.add_argument('--dataset', default='demo')
    ap.add_argument('--datadir', default=f'{basedir}/origin_data')
    ap.add_argument('--groupdir', default=None, help='group tables (default: the packaged ones)')
    ap.add_argument('--rot_batch', default=12, type=int, help='rotations per sparse tensor')
    args = ap.parse_args(argv)
    model = fcgf.from_checkpoint(args.model)
    for scene, dataset in get_dataset_name(args.dataset, args.datadir).items():
        if scene in ('wholesetname', 'valscenes'):
            continue
        write_group_features(model, dataset, args.outdir, 'FCGF', args.groupdir,       # dataset.name = '{dataset}/{scene}'
 args.voxel_size, args.rot_batch)


if __name__ == '__main__':
    main()
