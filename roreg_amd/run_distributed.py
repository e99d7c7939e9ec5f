"""Multi-GPU evaluation driver: one process per GPU, scan pairs sharded by scene, ONE gather of the result table.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 -m roreg_amd.run_distributed \
           --testset 3dmatch --ET yohoo|yohoc|sc2 [--sc2_tau 0.1] [--sc2_k 20] --keynum 5000 [--RD] [--RM] [--seed 0] [--icp [--icp_dist 0.07] [--icp_iter 30] [--icp_method point|plane|gicp] [--icp_normal_radius 0.14] [--icp_gicp_epsilon 1e-3] [--icp_loss tukey --icp_loss_scale 0.03]
           [--icp_voxel 0.025 [--icp_voxel_mode centroid|first]] [--icp_outlier_nb 16 --icp_outlier_std 1.0 | --icp_outlier_radius 0.1 --icp_outlier_min 8 |
            --icp_outlier_cluster_eps 0.08 --icp_outlier_cluster_min_size 100 [--icp_outlier_cluster_min_points 6]]]
           [--gt_info_dist 0.05 [--gt_info_voxel 0.025]]
           [--from_points --backbone_model CKPT [--voxel_size 0.025] [--rot_batch 12] [--save_group_features]]

Every rank builds the same shard plan (roreg_amd.distributed.shard_scenes), extracts only the clouds its pair ranges touch,
registers its pairs with the device-resident engine, computes the per-pair inlier ratio locally, and contributes fixed-width
float64 rows to one all_gather (backend nccl = RCCL over xGMI).  Rank 0 then writes the reference's result files
({ET}/{iters}iters/*.npz, pre.log) and computes FMR / IR / RR(pointdsc) / RR(predator) like test/evaluator.py:103-145.
With --seed every pair draws from its own generator stream (seed + crc32(scene, id0, id1)), and every block scale of the kernels is per
keypoint / per correspondence, so a pair's result is a function of the pair alone: the result table does not depend on the number of
ranks nor on how the shard plan cuts the scenes (tested at world size 1 vs 2).
--ET sc2 estimates every pair from its matched keypoints alone (spatial-compatibility hypotheses on the device, roreg_amd/sc2.py): no ET
checkpoint is loaded and no hypothesis is drawn; --sc2_tau is the compatibility threshold (default --ransac_ird), --sc2_k the consensus set size.
With --icp every rank also reads the dense clouds of its pairs (dataset.get_pc) and refines each pair's transform by point-to-point ICP on
the device (roreg_amd/icp.py; no reference counterpart).  A second table of the same row layout is gathered -- trans = the refined transform,
the n_match slot = ICP inliers, the recalltime slot = ICP iterations, the inlier-ratio slot = ICP rmse -- and rank 0 writes
{ET}_icp/{iters}iters/*.npz + pre.log and a second block, labelled ...-icp, to results.log.  Everything else is what it is without the flag.
--icp_method plane refines point-to-plane against the target's surface normals (estimated on the device from the points within
--icp_normal_radius, default twice the correspondence distance); its files go to {ET}_icp_plane/ and its block is labelled ...-icp-plane.
--icp_method gicp refines plane-to-plane (generalized ICP: both clouds' normals, --icp_gicp_epsilon the covariance along the normal); its files
go to {ET}_icp_gicp/ and its block is labelled ...-icp-gicp.
--icp_loss huber|cauchy|gm|tukey --icp_loss_scale K (with --icp_method plane or gicp only; refused otherwise) weights every correspondence inside
the distance gate by the loss's weight of its residual / K (roreg_amd/icp.py refine); folder and label then end in the loss and its scale,
e.g. {ET}_icp_plane_tukey0.03/ and ...-icp-plane-tukey0.03, so that runs under different losses do not overwrite each other.
--icp_voxel V downsamples every dense cloud to its voxel grid on the device as it is attached (roreg_amd/voxel.py; --icp_voxel_mode first keeps
the lowest original row of every voxel instead of the centroid); directories and labels stay, the results.log block names the voxel.
--icp_outlier_nb K --icp_outlier_std S (statistical) or --icp_outlier_radius R --icp_outlier_min N (radius) drop isolated points of every dense
cloud after that (roreg_amd/outliers.py); --icp_outlier_cluster_eps E --icp_outlier_cluster_min_size S [--icp_outlier_cluster_min_points P] is the
third filter: DBSCAN clusters of fewer than S points, and noise, are dropped (floating fragments the first two keep).  One filter at a time;
directories and labels stay, the results.log block names the filter.
--gt_info_dist D: for every scene that has a gt.log but no gt.info (and whose dataset has get_pc) rank 0 evaluates every gt.log pair's dense
clouds under the ground truth on the device (roreg_amd/dense_eval.py; correspondences within D, clouds voxel-downsampled first with
--gt_info_voxel V), writes the information matrices to {output_cache_fn}/{scene}/gt_info_{D:g}.info and computes RR(predator) from them.
It never writes into the dataset directory and never replaces an existing gt.info; without the flag nothing changes.
--from_points: the scenes need no {backbone}_Input_Group_feature files.  Every cloud's group feature is computed from its raw points
(dataset.get_pc, dataset.get_kps) by the FCGF network of --backbone_model on the device when the extractor asks for it, stays there in the
engine's storage type, and is computed once per cloud in the whole job: a cut scene's owner ships `before` beside `eqv`.  The result files
are those of the file-backed run on the features python -m roreg_amd.testset writes; --save_group_features writes those files too."""
from types import SimpleNamespace

import os
import zlib

import numpy as np
import torch

from . import distributed as D
from .utils import RR_cal
from .utils.r_eval import compute_R_diff
from .utils.utils import make_non_exists_dir, transform_points, load_checkpoint
from .test.estimator import pre_log_entry


# --from_points: a cloud through the backbone and the extractor against a pair through matcher and estimator, in the shard plan's pair-units
# (profiles/raw_scene_timing.txt, tools/time_raw_scene.py: seconds per cloud / seconds per pair; it shapes the plan, never a result)
RAW_CLOUD_COST = 450.0


def build_engine(cfg):
    from .engine import RegistrationEngine
    from .network import name2network

    def load(kind, sub, strict=True):
        net = name2network[kind](cfg)
        fn = f'{cfg.model_fn}/{sub}/model_best.pth'
        if not os.path.exists(fn):
            raise ValueError("No model exists")
        net.load_state_dict(load_checkpoint(fn)['network_state_dict'], strict=strict)
        return net.eval()
    gf = load('GF_test', 'GF')
    et = load('ET_test', 'ET', strict=False) if cfg.ET == 'yohoo' else None     # yohoc never evaluates the ET network (estimator.py:266-272), sc2 has no use for it
    rd = load('RD_test', 'RD') if cfg.RD else None
    rm = load('RM_test', 'RM') if cfg.RM else None
    return RegistrationEngine(cfg, gf, et, rd_net=rd, rm_net=rm)


def _feature_dir(cfg, dataset):
    name = f'3d{dataset.name[4:]}' if dataset.name[0:4] == '3dLo' else dataset.name
    return f'{cfg.output_cache_fn}/{name}/{cfg.backbone}_Input_Group_feature'


def inlier_ratio(cfg, result, keys0, keys1, gt):
    """Inlier ratio of a pair's (top-scored) correspondences under the ground truth, test/evaluator.py:50-81 (host numpy, float64)."""
    corr = result.matches.cpu().numpy() if torch.is_tensor(result.matches) else np.asarray(result.matches)
    if corr.shape[0] == 0:
        return 0.0
    if cfg.RM and result.scores is not None:
        num = max(result.scores.shape[0] * cfg.match_n, 10) if cfg.match_n < 0.999 else cfg.match_n
        corr = corr[np.argsort(result.scores)[-int(num):]]
    k0 = keys0[corr[:, 0]]; k1 = transform_points(keys1[corr[:, 1]], gt)
    return float(np.mean(np.sqrt(np.sum(np.square(k0 - k1), axis=-1)) < cfg.tau_2))


def scene_metrics(cfg, rows, gt_of):
    """rows: [{'id0','id1','trans','ir'}] of ONE scene in pair-list order; gt_of(id0, id1) -> [3,4] or [4,4] ground truth.
    -> (FMR, IR, RR(pointdsc), mean RRE, mean RTE of the successes) exactly as test/evaluator.py:50-101,111-129."""
    ir_s, ok_s, re_s, te_s = [], [], [], []
    for row in rows:
        T = row['trans']; gt = gt_of(row['id0'], row['id1'])
        ir_s.append(row['ir'])
        if np.isfinite(T).all():
            rd = compute_R_diff(T[0:3, 0:3], gt[0:3, 0:3]); td = np.sqrt(np.sum(np.square(T[0:3, -1] - gt[0:3, -1])))
            good = bool(rd < 15 and td < 0.3)
        else:
            good = False
        ok_s.append(1 if good else 0)
        if good:
            re_s.append(rd); te_s.append(td)
    return (float(np.mean([1 if i > cfg.tau_1 else 0 for i in ir_s])), float(np.mean(ir_s)), float(np.mean(ok_s)),
            float(np.mean(re_s)) if re_s else float('nan'), float(np.mean(te_s)) if te_s else float('nan'))


def _gt_stem(ds):
    return ds.gt_dir[:ds.gt_dir.rfind('.')]


def write_gt_info(cfg, datasets, scenes, max_dist, voxel=None):
    """For every scene with a gt.log, without a gt.info and with dense clouds (get_pc): the information matrix of every gt.log pair under
    ds.get_transform, in gt.log order, to {output_cache_fn}/{scene}/gt_info_{max_dist:g}.info -> {scene name: path}."""
    from . import dense_eval
    out = {}
    for s in scenes:
        ds = datasets[s]
        stem = _gt_stem(ds)
        if os.path.exists(f'{stem}.info') or not os.path.exists(f'{stem}.log') or not hasattr(ds, 'get_pc'):
            continue
        gt_pairs, _ = RR_cal.read_trajectory(f'{stem}.log')
        clouds = {}

        def cloud(i):
            if i not in clouds:
                clouds[i] = np.asarray(ds.get_pc(str(i)))
            return clouds[i]

        items = []
        for i, j, _ in gt_pairs:
            T = np.eye(4); T[:3] = np.asarray(ds.get_transform(str(i), str(j)), np.float64)[:3]
            items.append((cloud(int(i)), cloud(int(j)), T))
        res = dense_eval.evaluate(items, max_dist=max_dist, voxel=voxel)
        path = f'{cfg.output_cache_fn}/{ds.name}/gt_info_{max_dist:g}.info'
        make_non_exists_dir(os.path.dirname(path))
        RR_cal.write_trajectory_info(path, [(int(i), int(j)) for i, j, _ in gt_pairs], int(gt_pairs[0][2]) if len(gt_pairs) else len(ds.pc_ids),
                                     [r.info for r in res])
        out[ds.name] = path
    return out


def write_trajectory(path, ids, poses):
    """A Redwood .log of world poses: per cloud the header 'id id n_clouds' and the four rows of its pose, every entry with 17 significant
    digits, so that RR_cal.read_trajectory returns the float64 bits it was given."""
    with open(path, 'w') as f:
        for c, P in zip(ids, np.asarray(poses, np.float64).reshape(-1, 4, 4)):
            f.write(f'{int(c)}\t{int(c)}\t{len(ids)}\n')
            for row in P:
                f.write('\t'.join('%.17g' % v for v in row) + '\n')


def multiway_poses(cfg, datasets, scenes, engine, by_scene, max_dist, tau=None):
    """For every scene with dense clouds (get_pc): the scene's pose graph -- one edge per pair of the result table with a finite transform,
    weighted by the pair's information matrix within max_dist -- optimised on the device (RegistrationEngine.optimize_poses), anchored at
    the scene's first cloud; the poses go to {output_cache_fn}/{scene}/multiway_poses.log -> {scene key: (path, PoseGraphResult, rows)},
    rows = the scene's result rows in pair-list order with 'trans' replaced by the transform the poses imply (an unreached cloud: NaN)."""
    from .engine import CloudState
    from . import pose_graph
    out = {}
    for s in scenes:
        ds = datasets[s]
        if not hasattr(ds, 'get_pc'):
            continue
        ids = [int(c) for c in ds.pc_ids]
        pos = {c: k for k, c in enumerate(ids)}
        rows = [by_scene[s][p] for p in ds.pair_ids]
        edges = [(pos[int(r['id0'])], pos[int(r['id1'])]) for r in rows if np.isfinite(r['trans']).all()]
        T = [r['trans'] for r in rows if np.isfinite(r['trans']).all()]
        clouds = [engine.attach_points(CloudState(before=None), np.asarray(ds.get_pc(str(c)))) for c in ids]
        res = engine.optimize_poses(clouds, edges, np.stack(T) if T else np.zeros((0, 4, 4)), max_dist, anchor=0, robust_tau=tau)
        path = f'{cfg.output_cache_fn}/{ds.name}/multiway_poses.log'
        make_non_exists_dir(os.path.dirname(path))
        write_trajectory(path, ids, res.poses)
        implied = pose_graph.implied_pairs(res.poses, [(pos[int(r['id0'])], pos[int(r['id1'])]) for r in rows])
        new_rows = []
        for r, Tij in zip(rows, implied):
            ok = res.reached[pos[int(r['id0'])]] and res.reached[pos[int(r['id1'])]] and res.status != 'nonfinite'
            new_rows.append(dict(r, trans=Tij if ok else np.full((4, 4), np.nan)))
        out[s] = (path, res, new_rows)
    return out


def evaluate(cfg, datasets, engine, rank=0, world=1, seed=None, exchange=True, icp=None, gt_info=None, multiway=None, raw=None):
    """icp: None, or a dict of RegistrationEngine.icp_many's keyword arguments (max_dist, max_iter, method, normal_radius, gicp_epsilon, loss, loss_scale): refine every pair
    on its dense clouds (plus, optionally, voxel / voxel_mode and outliers: what attach_points does to every dense cloud first).  gt_info: None, or dict(max_dist=, voxel=None): rank 0 computes the information matrices of the scenes that have no
    gt.info (write_gt_info) and RR(predator) from them.  multiway: None, or dict(max_dist=, tau=None): rank 0 optimises every scene's pose
    graph after the table's all-gather (multiway_poses) and reports the recall of the implied pair transforms beside the pairwise one.
    raw: None, or dict(model=the device FCGF network, voxel_size=0.025, rot_batch=12, save=False, cloud_cost=RAW_CLOUD_COST) (--from_points): no
    feature files are read -- every cloud's group feature is computed from ds.get_pc / ds.get_kps on the device when the extractor asks for
    it (testset.GroupFeatureSource), once per cloud in the whole job; save=True also writes it where the file-backed run would read it
    (the testset CLI's bytes).  cloud_cost prices a cloud against a pair in the shard plan and shapes nothing but the plan."""
    scenes = [s for s in datasets if s not in ('wholesetname', 'valscenes')]
    pair_counts = {s: len(datasets[s].pair_ids) for s in scenes}
    cloud_counts = {s: len(datasets[s].pc_ids) for s in scenes}
    pair_lists = {s: datasets[s].pair_ids for s in scenes}
    exchange = bool(exchange and world > 1 and hasattr(engine, 'cloud_from_eqv'))
    plan = D.shard_scenes(pair_counts, world, cloud_counts, pair_lists=pair_lists, exchange=exchange,
                          **({} if raw is None else {'cloud_cost': float(raw.get('cloud_cost', RAW_CLOUD_COST))}))
    transfers = D.exchange_plan(plan, pair_lists)[1] if exchange else []
    inputs = {}

    class LazyFeats:
        """{cloud id: [N,32,60] float32} of one scene, memory-mapped on access and never held: a cloud's file is read when the engine uploads it
        (once per extraction), under the kernels of the scenes already in flight; the host keeps no copy (the page cache does)."""

        def __init__(self, fdir, used):
            self.fdir, self.used = fdir, set(used)

        def __getitem__(self, i):
            if int(i) not in self.used:
                raise KeyError(i)
            return np.load(f'{self.fdir}/{int(i)}.npy', mmap_mode='r')

        def __contains__(self, i):
            return int(i) in self.used

    class LazyPoints:
        """{cloud id: [n,3]} of one scene's dense clouds, read when the engine first attaches a cloud's points (once per cloud and rank)."""

        def __init__(self, ds):
            self.ds = ds

        def get(self, i, default=None):
            return self.ds.get_pc(str(int(i)))

    writers = []

    def raw_source(ds, used):
        """The scene's features from its raw clouds; float32 when they are also written (the files hold float32 whatever the storage type)."""
        from .testset import GroupFeatureSource
        on_feature = None
        if raw.get('save'):
            from .engine import StageFileWriter
            fdir = _feature_dir(cfg, ds)
            make_non_exists_dir(fdir)
            writers.append(StageFileWriter(cfg, ds.name, cfg.keynum))
            on_feature = lambda i, f, w=writers[-1]: w.save_path(f'{fdir}/{i}.npy', f)
        return GroupFeatureSource(raw['model'], lambda i: ds.get_pc(str(i)), lambda i: ds.get_kps(str(i)), raw.get('voxel_size', 0.025),
                                  raw.get('rot_batch', 12), torch.float32 if raw.get('save') else engine.feat_dtype, keep_points=icp is not None,
                                  on_feature=on_feature, ids=used)

    def scene_inputs(scene):
        """(feats, keys, pair_ids, seeds) of a scene: keypoints (small) are read once, input features stay on disk until they are uploaded"""
        if scene not in inputs:
            ds = datasets[scene]
            used = sorted({int(i) for sc, a, b in plan[rank] if sc == scene for p in ds.pair_ids[a:b] for i in p} |
                          {i for sc, i, src, dst in transfers if sc == scene and rank in (src, dst)})
            seeds = None if seed is None else [(int(seed) + zlib.crc32(f'{scene}:{p0}:{p1}'.encode())) % (2 ** 32) for p0, p1 in ds.pair_ids]
            if raw is not None:
                feats = raw_source(ds, used)
                inputs[scene] = (feats, {i: feats.keypoints(i) for i in used}, ds.pair_ids, seeds)
            else:
                inputs[scene] = (LazyFeats(_feature_dir(cfg, ds), used), {i: ds.get_kps(str(i)) for i in used}, ds.pair_ids, seeds)
            if icp is not None:
                inputs[scene] += ({'points': inputs[scene][0] if raw is not None else LazyPoints(ds), 'icp': dict(icp)},)
        return inputs[scene]

    rows, rows_icp = [], []
    for scene, a, b, res in D.run_plan(engine, plan[rank], scene_inputs, transfers, rank, seeded=seed is not None,
                                       keynum=cfg.keynum, max_iter=cfg.max_iter, keep_matches=True):
        ds = datasets[scene]
        keys = scene_inputs(scene)[1]
        for r in res:                                    # inlier ratio of the (top-scored) correspondences, evaluator.py:50-81
            r.ir = inlier_ratio(cfg, r, keys[int(r.id0)], keys[int(r.id1)], ds.get_transform(r.id0, r.id1))
        rows.append(D.pack_rows(scenes.index(scene), res))
        if icp is not None:                              # the same row layout: inliers / iterations / rmse in the n_match / recalltime / ir slots
            rows_icp.append(D.pack_rows(scenes.index(scene), [SimpleNamespace(id0=r.id0, id1=r.id1, n_match=r.icp_inliers, recalltime=r.icp_iters,
                                                                              trans=r.trans_icp, ir=r.icp_rmse) for r in res]))
    for w in writers:                                    # (--save_group_features: the feature files are complete before the table is gathered)
        w.close()
    with D.watchdog(D.collective_timeout(600.0), 'gather of the result table'):     # (waits for the slowest rank's whole share)
        table = D.gather_table(np.concatenate(rows, 0) if rows else np.zeros((0, D.ROW)))
        table_icp = D.gather_table(np.concatenate(rows_icp, 0) if rows_icp else np.zeros((0, D.ROW))) if icp is not None else None
    if rank != 0:
        return None
    by_scene = {s: {} for s in scenes}
    for row in D.unpack_rows(table):
        by_scene[scenes[row['scene']]][(row['id0'], row['id1'])] = row
    fmrs, irs, rrs, rres, rtes = [], [], [], [], []
    for s in scenes:
        ds = datasets[s]
        save_dir = f'{cfg.output_cache_fn}/{ds.name}/match_{cfg.keynum}/{cfg.ET}/{cfg.max_iter}iters'
        make_non_exists_dir(save_dir)
        with open(f'{save_dir}/pre.log', 'w') as w:
            for (a, b) in ds.pair_ids:
                row = by_scene[s][(a, b)]
                np.savez(f'{save_dir}/{a}-{b}.npz', trans=row['trans'], recalltime=row['recalltime'])
                w.write(pre_log_entry(a, b, len(ds.pc_ids), row['trans']))
        f, i, r, re, te = scene_metrics(cfg, [by_scene[s][p] for p in ds.pair_ids], ds.get_transform)
        fmrs.append(f); irs.append(i); rrs.append(r); rres.append(re); rtes.append(te)
    out = {'fmr': float(np.mean(fmrs)), 'ir': float(np.mean(irs)), 'rr': float(np.mean(rrs)), 'rre': float(np.mean(rres)),
           'rte': float(np.mean(rtes)), 'pairs': int(table.shape[0])}
    info_files = {}
    if gt_info is not None and datasets['wholesetname'] != 'demo':
        info_files = write_gt_info(cfg, datasets, scenes, float(gt_info['max_dist']), gt_info.get('voxel'))
    if datasets['wholesetname'] == 'demo' or not all(datasets[s].name in info_files or os.path.exists(_gt_stem(datasets[s]) + '.info') for s in scenes):
        out['rr_predator'] = 1.0 if datasets['wholesetname'] == 'demo' else float('nan')
    else:
        out['rr_predator'] = float(RR_cal.benchmark(cfg, datasets, cfg.keynum, cfg.max_iter, yoho_sign=cfg.ET, info_files=info_files or None)[0])
    msg = f"{datasets['wholesetname']}-{cfg.GF}-{'yoho_det' if cfg.RD else 'nodet'}-{'yoho_mat' if cfg.RM else 'matmul'}-{cfg.ET}-{cfg.keynum}keys-{cfg.max_iter}iters\n"
    msg += f"feature matching recall          : {out['fmr']:.5f}\n" \
           f"inlier ratio                     : {out['ir']:.5f}\n" \
           f"registration recall(predator)    : {out['rr_predator']:.5f}\n" \
           f"rotation error(pointdsc)         : {out['rre']:.5f}\n" \
           f"translation error(pointdsc)      : {out['rte']:.5f}\n" \
           f"registration recall(pointdsc)    : {out['rr']:.5f}"
    make_non_exists_dir(cfg.base_dir)
    with open(f'{cfg.base_dir}/results.log', 'a') as f:
        f.write(msg + '\n')
    print(msg)
    if multiway is not None:
        mw = multiway_poses(cfg, datasets, scenes, engine, by_scene, float(multiway['max_dist']), multiway.get('tau'))
        rr_mw = [scene_metrics(cfg, mw[s][2], datasets[s].get_transform)[2] for s in scenes if s in mw]
        out['multiway'] = {'rr': float(np.mean(rr_mw)) if rr_mw else float('nan'), 'files': {datasets[s].name: mw[s][0] for s in mw},
                           'status': {datasets[s].name: mw[s][1].status for s in mw}, 'iters': {datasets[s].name: mw[s][1].iters for s in mw}, 'poses': {datasets[s].name: mw[s][1].poses for s in mw}}
        msg_mw = f"{msg.split(chr(10), 1)[0]}-multiway\n" \
                 f"scenes with dense clouds         : {len(mw)} of {len(scenes)}\n" \
                 f"registration recall(pointdsc)    : {out['multiway']['rr']:.5f} (pairwise {out['rr']:.5f})"
        with open(f'{cfg.base_dir}/results.log', 'a') as f:
            f.write(msg_mw + '\n')
        print(msg_mw)
    if icp is not None:
        out['icp'] = _write_icp(cfg, datasets, scenes, table_icp, msg.split('\n', 1)[0], icp_suffix(icp),
                                (icp['voxel'], icp.get('voxel_mode', 'centroid')) if icp.get('voxel') is not None else None, icp.get('outliers'))
    return out


def _write_icp(cfg, datasets, scenes, table, label, suffix='', voxel=None, outliers=None):
    """Rank 0's files of the ICP table: {ET}_icp/{iters}iters/{a}-{b}.npz + pre.log per scene, and the '-icp' block of results.log
    (suffix (icp_suffix) '_plane': {ET}_icp_plane/ and '-icp-plane', '_gicp' and '_plane_tukey0.03' likewise; voxel = (size, mode): one more line of the block names it, and one more names the
    outlier filter, outliers = its dict)."""
    by_scene = {s: {} for s in scenes}
    for row in D.unpack_rows(table):
        by_scene[scenes[row['scene']]][(row['id0'], row['id1'])] = row
    rrs, rres, rtes = [], [], []
    for s in scenes:
        ds = datasets[s]
        save_dir = f'{cfg.output_cache_fn}/{ds.name}/match_{cfg.keynum}/{cfg.ET}_icp{suffix}/{cfg.max_iter}iters'
        make_non_exists_dir(save_dir)
        with open(f'{save_dir}/pre.log', 'w') as w:
            for (a, b) in ds.pair_ids:
                row = by_scene[s][(a, b)]
                np.savez(f'{save_dir}/{a}-{b}.npz', trans=row['trans'], recalltime=row['recalltime'], inliers=row['n_match'], rmse=row['ir'])
                w.write(pre_log_entry(a, b, len(ds.pc_ids), row['trans']))
        _, _, r, re, te = scene_metrics(cfg, [by_scene[s][p] for p in ds.pair_ids], ds.get_transform)
        rrs.append(r); rres.append(re); rtes.append(te)
    out = {'rr': float(np.mean(rrs)), 'rre': float(np.mean(rres)), 'rte': float(np.mean(rtes)), 'pairs': int(table.shape[0]), 'table': table}
    msg = f"{label}-icp{suffix.replace('_', '-')}\n" \
          + (f"voxel downsampling               : {voxel[0]:g} ({voxel[1]})\n" if voxel is not None else '') \
          + (f"outlier removal                  : {describe_outliers(outliers)}\n" if outliers is not None else '') + \
          f"rotation error(pointdsc)         : {out['rre']:.5f}\n" \
          f"translation error(pointdsc)      : {out['rte']:.5f}\n" \
          f"registration recall(pointdsc)    : {out['rr']:.5f}"
    with open(f'{cfg.base_dir}/results.log', 'a') as f:
        f.write(msg + '\n')
    print(msg)
    return out


def icp_suffix(icp):
    """The ICP dict of evaluate -> what its folder {ET}_icp... and (with '_' as '-') its block label ...-icp... end in: the method, then the
    loss and its scale, so that runs under different losses do not overwrite each other."""
    suffix = {'plane': '_plane', 'gicp': '_gicp'}.get(icp.get('method', 'point'), '')
    if icp.get('loss') is not None:
        suffix += f"_{icp['loss']}{float(icp['loss_scale']):g}"
    return suffix


def add_icp_arguments(parser):
    parser.add_argument('--icp', action='store_true', help='refine every pair by dense point-to-point ICP on the full clouds (dataset.get_pc), on the device')
    parser.add_argument('--icp_dist', type=float, default=None, help='ICP correspondence distance (default: --ransac_ird)')
    parser.add_argument('--icp_iter', type=int, default=30, help='ICP iterations at most')
    parser.add_argument('--icp_method', choices=('point', 'plane', 'gicp'), default='point',
                        help='point-to-point, point-to-plane against estimated surface normals, or plane-to-plane (generalized ICP) from both clouds\' normals')
    parser.add_argument('--icp_normal_radius', type=float, default=None, help='radius of the normal estimation under --icp_method plane or gicp (default: twice the ICP distance)')
    parser.add_argument('--icp_gicp_epsilon', type=float, default=1e-3, help='--icp_method gicp: covariance along the normal relative to the surface directions, in (0, 1]')
    parser.add_argument('--icp_loss', choices=('huber', 'cauchy', 'gm', 'tukey'), default=None,
                        help='--icp_method plane or gicp: a robust loss on every correspondence inside the distance gate (needs --icp_loss_scale)')
    parser.add_argument('--icp_loss_scale', type=float, default=None, help='--icp_loss: its scale k in metres (the weight is a function of residual / k)')
    parser.add_argument('--icp_voxel', type=float, default=None, help='voxel-grid downsample every dense cloud on the device before the ICP (voxel edge, e.g. 0.025)')
    parser.add_argument('--icp_voxel_mode', choices=('centroid', 'first'), default='centroid', help="a voxel's point: its centroid, or its lowest original row")
    parser.add_argument('--icp_outlier_nb', type=int, default=None, help='statistical outlier removal of every dense cloud before the ICP (after --icp_voxel): '
                        'neighbours per point, at most 32 (needs --icp_outlier_std)')
    parser.add_argument('--icp_outlier_std', type=float, default=None, help='--icp_outlier_nb: keep a point iff its mean neighbour distance is at most the mean + this many standard deviations')
    parser.add_argument('--icp_outlier_radius', type=float, default=None, help='radius outlier removal of every dense cloud before the ICP (needs --icp_outlier_min)')
    parser.add_argument('--icp_outlier_min', type=int, default=None, help='--icp_outlier_radius: keep a point iff at least this many other points lie within the radius')
    parser.add_argument('--icp_outlier_cluster_eps', type=float, default=None, help='cluster outlier removal of every dense cloud before the ICP: the DBSCAN radius '
                        '(needs --icp_outlier_cluster_min_size)')
    parser.add_argument('--icp_outlier_cluster_min_size', type=int, default=None, help='--icp_outlier_cluster_eps: keep a point iff its cluster has at least this many points')
    parser.add_argument('--icp_outlier_cluster_min_points', type=int, default=None, help='--icp_outlier_cluster_eps: a point is a core point iff its ball holds at least this many, '
                        'itself included (default 1: connected components)')


def outlier_options(cfg):
    """The parsed --icp_outlier... arguments -> the outliers dict of roreg_amd.outliers (None without them).  ValueError: without --icp, both
    two kinds at once, half a kind, or values the filter refuses."""
    from .outliers import check_args
    stat = (getattr(cfg, 'icp_outlier_nb', None), getattr(cfg, 'icp_outlier_std', None))
    rad = (getattr(cfg, 'icp_outlier_radius', None), getattr(cfg, 'icp_outlier_min', None))
    clu = (getattr(cfg, 'icp_outlier_cluster_eps', None), getattr(cfg, 'icp_outlier_cluster_min_size', None), getattr(cfg, 'icp_outlier_cluster_min_points', None))
    any_stat, any_rad, any_clu = any(v is not None for v in stat), any(v is not None for v in rad), any(v is not None for v in clu)
    if not any_stat and not any_rad and not any_clu:
        return None
    if not cfg.icp:
        raise ValueError('--icp_outlier_* need --icp (the filter runs on the dense clouds of the refinement)')
    if any_stat and any_rad:
        raise ValueError('--icp_outlier_nb / --icp_outlier_std and --icp_outlier_radius / --icp_outlier_min are two filters: give one')
    if any_clu and (any_stat or any_rad):
        raise ValueError('--icp_outlier_cluster_* is a third filter beside --icp_outlier_nb / --icp_outlier_std and --icp_outlier_radius / --icp_outlier_min: give one')
    if any_clu:
        if clu[0] is None or clu[1] is None:
            raise ValueError('--icp_outlier_cluster_eps and --icp_outlier_cluster_min_size go together (--icp_outlier_cluster_min_points is optional)')
        return check_args(dict(kind='cluster', eps=clu[0], min_size=clu[1], min_points=1 if clu[2] is None else clu[2]), '--icp_outlier_cluster_eps')
    if any_stat:
        if None in stat:
            raise ValueError('--icp_outlier_nb and --icp_outlier_std go together')
        return check_args(dict(kind='statistical', nb_neighbors=stat[0], std_ratio=stat[1]), '--icp_outlier_nb')
    if None in rad:
        raise ValueError('--icp_outlier_radius and --icp_outlier_min go together')
    return check_args(dict(kind='radius', radius=rad[0], min_neighbors=rad[1]), '--icp_outlier_radius')


def describe_outliers(spec):
    from .outliers import describe
    return describe(spec)


def icp_options(cfg):
    """The parsed --icp... arguments -> evaluate's icp dict (None without --icp).  ValueError: a loss under a method that has none, a loss
    without a usable scale, or outlier flags outlier_options refuses."""
    from .icp import check_loss
    outlier_spec = outlier_options(cfg)
    if cfg.icp_loss is not None or cfg.icp_loss_scale is not None:
        if cfg.icp_loss is None:
            raise ValueError('--icp_loss_scale needs --icp_loss')
        if cfg.icp_method not in ('plane', 'gicp'):
            raise ValueError(f'--icp_loss needs --icp_method plane or gicp, not {cfg.icp_method}')
        check_loss(cfg.icp_method, cfg.icp_loss, cfg.icp_loss_scale, '--icp_loss')
    icp = dict(max_dist=cfg.ransac_ird if cfg.icp_dist is None else cfg.icp_dist, max_iter=cfg.icp_iter) if cfg.icp else None
    if icp is not None and cfg.icp_method == 'plane':
        icp.update(method='plane', normal_radius=cfg.icp_normal_radius)
    if icp is not None and cfg.icp_method == 'gicp':
        icp.update(method='gicp', normal_radius=cfg.icp_normal_radius, gicp_epsilon=cfg.icp_gicp_epsilon)
    if icp is not None and cfg.icp_loss is not None:
        icp.update(loss=cfg.icp_loss, loss_scale=cfg.icp_loss_scale)
    if icp is not None and cfg.icp_voxel is not None:
        icp.update(voxel=cfg.icp_voxel, voxel_mode=cfg.icp_voxel_mode)
    if icp is not None and outlier_spec is not None:
        icp.update(outliers=outlier_spec)
    return icp


def main():
    from .parses.parses_test import build_parser
    from .dataops.dataset import get_dataset_name
    parser = build_parser()
    add_icp_arguments(parser)
    parser.add_argument('--seed', type=int, default=None, help='one generator stream per pair (results independent of the number of ranks)')
    parser.add_argument('--gt_info_dist', type=float, default=None, help='compute the information matrices of scenes without a gt.info from their dense clouds '
                        '(correspondences within this distance under the ground truth) and RR(predator) from them')
    parser.add_argument('--gt_info_voxel', type=float, default=None, help='voxel-grid downsample the dense clouds first under --gt_info_dist')
    parser.add_argument('--multiway', action='store_true', help='optimise every scene\'s pose graph on the device after the pairwise run (scenes with dense '
                        'clouds, dataset.get_pc) and write {output_cache_fn}/{scene}/multiway_poses.log')
    parser.add_argument('--multiway_tau', type=float, default=None, help='scale in metres of the robust kernel that votes wrong pairs down (default: none)')
    parser.add_argument('--from_points', action='store_true', help='no feature files: compute every cloud\'s group feature from its raw points on the device '
                        '(dataset.get_pc / get_kps through the FCGF backbone), once per cloud, and keep it there')
    parser.add_argument('--backbone_model', default=None, help='--from_points: the FCGF checkpoint (config + state_dict)')
    parser.add_argument('--voxel_size', type=float, default=0.025, help='--from_points: the backbone\'s voxel edge')
    parser.add_argument('--rot_batch', type=int, default=12, help='--from_points: rotations per sparse tensor')
    parser.add_argument('--save_group_features', action='store_true', help='--from_points: also write every cloud\'s group feature where the file-backed run '
                        'reads it ({backbone}_Input_Group_feature/{pc}.npy, the bytes of python -m roreg_amd.testset)')
    parser.add_argument('--multiway_dist', type=float, default=None, help='correspondence distance of the information matrices (default: --ransac_ird)')
    parser.add_argument('--sc2_tau', type=float, default=None, help='--ET sc2: the compatibility threshold in metres (default: --ransac_ird)')
    parser.add_argument('--sc2_k', type=int, default=None, help='--ET sc2: members of a consensus set at most, 3..64 (default: 20)')
    cfg, _ = parser.parse_known_args()
    rank = int(os.environ.get('RANK', 0)); world = int(os.environ.get('WORLD_SIZE', 1)); local = int(os.environ.get('LOCAL_RANK', 0))
    torch.cuda.set_device(local)
    if world > 1 or D.forced():
        D.init_collectives('nccl', rank, world, local)
    try:
        icp = icp_options(cfg)
    except ValueError as e:
        parser.error(str(e))
    datasets = get_dataset_name(cfg.testset, cfg.origin_data_dir)
    gt_info = dict(max_dist=cfg.gt_info_dist, voxel=cfg.gt_info_voxel) if cfg.gt_info_dist is not None else None
    multiway = dict(max_dist=cfg.ransac_ird if cfg.multiway_dist is None else cfg.multiway_dist, tau=cfg.multiway_tau) if cfg.multiway else None
    raw = None
    if cfg.from_points:
        if not cfg.backbone_model:
            parser.error('--from_points needs --backbone_model CKPT')
        from .backbone import fcgf
        raw = dict(model=fcgf.from_checkpoint(cfg.backbone_model), voxel_size=cfg.voxel_size, rot_batch=cfg.rot_batch, save=cfg.save_group_features)
    evaluate(cfg, datasets, build_engine(cfg), rank, world, cfg.seed, icp=icp, gt_info=gt_info, multiway=multiway, raw=raw)
    if world > 1 or D.forced():
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
