"""Raw clouds to registrations on the device: the group-feature assembly kernel (csrc/group_feature.hip), group_features_device, the lazy
feature source behind the engine, Registrar, and the multi-GPU driver's --from_points route.  GPU only.

One narrow FCGF network (tests/test_hip_sparse_conv.py's), three 2000-point clouds at voxel 0.05 with 64 keypoints each; the host features of
extract_group_features and the scene's results on them are computed once per module and shared."""
import filecmp
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _raw_scene_cases as K
import _sparse_conv_oracle as O
from test_sparse_conv_oracle import NARROW
from test_hip_sparse_conv import device_model
from test_hip_icp import _cfg_and_nets, _same_bits
from roreg_amd import synth

pytestmark = pytest.mark.gpu

VOXEL, N_KPS, KEYNUM = 0.05, 64, 48
PAIRS = [('0', '1'), ('0', '2'), ('1', '2')]
RUN_KW = dict(keynum=KEYNUM, keep_matches=True)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1, 2: the kernel --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [32, 16])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 257])
def test_assembly_kernel_equals_numpy_bitwise_at_its_edges(N, F):
    """Every R in {1, 3, 12, 60} with the window at column 0 and ending at column 59 (aligned and unaligned windows: both store forms), float32
    and bfloat16 output, items of one row, first and last rows named, exact rounding ties: the window holds numpy's bits, the rest the sentinel."""
    from roreg_amd import hip
    for R in (1, 3, 12, 60):
        feats, cuts, nn = K.kernel_case(7, N, R, F)
        for g0 in sorted({0, 60 - R}):
            want = torch.from_numpy(K.assemble_numpy(feats, cuts, nn, g0, np.full((N, F, 60), K.SENTINEL, np.float32)))
            for dtype, view in ((torch.float32, torch.int32), (torch.bfloat16, torch.int16)):
                out = torch.full((N, F, 60), K.SENTINEL, dtype=dtype, device='cuda')
                got = hip.group_feature_assemble(_dev(feats), _dev(cuts), _dev(nn), g0, out)
                assert got is out
                assert torch.equal(out.cpu().view(view), want.to(dtype).view(view)), (N, F, R, g0, dtype)
        ties = (feats.view(np.uint32) & 0xFFFF) == 0x8000
        assert ties.any() and (want[:, :, 60 - R:].to(torch.bfloat16).float() != want[:, :, 60 - R:]).any()          # the rounding had work to do


def test_rejected_arguments_and_the_next_call_is_correct():
    from roreg_amd import hip
    N, R, F = 65, 12, 32
    feats, cuts, nn = K.kernel_case(8, N, R, F)
    f, c, n = _dev(feats), _dev(cuts), _dev(nn)
    out = torch.full((N, F, 60), K.SENTINEL, dtype=torch.float32, device='cuda')
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, n, 49, out)                                       # g0 + R = 61
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, n[:0], 0, out)                                    # R < 1
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f.double(), c, n, 0, out)
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, n.int(), 0, out)
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, n, 0, out.half())
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c[:-1], n, 0, out)
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, n, 0, out[:-1])
    assert (out == K.SENTINEL).all()                                                       # nothing was launched
    bad = nn.copy()
    bad[5, 17] = cuts[6] - cuts[5]                                                         # the item's row count: one past its last row
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, _dev(bad), 0, out)
    last = nn.copy()
    last[R - 1, 3] = cuts[R] - cuts[R - 1]                                                 # ... of the last item: the row past the end of feats
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, _dev(last), 0, out)
    neg = nn.copy()
    neg[0, 0] = -1
    with pytest.raises(hip.HipError):
        hip.group_feature_assemble(f, c, _dev(neg), 0, out)
    out.fill_(K.SENTINEL)
    hip.group_feature_assemble(f, c, n, 48, out)
    want = K.assemble_numpy(feats, cuts, nn, 48, np.full((N, F, 60), K.SENTINEL, np.float32))
    assert _same_bits(out.cpu().numpy(), want)


# ---- the scene the rest shares ---------------------------------------------------------------------------------------------------------------------
class RawScene:
    """A dataset as run_distributed.evaluate uses one, with raw clouds and keypoints and no files."""
    name = 'synth/raw0'

    def __init__(self, clouds, kps, gt, root):
        self.clouds, self.kps, self.gt = clouds, kps, gt
        self.pc_ids = [str(i) for i in range(len(clouds))]
        self.pair_ids = list(PAIRS)
        self.gt_dir = f'{root}/nonexistent/{self.name}/gt.log'

    def get_pc(self, i):
        return self.clouds[int(i)]

    def get_kps(self, i):
        return self.kps[int(i)]

    def get_transform(self, a, b):
        return (np.linalg.inv(self.gt[int(a)]) @ self.gt[int(b)])[:3]


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    """Model, three clouds with keypoints, engine parts, the host features of extract_group_features and the scene's results on them."""
    from roreg_amd import testset
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.register import pair_seeds
    root = tmp_path_factory.mktemp('raw_scene')
    model = device_model(O.random_state_dict(12, conv1_kernel_size=3, **NARROW), 3, **NARROW)
    p0, p1, Tg = synth.make_dense_pair(3, 2000)
    T2 = synth.dense_gt(25.0, (0.0, 0.0, 1.0), (0.3, -0.2, 0.0))
    rng = np.random.default_rng(6)
    p2 = ((p0[rng.permutation(2000)].astype(np.float64) + rng.normal(0, 0.002, (2000, 3)) - T2[:3, 3]) @ T2[:3, :3]).astype(np.float32)       # p0 ~ p2 R^T + t
    clouds = [p0, p1, p2]
    kps = [c[np.random.default_rng(10 + q).choice(2000, N_KPS, replace=False)].astype(np.float64) for q, c in enumerate(clouds)]
    cfg, gf, et = _cfg_and_nets(root, dict(keynum=KEYNUM), ET='yohoo', testset='synth')
    host = [testset.extract_group_features(model, c, k, voxel_size=VOXEL, rot_batch=3) for c, k in zip(clouds, kps)]
    seeds = pair_seeds(5, PAIRS)
    want = {}
    eng = RegistrationEngine(cfg, gf, et)
    for name in ('fp32', 'bf16'):
        eng.set_descriptor_dtype(name)
        want[name] = eng.run_scene(dict(enumerate(host)), dict(enumerate(kps)), PAIRS, pair_seeds=seeds, max_iter=cfg.max_iter, **RUN_KW)
    assert sum(r.n_match for r in want['fp32']) > 0
    return NS(root=root, model=model, clouds=clouds, kps=kps, gt=[np.eye(4), Tg, T2], cfg=cfg, gf=gf, et=et, host=host, seeds=seeds, want=want)


def _engine(scene, dtype='fp32'):
    from roreg_amd.engine import RegistrationEngine
    eng = RegistrationEngine(scene.cfg, scene.gf, scene.et)
    eng.set_descriptor_dtype(dtype)
    return eng


def _source(scene, eng, **kw):
    from roreg_amd.testset import GroupFeatureSource
    return GroupFeatureSource(scene.model, lambda i: scene.clouds[i], lambda i: scene.kps[i], VOXEL, 12, eng.feat_dtype, **kw)


def _assert_same_results(got, want):
    assert [(r.id0, r.id1) for r in got] == [(r.id0, r.id1) for r in want]
    for g, w in zip(got, want):
        assert _same_bits(g.trans, w.trans) and g.n_match == w.n_match and g.recalltime == w.recalltime, (g.id0, g.id1)
        assert torch.equal(g.matches, w.matches), (g.id0, g.id1)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_device_extraction_equals_the_existing_path(scene):
    from roreg_amd import testset
    ref = torch.from_numpy(scene.host[0])
    assert ref.shape == (N_KPS, 32, 60)
    for r in (1, 7, 60):                                          # 7 does not divide 60: the last batch is short (and its window unaligned)
        got = testset.group_features_device(scene.model, scene.clouds[0], scene.kps[0], voxel_size=VOXEL, rot_batch=r)
        assert got.is_cuda and got.dtype == torch.float32
        assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)), r
    got = testset.group_features_device(scene.model, scene.clouds[0], scene.kps[0], voxel_size=VOXEL, rot_batch=12, dtype=torch.bfloat16)
    assert got.dtype == torch.bfloat16 and torch.equal(got.cpu().view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))
    with pytest.raises(ValueError):
        testset.group_features_device(scene.model, scene.clouds[0], scene.kps[0], voxel_size=VOXEL, dtype=torch.float16)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_the_engine_cannot_tell_a_source_from_host_arrays(scene, dtype):
    eng = _engine(scene, dtype)
    src = _source(scene, eng)
    assert src.rows(1) == N_KPS and src.like(2).shape == (N_KPS, 32, 60) and src.runs == {}         # the row count costs no backbone run
    got = eng.run_scene(src, dict(enumerate(scene.kps)), PAIRS, pair_seeds=scene.seeds, max_iter=scene.cfg.max_iter, **RUN_KW)
    _assert_same_results(got, scene.want[dtype])
    assert src.runs == {0: 1, 1: 1, 2: 1}


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_registrar(scene):
    from roreg_amd import icp
    from roreg_amd.register import Registrar
    reg = Registrar(_engine(scene), scene.model, voxel_size=VOXEL, rot_batch=12, n_keypoints=N_KPS)
    got = reg.scene(scene.clouds, [(0, 1), (0, 2), (1, 2)], keypoints=scene.kps, seed=5, max_iter=scene.cfg.max_iter, **RUN_KW)
    _assert_same_results(got, scene.want['fp32'])
    assert reg.last_source.runs == {0: 1, 1: 1, 2: 1}
    assert all(r.keypoints0 is scene.kps[int(r.id0)] or np.array_equal(r.keypoints0, scene.kps[int(r.id0)]) for r in got)
    opts = dict(max_dist=0.1, max_iter=10)
    one = reg.pair(scene.clouds[0], scene.clouds[1], scene.kps[0], scene.kps[1], seed=5, icp=opts, max_iter=scene.cfg.max_iter, **RUN_KW)
    _assert_same_results([one], scene.want['fp32'][:1])
    assert reg.last_source.runs == {0: 1, 1: 1}
    ref = icp.refine(scene.clouds[0], scene.clouds[1], one.trans, **opts)
    assert _same_bits(one.trans_icp, ref.T) and one.icp_iters == ref.iters and one.icp_inliers == ref.inliers and one.icp_status == ref.status
    # default keypoints: a seeded call is a function of its arguments and leaves the global generator alone
    np.random.seed(99)
    state = np.random.get_state()
    a = reg.pair(scene.clouds[0], scene.clouds[1], seed=11, max_iter=scene.cfg.max_iter, **RUN_KW)
    b = reg.pair(scene.clouds[0], scene.clouds[1], seed=11, max_iter=scene.cfg.max_iter, **RUN_KW)
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]
    _assert_same_results([a], [b])
    assert a.keypoints0.shape == (N_KPS, 3) and _same_bits(a.keypoints0, b.keypoints0) and _same_bits(a.keypoints1, b.keypoints1)
    rows = np.arange(2000); np.random.RandomState(11).shuffle(rows)
    assert _same_bits(a.keypoints0, scene.clouds[0][rows[:N_KPS]].astype(np.float64))


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_driver_from_points_writes_the_file_backed_run_s_files(scene):
    """run_distributed.evaluate at world size 1: from raw points (raw=, with save) against the file-backed run on write_group_features's files."""
    from roreg_amd import run_distributed as RD_, testset
    from roreg_amd.engine import RegistrationEngine
    outs, cfgs = {}, {}
    for kind in ('files', 'raw'):
        root = scene.root / f'driver_{kind}'
        root.mkdir()
        cfg = cfgs[kind] = NS(**{**vars(scene.cfg), 'output_cache_fn': f'{root}/cache', 'base_dir': str(root)})
        ds = RawScene(scene.clouds, scene.kps, scene.gt, root)
        if kind == 'files':
            testset.write_group_features(scene.model, ds, cfg.output_cache_fn, cfg.backbone, voxel_size=VOXEL, rot_batch=12)
        raw = dict(model=scene.model, voxel_size=VOXEL, rot_batch=12, save=True) if kind == 'raw' else None
        outs[kind] = RD_.evaluate(cfg, {'wholesetname': 'synth', 'scene0': ds}, RegistrationEngine(cfg, scene.gf, scene.et), rank=0, world=1, seed=3, raw=raw)
    assert outs['files'].keys() == outs['raw'].keys()
    for k in outs['files']:
        assert outs['files'][k] == outs['raw'][k] or (np.isnan(outs['files'][k]) and np.isnan(outs['raw'][k])), k
    d0, d1 = (f"{cfgs[k].output_cache_fn}/{RawScene.name}" for k in ('files', 'raw'))
    sub = f'match_{scene.cfg.keynum}/yohoo/{scene.cfg.max_iter}iters'
    files = sorted(os.listdir(f'{d0}/{sub}'))
    assert files == sorted(os.listdir(f'{d1}/{sub}')) and len(files) == len(PAIRS) + 1 and 'pre.log' in files
    for f in files:
        if f.endswith('.npz'):                                    # (an archive's member headers carry the time it was written: the members' bytes)
            a, b = np.load(f'{d0}/{sub}/{f}'), np.load(f'{d1}/{sub}/{f}')
            assert sorted(a.files) == sorted(b.files) == ['recalltime', 'trans'] and all(_same_bits(a[k], b[k]) for k in a.files), f
        else:
            assert filecmp.cmp(f'{d0}/{sub}/{f}', f'{d1}/{sub}/{f}', shallow=False), f
    fdir = f'{scene.cfg.backbone}_Input_Group_feature'
    assert sorted(os.listdir(f'{d0}/{fdir}')) == sorted(os.listdir(f'{d1}/{fdir}')) == ['0.npy', '1.npy', '2.npy']
    for f in ('0.npy', '1.npy', '2.npy'):
        assert filecmp.cmp(f'{d0}/{fdir}/{f}', f'{d1}/{fdir}/{f}', shallow=False), f
    assert _same_bits(np.load(f'{d1}/{fdir}/1.npy'), scene.host[1])


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------------
def test_a_cut_scene_runs_the_backbone_once_per_cloud(scene):
    from roreg_amd import distributed as D
    eng = _engine(scene)
    lists = {'s': PAIRS}
    keys = dict(enumerate(scene.kps))
    kw = dict(keynum=KEYNUM, max_iter=scene.cfg.max_iter, keep_matches=True)

    # one rank that ships two clouds to itself, host-staged: the whole exchange branch over a computing source
    src = _source(scene, eng)
    pieces = [('s', 0, len(PAIRS))]
    transfers = D.self_transfers(pieces, lists, rank=0, n_clouds=2)
    assert len(transfers) == 2
    stats = {}
    done = D.run_plan(eng, pieces, lambda s: (src, keys, PAIRS, scene.seeds), transfers, 0, exchange=D.EqvExchange(0, device_payloads=False), stats=stats, **kw)
    _assert_same_results([r for _, _, _, res in done for r in res], scene.want['fp32'])
    assert src.runs == {0: 1, 1: 1, 2: 1}
    one = 2 * N_KPS * 32 * 60 * 4
    assert stats == {'eqv_bytes_sent': one, 'eqv_bytes_received': one, 'before_bytes_sent': one, 'before_bytes_received': one}

    # an emulated world of 2, each rank's share in turn, under two prices of a cloud: the plan may differ, the table may not
    tables = []
    for cost in (9.0, 100.0):
        plan = D.shard_scenes({'s': len(PAIRS)}, 2, {'s': 3}, cloud_cost=cost, pair_lists=lists, exchange=True)
        _, transfers = D.exchange_plan(plan, lists)
        order = K.rank_order(plan, 's')
        assert len(order) == 2 and transfers and all(order.index(a) < order.index(b) for _, _, a, b in transfers)
        box, rows, sources = {}, {}, []
        for rank in order:
            s_r = _source(scene, eng)
            sources.append(s_r)
            for _, _, _, res in D.run_plan(eng, plan[rank], lambda s: (s_r, keys, PAIRS, scene.seeds), transfers, rank, exchange=K.Mailbox(rank, box), **kw):
                rows.update({(r.id0, r.id1): r for r in res})
        assert all(sources[0].runs.get(i, 0) + sources[1].runs.get(i, 0) == 1 for i in range(3))
        tables.append([rows[p] for p in PAIRS])
    _assert_same_results(tables[0], scene.want['fp32'])
    _assert_same_results(tables[1], scene.want['fp32'])
