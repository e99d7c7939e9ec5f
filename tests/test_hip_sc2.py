"""The spatial-compatibility estimator on the device (csrc/sc2.hip, roreg_amd/sc2.py, cfg.ET = 'sc2') against its numpy definition
(tests/_sc2_oracle.py) and against the pinned scorer / refiner.  GPU only.  The cases and their oracle results are built once per process
(tests/_sc2_cases.py); tests/test_sc2_oracle.py asserts on the CPU that they keep the threshold margin and the conditioning cap."""
import filecmp
import glob
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _sc2_cases as C
from oracle import ref_numpy as R
from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu

STAGE_CASES = C.stage_cases()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _task(case, seed=0):
    """the case's correspondences behind a match list: keypoint tables in scrambled order with rows no match uses"""
    M = case.P.shape[0]
    rng = np.random.default_rng(seed)
    r0, r1 = rng.permutation(M + 7)[:M], rng.permutation(M + 3)[:M]
    k0 = rng.uniform(-9, 9, (M + 7, 3)); k1 = rng.uniform(-9, 9, (M + 3, 3))
    k0[r0] = case.P; k1[r1] = case.Q
    return _dev(k0), _dev(k1), _dev(np.stack([r0, r1], 1).astype(np.int64))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_against_oracle(case, Trans, dbg):
    ref = case.ref
    assert dbg['guards_ok']
    assert _same_bits(dbg['bits'], ref.bits), 'bit rows (zero padding included)'
    assert _same_bits(dbg['deg'], ref.deg) and _same_bits(dbg['seeds'], ref.seeds)
    assert _same_bits(dbg['N2'], ref.N2) and _same_bits(dbg['cons'], ref.cons)
    T = Trans.cpu().numpy()
    assert T.shape == ref.Trans.shape
    fitted, ok = C.fitted_rows(case)
    assert _same_bits(T[~fitted], ref.Trans[~fitted]), 'sets of fewer than 3 members: R = I, t = P_s - Q_s exactly'
    if ok.any():
        err = np.abs(T[ok] - ref.Trans[ok]).reshape(int(ok.sum()), -1).max(1)
        bound = 1e-9 * np.maximum(1.0, np.linalg.norm(ref.Trans[ok][:, :, 3], axis=1))
        det = np.linalg.det(T[ok][:, :, :3])
        print(f'{case.name}: {int(ok.sum())} fitted rows, max error {err.max():.2e}, max |det - 1| {np.abs(det - 1).max():.2e}, '
              f'{int((np.linalg.det(C.unfixed_rotations(case, ok)) < 0).sum())} of them with a reflection to fix')
        assert (err <= bound).all() and np.abs(det - 1.0).max() < 1e-12
    assert np.isfinite(T).all()


@pytest.mark.parametrize('idx', range(len(STAGE_CASES)), ids=[c.name for c in STAGE_CASES])
def test_stages_bit_exact_and_hypotheses(idx):
    """bit rows, degrees, seeds, N2 and consensus lists equal the oracle's bit for bit; hypotheses of small sets bit for bit, fitted ones within
    1e-9 max(1, |t|) with det R = +1"""
    from roreg_amd import hip
    case = STAGE_CASES[idx]
    Trans, offsets, dbg = hip.sc2_hypotheses_batch([_task(case, idx)], case.tau, case.max_seeds, case.K, debug=True)
    assert offsets == [(0, min(case.P.shape[0], case.max_seeds))]
    _check_against_oracle(case, Trans, dbg[0])


def test_batching_does_not_change_a_pair():
    """three pairs of different M in one call, in either order and cut into groups by a small workspace cap: each pair's rows and stages are
    bit for bit those of its single call; the guards behind every region and output are intact"""
    from roreg_amd import hip
    cases = [C.synth_case(11, 65, 0.6), C.synth_case(11, 257, 0.6), C.synth_case(11, 0, 0.6), C.synth_case(11, 129, 0.6)]
    tasks = [_task(c, 40 + q) for q, c in enumerate(cases)]
    single = [hip.sc2_hypotheses_batch([t], C.TAU, 100, 20, debug=True) for t in tasks]
    for order, cap in (([0, 1, 2, 3], None), ([3, 2, 1, 0], None), ([1, 3, 0, 2], 200000)):
        Trans, offsets, dbg = hip.sc2_hypotheses_batch([tasks[q] for q in order], C.TAU, 100, 20, debug=True, workspace_cap=cap)
        assert [S for _, S in offsets] == [min(cases[q].P.shape[0], 100) for q in order]
        for pos, q in enumerate(order):
            o, S = offsets[pos]
            assert _same_bits(Trans[o:o + S].cpu().numpy(), single[q][0].cpu().numpy()), (order, q)
            assert dbg[pos]['guards_ok']
            for k in ('bits', 'deg', 'seeds', 'N2', 'cons'):
                assert _same_bits(dbg[pos][k], single[q][2][0][k]), (order, q, k)
    plain, off2 = hip.sc2_hypotheses_batch(tasks, C.TAU, 100, 20)                   # and without debug: the same rows
    assert _same_bits(plain.cpu().numpy(), np.concatenate([s[0].cpu().numpy() for s in single]))


@pytest.mark.parametrize('which', ['M257-60', 'M1500-90'])
def test_register_is_the_pinned_scorer_and_refiner_on_the_device_hypotheses(which):
    """sc2.register = oracle.ref_numpy's overlap scan and two refinements applied to the DEVICE's hypotheses: same winner, transform within
    the refinement tests' 1e-9; and it lands on the case's ground truth"""
    from roreg_amd import sc2
    case = C.synth_case(11, 257, 0.6) if which == 'M257-60' else C.synth_case(11, 1500, 0.9)
    k0, k1, m = _task(case, 3)
    rng = np.random.default_rng(8)
    for scores in (None, rng.uniform(0.2, 1.0, case.P.shape[0])):
        hyp = sc2.hypotheses(k0, k1, m, tau=case.tau).cpu().numpy()
        res = sc2.register(k0, k1, m, scores, ird=case.tau)
        w = np.ones(case.P.shape[0]) if scores is None else scores
        ov = np.array([R.overlap_cal(case.P, case.Q, T, w, case.tau) for T in hyp])
        best = int(np.argmax(ov))
        want = R.refine_trans(case.P, case.Q, R.refine_trans(case.P, case.Q, hyp[best], w, 2 * case.tau), w, case.tau)
        assert res.row == best and res.n_hyp == hyp.shape[0]
        assert np.abs(res.T - want).max() < 1e-9
        assert np.abs(res.T - C.ground_truth()).max() < 0.02
    many = sc2.register([(k0, k1, m, None), (case.P, case.Q), (case.P[:0], case.Q[:0])], ird=case.tau)
    assert _same_bits(many[0].T, sc2.register(k0, k1, m, ird=case.tau).T) and _same_bits(many[1].T, many[0].T) and many[1].row == many[0].row
    assert many[2].row == -1 and np.isnan(many[2].T[:3]).all()


def test_rejected_arguments_and_the_next_call_is_correct():
    from roreg_amd import hip
    case = C.synth_case(11, 65, 0.6)
    k0, k1, m = _task(case, 1)
    big = torch.zeros((hip.SC2_MAX_M + 1, 2), dtype=torch.int64, device='cuda')
    for bad, exc in ((lambda: hip.sc2_hypotheses_batch([(k0, k1, big)], 0.1), hip.HipError),
                     (lambda: hip.sc2_hypotheses_batch([(k0.float(), k1, m)], 0.1), hip.HipError),
                     (lambda: hip.sc2_hypotheses_batch([(k0, k1, m.int())], 0.1), hip.HipError),
                     (lambda: hip.sc2_hypotheses_batch([(k0, k1, m)], 0.1, K=2), ValueError),
                     (lambda: hip.sc2_hypotheses_batch([(k0, k1, m)], 0.1, K=65), ValueError),
                     (lambda: hip.sc2_hypotheses_batch([(k0, k1, m)], float('nan')), ValueError)):
        with pytest.raises(exc):
            bad()
        Trans, _, dbg = hip.sc2_hypotheses_batch([(k0, k1, m)], case.tau, case.max_seeds, case.K, debug=True)
        _check_against_oracle(case, Trans, dbg[0])
    rc = hip.lib().roreg_sc2_hypotheses_batch(None, 1, 10, 10, 100, 10, 10, 0.1, 2, None, None, None, None, 0, None)     # the C entry refuses K itself
    assert rc != 0 and b'K must lie in 3..64' in hip.lib().roreg_last_error()


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------
KEYNUM, N_KPTS = 150, 192


def _scene_and_nets(tmp_path, **kw):
    from roreg_amd.network import name2network
    root = str(tmp_path)
    cfg = default_config(output_cache_fn=f'{root}/cache', model_fn=f'{root}/ckpt', base_dir=root, SO3_related_files=None, keynum=KEYNUM, bs_GF=50,
                         ET='sc2', max_iter=1000, **kw)
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    os.makedirs(f'{root}/ckpt/GF', exist_ok=True)                                # a GF checkpoint and NO ET checkpoint: sc2 must not ask for one
    torch.save({'best_para': 0, 'network_state_dict': gf.state_dict()}, f'{root}/ckpt/GF/model_best.pth')
    ds = synth.make_scene(41, n_clouds=3, n_kpts=N_KPTS, overlap=0.6, name='synth/scene0')
    ds.gt_dir = f'{root}/nonexistent/{ds.name}/gt.log'
    return cfg, gf, ds


def test_engine_sc2_equals_register_and_draws_nothing(tmp_path):
    """cfg.ET = 'sc2' with et_net = None: every PairResult is bit for bit sc2.register on the pair's matches; the estimator consumes no random
    number -- numpy's global generator ends where the matcher's two shuffles per pair leave it, and with per-pair streams (two different seed
    lists) the results are still register's on the matches each run produced and the global generator is untouched"""
    from roreg_amd import sc2
    from roreg_amd.engine import RegistrationEngine
    cfg, gf, ds = _scene_and_nets(tmp_path)
    keys = [ds.get_kps(i) for i in ds.pc_ids]
    eng = RegistrationEngine(cfg, gf, None)
    assert len(ds.pair_ids) == 3

    def check(res):
        want = sc2.register([(keys[int(r.id0)], keys[int(r.id1)], r.matches) for r in res], ird=cfg.ransac_ird, max_seeds=1000)
        for r, w in zip(res, want):
            assert r.n_match > 20 and np.isfinite(r.trans).all()
            assert _same_bits(r.trans, w.T) and r.recalltime == w.row, (r.id0, r.id1)
            gt = np.eye(4); gt[:3] = ds.get_transform(r.id0, r.id1)
            assert np.abs(r.trans - gt).max() < 0.05
    np.random.seed(5)
    res = eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=KEYNUM, max_iter=1000, keep_matches=True)
    after = np.random.get_state()
    np.random.seed(5)
    for _ in ds.pair_ids:
        for _ in range(2):
            idx = np.arange(N_KPTS); np.random.shuffle(idx)
    left = np.random.get_state()
    assert after[0] == left[0] and np.array_equal(after[1], left[1]) and after[2:] == left[2:]
    check(res)
    for seeds in ([10, 20, 30], [11, 21, 31]):
        np.random.seed(5)
        before = np.random.get_state()
        check(eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=KEYNUM, max_iter=1000, keep_matches=True, pair_seeds=seeds))
        now = np.random.get_state()
        assert np.array_equal(before[1], now[1]) and before[2:] == now[2:]
    # cfg.sc2_tau / cfg.sc2_k reach the kernels
    cfg2 = NS(**{**vars(cfg), 'sc2_tau': 0.05, 'sc2_k': 8})
    np.random.seed(5)
    res2 = RegistrationEngine(cfg2, gf, None).run_scene(ds.feats, keys, ds.pair_ids, keynum=KEYNUM, max_iter=1000, keep_matches=True)
    want2 = sc2.register([(keys[int(r.id0)], keys[int(r.id1)], r.matches) for r in res2], ird=cfg.ransac_ird, tau=0.05, k=8)
    assert all(_same_bits(r.trans, w.T) for r, w in zip(res2, want2))


def test_stage_class_and_evaluator_engine_route_write_identical_archives(tmp_path, monkeypatch):
    """yoho_evaluator.process_scene under --ET sc2 through the chain of stage.run() calls and through the engine: the same match and score
    files, result archives equal member by member, the same pre.log; no DR_index or Trans_pre file, no ET checkpoint anywhere"""
    from roreg_amd.test import _cache
    from roreg_amd.test.evaluator import yoho_evaluator
    cfg, gf, ds = _scene_and_nets(tmp_path)
    roots = {}
    for route in ('stages', 'engine'):
        c = NS(**{**vars(cfg), 'output_cache_fn': f'{tmp_path}/cache_{route}'})
        ds.write_inputs(c.output_cache_fn)
        monkeypatch.setenv('ROREG_EVALUATOR', route)
        _cache.clear()
        ev = yoho_evaluator(c)
        assert ev._engine_route() == (route == 'engine')
        np.random.seed(77)
        ev.process_scene(ds)
        roots[route] = f'{c.output_cache_fn}/{ds.name}'
    a, b = roots['stages'], roots['engine']
    rel = sorted(os.path.relpath(f, a) for f in glob.glob(f'{a}/**/*.npy', recursive=True) if 'Input_Group_feature' not in f)
    assert rel == sorted(os.path.relpath(f, b) for f in glob.glob(f'{b}/**/*.npy', recursive=True) if 'Input_Group_feature' not in f)
    assert not any('DR_index' in r or 'Trans_pre' in r for r in rel) and any(r.startswith(f'match_{KEYNUM}/scores') for r in rel)
    for r in rel:
        assert filecmp.cmp(f'{a}/{r}', f'{b}/{r}', shallow=False), r
    rdir = f'match_{KEYNUM}/sc2/1000iters'
    for p0, p1 in ds.pair_ids:
        x, y = np.load(f'{a}/{rdir}/{p0}-{p1}.npz'), np.load(f'{b}/{rdir}/{p0}-{p1}.npz')
        assert sorted(x.files) == sorted(y.files) == ['recalltime', 'trans']
        for k in x.files:
            assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), (p0, p1, k)
        assert np.isfinite(x['trans']).all()
    assert open(f'{a}/{rdir}/pre.log').read() == open(f'{b}/{rdir}/pre.log').read()


def test_run_distributed_and_registrar_under_sc2(tmp_path):
    """run_distributed.evaluate with cfg.ET = 'sc2' at world size 1 registers the synthetic scene and writes sc2/ archives; Registrar over an
    engine without an ET network registers a pair of raw clouds"""
    import _sparse_conv_oracle as SO
    from test_sparse_conv_oracle import NARROW
    from test_hip_sparse_conv import device_model
    from roreg_amd import run_distributed as RD_
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.register import Registrar
    cfg, gf, ds = _scene_and_nets(tmp_path, testset='synth')
    ds.write_inputs(cfg.output_cache_fn)
    out = RD_.evaluate(cfg, {'wholesetname': 'synth', 'scene0': ds}, RegistrationEngine(cfg, gf, None), rank=0, world=1, seed=3)
    assert out['pairs'] == 3 and out['rr'] == 1.0
    assert len(glob.glob(f'{cfg.output_cache_fn}/{ds.name}/match_{KEYNUM}/sc2/1000iters/*.npz')) == 3
    model = device_model(SO.random_state_dict(12, conv1_kernel_size=3, **NARROW), 3, **NARROW)
    p0, p1, _ = synth.make_dense_pair(3, 2000)
    r = Registrar(RegistrationEngine(cfg, gf, None), model, voxel_size=0.05, rot_batch=12, n_keypoints=64).pair(p0, p1, seed=5, keynum=48, max_iter=100)
    assert r.trans.shape == (4, 4) and r.n_match >= 0 and r.keypoints0.shape == (64, 3)


def test_yohoo_is_untouched_on_the_golden_pair(tmp_path):
    """the one-shot estimator on the recorded config-1 pair: the golden matches and transform, and numpy's global generator where the reference's
    calls leave it (two shuffles in the matcher, one in the estimator) -- what the parent commit gives"""
    from conftest import load_golden
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.network import name2network
    z = load_golden('pipeline_config1')
    cfg = default_config(output_cache_fn=f'{tmp_path}/cache', model_fn=f'{tmp_path}/ckpt', base_dir=str(tmp_path), SO3_related_files=None, keynum=256, ET='yohoo')
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    ds = synth.config1_pair()
    np.random.seed(1234)
    res = RegistrationEngine(cfg, gf, et).run_scene({0: ds.feats[0], 1: ds.feats[1]}, {0: ds.get_kps('0'), 1: ds.get_kps('1')}, ds.pair_ids, keynum=256,
                                                   max_iter=1000, keep_matches=True)
    after = np.random.get_state()
    assert np.array_equal(res[0].matches.cpu().numpy(), z['match_0_1']) and np.abs(res[0].trans - z['trans_0_1']).max() < 1e-6
    np.random.seed(1234)
    for n in (256, 256, res[0].n_match):
        idx = np.arange(n); np.random.shuffle(idx)
    left = np.random.get_state()
    assert np.array_equal(after[1], left[1]) and after[2:] == left[2:]


def test_dropin_end_to_end_with_et_sc2(tmp_path, monkeypatch):
    """an unchanged Test.py flow (parse flags -> yoho_evaluator(cfg).run()) with --ET sc2 through the drop-in aliases, on a demo-layout dataset
    with a GF checkpoint only: registers the pair and labels its results.log block sc2"""
    import sys
    from roreg_amd import dropin
    from roreg_amd.network import name2network
    root = str(tmp_path)
    scene = synth.make_scene(31, n_clouds=2, n_kpts=160, overlap=0.7, name='demo/kitchen')
    base = f'{root}/data/origin_data/demo/kitchen'
    os.makedirs(f'{base}/PointCloud'); os.makedirs(f'{base}/Keypoints')
    rng = np.random.default_rng(0)
    for i in range(2):
        kps = scene.get_kps(str(i)).astype(np.float32)
        pts = np.concatenate([rng.uniform(0, 3, (300, 3)).astype(np.float32), kps], 0)          # keypoints are indices into the cloud
        rec = np.zeros(pts.shape[0], dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4')])
        rec['x'], rec['y'], rec['z'] = pts[:, 0], pts[:, 1], pts[:, 2]
        hdr = f'ply\nformat binary_little_endian 1.0\nelement vertex {pts.shape[0]}\nproperty float x\nproperty float y\nproperty float z\nend_header\n'
        open(f'{base}/PointCloud/cloud_bin_{i}.ply', 'wb').write(hdr.encode() + rec.tobytes())
        np.savetxt(f'{base}/Keypoints/cloud_bin_{i}Keypoints.txt', np.arange(300, 300 + kps.shape[0]))
    gt = scene.get_transform('0', '1')
    with open(f'{base}/PointCloud/gt.log', 'w') as f:
        f.write('0\t 1\t 2\t\n' + ''.join('\t'.join(repr(float(v)) for v in gt[r]) + '\n' for r in range(3)) + '0.0\t0.0\t0.0\t1.0\n')
    cache = f'{root}/data/YOHO_FCGF/Testset'
    scene.write_inputs(cache)
    net = name2network['GF_test'](default_config()); synth.seeded_state_dict(net, 101)
    os.makedirs(f'{root}/ckpt/GF')
    torch.save({'best_para': 0, 'network_state_dict': net.state_dict()}, f'{root}/ckpt/GF/model_best.pth')
    saved = {k: sys.modules.get(k) for k in dropin._ALIASES}
    monkeypatch.setattr(sys, 'argv', ['Test.py', '--testset', 'demo', '--ET', 'sc2', '--keynum', '160', '--max_iter', '1000',
                                      '--base_dir', f'{root}/data', '--origin_data_dir', f'{root}/data/origin_data', '--output_cache_fn', cache,
                                      '--model_fn', f'{root}/ckpt', '--SO3_related_files', f'{root}/no_such_dir'])
    try:
        dropin.install()
        import parses.parses_test as parses_test
        from test.evaluator import yoho_evaluator
        config, _ = parses_test.get_config()
        np.random.seed(3)
        out = yoho_evaluator(config).run()
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    log = open(f'{root}/data/results.log').read()
    assert log.startswith('demo-yoho_des-nodet-matmul-sc2-160keys-1000iters\n') and 'registration recall(predator)    : 1.00000' in log
    assert out['fmr'] == 1.0 and out['rr'] == 1.0
    T = np.load(f'{cache}/demo/kitchen/match_160/sc2/1000iters/0-1.npz')['trans']
    assert np.abs(T[:3] - gt).max() < 1e-3
    assert not os.path.exists(f'{root}/ckpt/ET') and not glob.glob(f'{cache}/demo/kitchen/match_160/DR_index/*.npy')
