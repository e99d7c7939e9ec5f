"""Dense pair evaluation on the device (csrc/icp.hip "v6g": overlap, RMSE, information matrix) against its numpy restatement
(tests/_dense_eval_oracle.py).  GPU only.

Tolerances: counts and assignments exact; every sum within n 2^-52 sum |term| + 4 ulp of math.fsum (the oracle computes that bound: it holds
for any order of summation and nothing in it is measured from the device).  sum x and the off-diagonal of sum x x^T are read back from
Lambda exactly (Lambda_tr = -2 [sum x]x and Lambda_rr's off-diagonal = -4 sum x_i x_j are exact scalings); the diagonal of sum x x^T enters
Lambda as 4 (sum x_j^2 + sum x_k^2), checked against the bound of that sum of 2 n terms."""
import filecmp
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
import _dense_eval_cases as K
import _dense_eval_oracle as E
import _icp_cases as C
import _icp_oracle as O
from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu


def _dev(T):
    return torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()


def _grid(p, d):
    from roreg_amd import hip
    return hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _run(pairs, d, grid_d=None):
    """pairs [(cloud 0, cloud 1, T)] -> rows [(stats [8], info [6,6], status, assign01, assign10)] of one batch"""
    from roreg_amd import hip
    grids = {}

    def g(p, r):
        if (id(p), r) not in grids:
            grids[(id(p), r)] = _grid(p, r)
        return grids[(id(p), r)]
    stats, info, status, a01, a10 = hip.icp_eval_batch([(g(a, d if grid_d is None else grid_d), g(b, d), _dev(T)) for a, b, T in pairs], d, want_assign=True)
    stats, info, status = stats.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy()
    return [(stats[i], info[i], int(status[i]), a01[i].cpu().numpy(), a10[i].cpu().numpy()) for i in range(len(pairs))]


def _check(row, ref, n_tgt, n_src, name=''):
    from roreg_amd import hip
    stats, info, status, a01, a10 = row
    print(f'{name}: n01 {int(stats[0])} (oracle {ref.n01}), n10 {int(stats[1])} ({ref.n10}), S01 {stats[6]!r} ({ref.S01[0]!r} +- {ref.S01[1]:.2e}), '
          f'S10 {stats[7]!r} ({ref.S10[0]!r} +- {ref.S10[1]:.2e}), max |Lambda - oracle| / bound '
          f'{(np.abs(info - ref.info) / np.maximum(ref.info_bound, 1e-300)).max():.3f}')
    assert hip.ICP_EVAL_STATUS[status] == ref.status
    assert np.array_equal(a01, ref.assign01) and np.array_equal(a10, ref.assign10), name
    assert stats[0] == ref.n01 and stats[1] == ref.n10
    assert abs(stats[6] - ref.S01[0]) <= ref.S01[1] and abs(stats[7] - ref.S10[0]) <= ref.S10[1]
    # the moments, read back from Lambda
    sx = (info[1, 5] / 2.0, info[2, 3] / 2.0, info[0, 4] / 2.0)
    for i in range(3):
        assert abs(sx[i] - ref.sx[i][0]) <= ref.sx[i][1], (name, i)
    for (i, j) in ((0, 1), (0, 2), (1, 2)):
        assert abs(-info[3 + i, 3 + j] / 4.0 - ref.M[(i, j)][0]) <= ref.M[(i, j)][1], (name, i, j)
    assert (np.abs(info - ref.info) <= ref.info_bound).all(), name
    assert np.array_equal(info, info.T) and np.array_equal(info[:3, :3], ref.n01 * np.eye(3))
    for got, S, n in ((stats[4], ref.S01, ref.n01), (stats[5], ref.S10, ref.n10)):
        if n:
            assert abs(got - np.sqrt(S[0] / n)) <= E.rmse_bound(S, n), name
        else:
            assert np.isnan(got)
    for got, n, m in ((stats[2], ref.n10, n_tgt), (stats[3], ref.n01, n_src)):
        assert (np.isnan(got) if m == 0 else got == n / m), name


@pytest.mark.parametrize('d', K.PAIR_DISTS)
def test_one_pair(d):
    p0, p1, Tg = K.pair()
    ref = K.pair_reference(d)
    assert abs(ref.overlap1 - {0.02: 0.281, 0.05: 0.358, 0.1: 0.495}[d]) < 1e-3 and abs(ref.overlap0 - {0.02: 0.277, 0.05: 0.359, 0.1: 0.494}[d]) < 1e-3
    _check(_run([(p0, p1, Tg)], d)[0], ref, p0.shape[0], p1.shape[0], f'd = {d}')


def test_chunk_edges_in_both_directions():
    pairs = C.chunk_pairs()
    rows = _run([(q, p, T0) for _, q, p, T0 in pairs], C.CHUNK_DIST)
    for (name, q, p, _), row, ref in zip(pairs, rows, K.chunk_reference()):
        _check(row, ref, q.shape[0], p.shape[0], name)


def test_thresholds_and_the_target_grids_radius():
    """At exactly max_dist: in; one step beyond: out -- in both directions (both role orders of the family); the rows do not depend on the
    radius cloud 0's grid was built for."""
    pairs = K.threshold_pairs()
    rows = {gd: _run([(a, b, np.eye(4)) for _, a, b in pairs], C.THR_DIST, grid_d=gd) for gd in C.THR_GRID_DISTS}
    for k, ((name, a, b), ref) in enumerate(zip(pairs, K.threshold_reference())):
        _check(rows[C.THR_DIST][k], ref, a.shape[0], b.shape[0], name)
        for gd in C.THR_GRID_DISTS[1:]:
            for x, y in zip(rows[C.THR_DIST][k], rows[gd][k]):
                assert _bits(x) == _bits(y), (name, gd)
    for base in C.THR_BASES:
        kind = C.threshold_case(base)[2]
        plain, swapped = [rows[C.THR_DIST][k] for k, (n, _, _) in enumerate(pairs) if n.startswith(f'base{base:g}')]
        assert (plain[3][kind == C.KIND_BEYOND] == -1).all() and (plain[3][kind == C.KIND_FACE] >= 0).all()
        assert (swapped[4][kind == C.KIND_BEYOND] == -1).all() and (swapped[4][kind == C.KIND_FACE] >= 0).all()


def test_batch_independence():
    """The same pairs alone, in one batch, permuted and in sub-batches: bit-identical rows."""
    from roreg_amd import hip
    d = 0.07
    clouds, pairs = [], []
    for seed, n in ((21, 3000), (22, 5000), (23, 8000), (24, 700)):
        p0, p1, Tg = synth.make_dense_pair(seed, n)
        clouds += [p0, p1]
        pairs += [(len(clouds) - 2, len(clouds) - 1, O.perturb(Tg, 1.0, 0.02, seed)), (len(clouds) - 1, len(clouds) - 2, np.linalg.inv(Tg))]
    pairs += [(0, 3, np.eye(4)), (6, 6, np.eye(4))]
    grids = [_grid(c, d) for c in clouds]
    items = [(grids[i], grids[j], _dev(T)) for i, j, T in pairs]

    def run(sel):
        out = hip.icp_eval_batch([items[k] for k in sel], d, want_assign=True)
        s, L, st = (v.cpu().numpy() for v in out[:3])
        return {k: (_bits(s[q]), _bits(L[q]), int(st[q]), _bits(out[3][q].cpu().numpy()), _bits(out[4][q].cpu().numpy())) for q, k in enumerate(sel)}
    whole = run(list(range(len(items))))
    assert whole == run(list(range(len(items))))
    perm = [int(v) for v in np.random.default_rng(5).permutation(len(items))]
    assert run(perm) == whole
    for k in range(len(items)):
        assert run([k])[k] == whole[k], k
    for sel in ([0, 5, 9], [8, 2], [1, 3, 4, 6, 7]):
        sub = run(sel)
        assert all(sub[k] == whole[k] for k in sel)


def test_agrees_with_one_icp_iteration():
    """n01 is icp_batch(max_iter=1)'s inlier count and rmse01 its rmse (both are sqrt(sum d2 / n) of the same correspondences, summed in
    two ways: each within the oracle's bound of the exact value)."""
    from roreg_amd import hip
    p0, p1, Tg = K.pair()
    T0 = O.perturb(Tg, 1.0, 0.02, 5)
    for d in (0.05, 0.1):
        ref = E.evaluate(p0, p1, T0, d)
        g0, g1 = _grid(p0, d), _grid(p1, d)
        _, iters, inl, rmse, _, assign = hip.icp_batch([(g0, g1, _dev(T0))], d, max_iter=1, want_assign=True)
        stats, _, _, a01, _ = hip.icp_eval_batch([(g0, g1, _dev(T0))], d, want_assign=True)
        stats = stats.cpu().numpy()[0]
        assert int(iters[0]) == 1 and int(inl[0]) == stats[0] == ref.n01 and torch.equal(assign[0], a01[0])
        assert abs(float(rmse[0]) - stats[4]) <= 2.0 * E.rmse_bound(ref.S01, ref.n01)


def test_edges():
    from roreg_amd import dense_eval
    p0, p1, Tg = K.pair()
    Tn = np.full((4, 4), np.nan); Tn[3] = [0, 0, 0, 1]
    Ti = Tg.copy(); Ti[1, 3] = np.inf
    r = dense_eval.evaluate([(p0, p1, Tn), (p0, p1, Tg), (p0, p1, Ti)], max_dist=0.05)
    for e in (r[0], r[2]):
        assert e.status == 'nonfinite' and e.n01 == 0 == e.n10 and np.isnan(e.rmse01) and np.isnan(e.rmse10) and not e.info.any()
        assert e.overlap0 == 0.0 == e.overlap1
    assert r[1].status == 'ok' and r[1].n01 == K.pair_reference(0.05).n01 and r[1].n10 == K.pair_reference(0.05).n10
    for name, a, b, T in K.disjoint_pairs():
        e = dense_eval.evaluate(a, b, T, max_dist=K.DISJOINT_DIST)
        assert e.status == 'ok' and e.n01 == 0 == e.n10 and np.isnan(e.rmse01) and np.isnan(e.rmse10) and not e.info.any() and e.overlap0 == 0.0 == e.overlap1, name
    for shift in (1e6, 1e30, 1e300):
        far = Tg.copy(); far[:3, 3] += shift
        e = dense_eval.evaluate(p0, p1, far, max_dist=0.05)
        assert e.status == 'ok' and e.n01 == 0 == e.n10 and not e.info.any(), shift
    # one-point clouds
    one = p0[:1]
    e, m0, m1 = dense_eval.evaluate(one, one, np.eye(4), max_dist=0.05, overlap_masks=True)
    ref = E.evaluate(one, one, np.eye(4), 0.05)
    assert e.n01 == 1 == e.n10 and e.overlap0 == 1.0 == e.overlap1 and e.rmse01 == 0.0 == e.rmse10 and m0.all() and m1.all()
    assert (np.abs(e.info - ref.info) <= ref.info_bound).all()
    e = dense_eval.evaluate(one, p1, Tg, max_dist=0.05)
    ref = E.evaluate(one, p1, Tg, 0.05)
    assert (e.n01, e.n10) == (ref.n01, ref.n10)
    # empty clouds: overlaps of an empty cloud are NaN
    none = np.zeros((0, 3), np.float32)
    e = dense_eval.evaluate(p0, none, Tg, max_dist=0.05)
    assert e.status == 'ok' and e.n01 == 0 == e.n10 and np.isnan(e.overlap1) and e.overlap0 == 0.0
    e = dense_eval.evaluate(none, none, Tg, max_dist=0.05)
    assert e.n01 == 0 == e.n10 and np.isnan(e.overlap1) and np.isnan(e.overlap0)
    # an identical pair under the identity
    e, m0, m1 = dense_eval.evaluate(p0, p0, np.eye(4), max_dist=0.05, overlap_masks=True)
    ref = E.evaluate(p0, p0, np.eye(4), 0.05)
    assert ref.n01 == p0.shape[0] and e.n01 == p0.shape[0] == e.n10 and e.overlap0 == 1.0 == e.overlap1 and e.rmse01 == 0.0 == e.rmse10 and m0.all() and m1.all()
    assert (np.abs(e.info - ref.info) <= ref.info_bound).all() and e.info[0, 0] == p0.shape[0]
    # the masks are the oracle's assignments
    (e, m0, m1), = dense_eval.evaluate([(p0, p1, Tg)], max_dist=0.05, overlap_masks=True)
    ref = K.pair_reference(0.05)
    assert np.array_equal(m1, ref.assign01 >= 0) and np.array_equal(m0, ref.assign10 >= 0) and m1.sum() == e.n01 and m0.sum() == e.n10


def _engine():
    from roreg_amd.engine import RegistrationEngine
    return RegistrationEngine(default_config(), None, None)


def test_engine_evaluate_many_is_dense_eval():
    from roreg_amd import dense_eval, hip
    from roreg_amd.engine import CloudState
    eng = _engine()
    clouds, poses = K.scene()
    states = [eng.attach_points(CloudState(before=None), c) for c in clouds]
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (0, 4)]
    Ts = [K.relative(poses, i, j) for i, j in pairs]
    stats, info, status = eng.evaluate_many([(states[i], states[j], _dev(T)) for (i, j), T in zip(pairs, Ts)], K.SCENE_DIST)
    stats, info, status = stats.cpu().numpy(), info.cpu().numpy(), status.cpu().numpy()
    want = dense_eval.evaluate([(clouds[i], clouds[j], T) for (i, j), T in zip(pairs, Ts)], max_dist=K.SCENE_DIST)
    for k, w in enumerate(want):
        assert (int(stats[k, 0]), int(stats[k, 1])) == (w.n01, w.n10) and hip.ICP_EVAL_STATUS[int(status[k])] == w.status
        assert _bits(stats[k, 2:6]) == _bits(np.array([w.overlap0, w.overlap1, w.rmse01, w.rmse10])) and _bits(info[k]) == _bits(w.info)
    assert want[0].n01 > 500 and want[2].n01 == 81 == want[2].n10 and want[4].n01 == 0


def test_overlap_matrix_equals_every_ordered_pair_unfiltered():
    from roreg_amd import dense_eval
    from roreg_amd.engine import CloudState
    eng = _engine()
    clouds, poses = K.scene()
    states = [eng.attach_points(CloudState(before=None), c) for c in clouds]
    calls = []
    many = eng.evaluate_many
    eng.evaluate_many = lambda items, max_dist: (calls.append(len(items)), many(items, max_dist))[1]
    counts, overlap = eng.overlap_matrix(states, poses, K.SCENE_DIST)
    order = [(i, j) for i in range(6) for j in range(6) if i != j]
    want = dense_eval.evaluate([(clouds[i], clouds[j], K.relative(poses, i, j)) for i, j in order], max_dist=K.SCENE_DIST)
    for (i, j), w in zip(order, want):
        assert counts[i, j] == w.n01 and _bits(np.float64(overlap[i, j])) == _bits(np.float64(w.overlap1)), (i, j)
    assert all(counts[i, i] == 2000 and overlap[i, i] == 1.0 for i in range(6))
    assert counts[2, 3] == 81 == counts[3, 2] and counts[0, 1] > 500
    assert counts[4].sum() == 2000 == counts[:, 4].sum() and counts[5].sum() == 2000 == counts[:, 5].sum()      # the far clouds meet nobody
    assert len(calls) == 1 and calls[0] <= 30 - 16                               # the far clouds' pairs got no task
    print('tasks', calls, 'of 30 ordered pairs')


def _dense_scene(ds, n, seed):
    """Dense clouds consistent with a synth.make_scene scene's poses: cloud c sees world points x_w at R_g^T (x_w - t_c)."""
    from roreg_amd.group import tables
    rng = np.random.default_rng(seed)
    world = synth.make_dense_pair(seed, 3 * n, noise=0.0)[0].astype(np.float64) + np.array([2.0, 1.5, 0.0])
    out = {}
    for c, (g, t) in enumerate(ds.poses):
        x = world[rng.permutation(world.shape[0])[:n]] + rng.normal(0, 0.002, (n, 3))
        out[c] = np.ascontiguousarray((x - t) @ tables().R[g], np.float32)
    return out


def test_run_distributed_computes_the_information_matrices(tmp_path):
    """run_distributed.evaluate at world size 1 on a synthetic scene with get_pc and a gt.log but no gt.info: without gt_info= rr_predator
    is NaN and the files are what they were; with it the value is RR_cal.benchmark's on the oracle's matrices, the .info lands under
    output_cache_fn and nothing appears under the dataset directory."""
    from roreg_amd import run_distributed as RD_
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.network import name2network
    from roreg_amd.test.estimator import pre_log_entry
    from roreg_amd.utils import RR_cal
    z = load_golden('pipeline_mutual_yohoo')
    d = 0.05
    outs, cfgs, dirs = {}, {}, {}
    for kind in ('plain', 'info'):
        root = tmp_path / kind
        root.mkdir()
        cfg = default_config(output_cache_fn=f'{root}/cache', model_fn=f'{root}/ckpt', base_dir=str(root), SO3_related_files=None, keynum=int(z['keynum']),
                             bs_GF=50, bs_ET=40, ET='yohoo', testset='synth')
        gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
        et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
        ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
        ds.write_inputs(cfg.output_cache_fn)
        data = root / 'data' / 'synth' / 'scene0'
        data.mkdir(parents=True)
        ds.gt_dir = f'{data}/gt.log'
        with open(ds.gt_dir, 'w') as f:
            for a, b in ds.pair_ids:
                f.write(pre_log_entry(a, b, len(ds.pc_ids), np.concatenate([ds.get_transform(a, b).astype(np.float64), [[0, 0, 0, 1]]])))
        dense = _dense_scene(ds, 8000, 31)
        ds.get_pc = lambda i, dense=dense: dense[int(i)]
        datasets = {'wholesetname': 'synth', 'scene0': ds}
        outs[kind] = RD_.evaluate(cfg, datasets, RegistrationEngine(cfg, gf, et), rank=0, world=1, seed=3, **({'gt_info': dict(max_dist=d)} if kind == 'info' else {}))
        cfgs[kind], dirs[kind] = cfg, data
        assert os.listdir(data) == ['gt.log']
    plain, info = outs['plain'], outs['info']
    assert np.isnan(plain['rr_predator']) and np.isfinite(info['rr_predator']) and set(plain) == set(info)
    for k in plain:
        assert k == 'rr_predator' or plain[k] == info[k] or (np.isnan(plain[k]) and np.isnan(info[k])), k
    c0, c1 = (f"{cfgs[k].output_cache_fn}/{ds.name}" for k in ('plain', 'info'))
    sub = f'match_{cfg.keynum}/yohoo/{cfg.max_iter}iters'
    files = sorted(os.listdir(f'{c0}/{sub}'))
    assert files == sorted(os.listdir(f'{c1}/{sub}')) and len(files) == len(ds.pair_ids) + 1
    for f in files:
        if f.endswith('.npz'):
            a, b = np.load(f'{c0}/{sub}/{f}'), np.load(f'{c1}/{sub}/{f}')
            assert _bits(a['trans']) == _bits(b['trans']) and int(a['recalltime']) == int(b['recalltime'])
        else:
            assert filecmp.cmp(f'{c0}/{sub}/{f}', f'{c1}/{sub}/{f}', shallow=False)
    assert sorted(set(os.listdir(c1)) - set(os.listdir(c0))) == ['gt_info_0.05.info']
    assert not os.path.exists(f'{cfgs["plain"].output_cache_fn}/synth/Eval_results')
    # the written matrices against the oracle's, and the recall they give
    n, got = RR_cal.read_trajectory_info(f'{c1}/gt_info_0.05.info')
    assert n == len(ds.pc_ids) and got.shape == (len(ds.pair_ids), 6, 6)
    refs = []
    for (a, b), L in zip(ds.pair_ids, got):
        T = np.eye(4); T[:3] = ds.get_transform(a, b).astype(np.float64)
        ref = E.evaluate(dense[int(a)], dense[int(b)], T, d)
        assert ref.n01 > 100 and (np.abs(L - ref.info) <= ref.info_bound).all()
        refs.append(ref.info)
    path = tmp_path / 'oracle.info'
    RR_cal.write_trajectory_info(str(path), [(int(a), int(b)) for a, b in ds.pair_ids], len(ds.pc_ids), refs)
    want = RR_cal.benchmark(cfgs['info'], {'wholesetname': 'synth', 'scene0': ds}, cfg.keynum, cfg.max_iter, yoho_sign='yohoo', info_files={ds.name: str(path)})[0]
    assert info['rr_predator'] == float(want)
    log0 = open(f'{cfgs["plain"].base_dir}/results.log').read(); log1 = open(f'{cfgs["info"].base_dir}/results.log').read()
    assert [l for l in log0.splitlines() if 'predator' not in l] == [l for l in log1.splitlines() if 'predator' not in l]
