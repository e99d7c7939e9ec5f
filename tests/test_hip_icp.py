"""Dense ICP refinement on the device (csrc/icp.hip) against its numpy restatement (tests/_icp_oracle.py).  GPU only."""
import filecmp
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from conftest import load_golden
import _icp_oracle as O
from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu


def _dev(T):
    return torch.from_numpy(np.ascontiguousarray(T, np.float64)).cuda()


def _grid(p, d):
    from roreg_amd import hip
    return hip.IcpGrid(torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 3)).cuda(), d)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def conv_pair():
    return synth.make_dense_pair(O.CONV_SEED, O.CONV_N)


def test_grid_is_a_counting_sort_in_canonical_order():
    """The grid's records are the cloud's points sorted by cell, ascending original row inside a cell; the cell starts delimit them; two
    builds give the same bytes (the fill's atomics decide nothing)."""
    p0 = synth.make_dense_pair(8, 30000)[0]
    p0[200:260] = p0[7000:7060]                                # duplicated points share a cell
    g = _grid(p0, 0.1)
    xyz, rows = (t.cpu().numpy() for t in g.records())
    assert np.array_equal(np.sort(rows), np.arange(p0.shape[0])) and np.array_equal(xyz, p0[rows])
    d = g.desc
    c = np.floor((xyz.astype(np.float64) - d['origin'][0]) * (1.0 / d['edge'][0])).astype(np.int64)
    assert (c >= 1).all() and (c <= np.array(d['dims'][0]) - 2).all()          # one cell of padding around the box
    cid = (c[:, 2] * d['dims'][0][1] + c[:, 1]) * d['dims'][0][0] + c[:, 0]
    assert (np.diff(cid) >= 0).all()
    assert (np.diff(rows)[np.diff(cid) == 0] > 0).all()
    starts = g.cell_starts().cpu().numpy()
    assert starts[0] == 0 and starts[-1] == p0.shape[0]
    assert np.array_equal(starts, np.concatenate([[0], np.cumsum(np.bincount(cid, minlength=int(d['cells'][0])))]))
    assert torch.equal(g.buf, _grid(p0, 0.1).buf)


def test_one_iteration_from_a_given_transform():
    """Assignments (with planted exact ties: the lowest row wins) and the inlier count equal the oracle's; centroids and H to 1e-12."""
    from roreg_amd import hip
    p0, p1, Tg = synth.make_dense_pair(5, 20000)
    p0[100:1100] = p0[5000:6000]                               # target rows 100.. duplicate rows 5000..: an exact tie for every query near them
    T0 = O.perturb(Tg, 1.0, 0.02, 5)
    for d in (0.05, 0.1):
        want = O.iterate(p0.astype(np.float64), p1.astype(np.float64), T0[:3, :3], T0[:3, 3], d)
        assert np.isin(want['assign'], np.arange(100, 1100)).sum() > 50 and not np.isin(want['assign'], np.arange(5000, 6000)).any()
        T, iters, inl, rmse, status, assign, stats = hip.icp_batch([(_grid(p0, d), _grid(p1, d), _dev(T0))], d, max_iter=1, want_assign=True, want_stats=True)
        assign = assign[0].cpu().numpy(); stats = stats[0].cpu().numpy()
        print(f'd = {d}: {int(inl[0])} inliers (oracle {want["n"]}), {int((assign != want["assign"]).sum())} assignments differ')
        assert np.array_equal(assign, want['assign'])
        assert int(inl[0]) == want['n'] == int(stats[0]) and int(iters[0]) == 1
        cq, cp, H = stats[1:4], stats[4:7], stats[7:16].reshape(3, 3)
        err = (np.abs(cq - want['cq']).max() / np.abs(want['cq']).max(), np.abs(cp - want['cp']).max() / np.abs(want['cp']).max(),
               np.abs(H - want['H']).max() / np.abs(want['H']).max())
        print('relative differences of c_q, c_p, H:', err)
        assert max(err) <= 1e-12
        assert abs(float(rmse[0]) - np.sqrt(want['sum_d2'] / want['n'])) <= 1e-12
        new = O.solve(want['H'], want['cq'], want['cp'])          # the update itself: the sums' 1e-12 times the 3x3 problem's conditioning (<= 100)
        assert np.abs(T[0].cpu().numpy()[:3, :3] - new[0]).max() <= 1e-10 and np.abs(T[0].cpu().numpy()[:3, 3] - new[1]).max() <= 1e-10


@pytest.mark.parametrize('d', [0.05, 0.1])
def test_full_runs_end_at_the_oracles_transform(conv_pair, d):
    """From the ground truth perturbed by 3 degrees / 5 cm and by 5 degrees / 10 cm, max_iter = 50: every entry of the final T within 1e-9
    of the oracle's and the same number of iterations.  (Reordering a float64 sum of <= 1e5 terms is worth ~1e-11 relative, a factor 100 for
    the conditioning of the 3x3 problem; an assignment flips only if a point sits within ~1e-13 of the threshold or of a tie -- a larger
    difference means a wrong assignment, not a loose tolerance.)"""
    from roreg_amd import icp
    p0, p1, Tg = conv_pair
    starts = [O.perturb(Tg, deg, shift, O.CONV_SEED) for deg, shift in O.CONV_STARTS]
    got = icp.refine([(p0, p1, T0) for T0 in starts], max_dist=d, max_iter=50)
    for T0, g in zip(starts, got):
        want = O.icp(p0, p1, T0, d, max_iter=50)
        e = O.pose_error(g.T, Tg)
        print(f'd = {d}: device {g.iters} iterations, {g.inliers} inliers, rmse {g.rmse * 1e3:.3f} mm, {g.status}, {e[0]:.4f} deg / {e[1] * 1e3:.3f} mm from the '
              f'ground truth; oracle {want.iters}, {want.inliers}, {want.rmse * 1e3:.3f} mm, {want.status}; max |T - T_oracle| = {np.abs(g.T - want.T).max():.3e}')
        assert g.iters == want.iters and g.status == want.status and g.inliers == want.inliers
        assert np.abs(g.T - want.T).max() <= 1e-9
        assert abs(g.rmse - want.rmse) <= 1e-9
        if d == 0.05:
            assert e[0] < 0.05 and e[1] < 0.002


def test_grid_reuse_and_batch_independence():
    """A pair refined alone, inside a batch of many pairs, and inside the same batch in another order: bit-identical T, iters, inliers,
    rmse; two runs in a row too.  Grids are shared by the pairs that use the same cloud, as a target or as a source."""
    from roreg_amd import hip
    d = 0.07
    clouds, pairs = [], []
    for seed, n in ((21, 6000), (22, 9000), (23, 20000), (24, 1500)):
        p0, p1, Tg = synth.make_dense_pair(seed, n)
        g0, g1 = _grid(p0, d), _grid(p1, d)
        T0 = O.perturb(Tg, 2.0, 0.04, seed)
        pairs.append((g0, g1, _dev(T0)))
        pairs.append((g1, g0, _dev(np.linalg.inv(T0))))        # the same two grids in the other roles
    pairs.append((pairs[0][0], pairs[0][0], _dev(O.perturb(np.eye(4), 1.0, 0.02, 9))))       # a cloud against itself
    Tn = np.full((4, 4), np.nan); Tn[3] = [0, 0, 0, 1]
    pairs.append((pairs[2][0], pairs[2][1], _dev(Tn)))

    def run(order):
        out = hip.icp_batch([pairs[q] for q in order], d, max_iter=25)
        return [v.cpu().numpy() for v in out]

    full = list(range(len(pairs)))
    a = run(full)
    b = run(full)
    perm = [int(q) for q in np.random.default_rng(4).permutation(len(pairs))]
    c = run(perm)
    assert (a[1][:8] > 1).all() and (a[2][:8] > 100).all()           # real work: several iterations, hundreds of inliers
    for x, y in zip(a, b):
        assert _same_bits(x, y)
    for x, y in zip(a, c):
        assert _same_bits(x[perm], y)
    for q in (0, 3, 5, 8, 9):
        alone = run([q])
        for x, y in zip(a, alone):
            assert _same_bits(x[q:q + 1], y), q
    sub = [5, 4, 0]
    s = run(sub)
    for x, y in zip(a, s):
        assert _same_bits(x[sub], y)


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


def _cfg_and_nets(tmp_path, z, **kw):
    from roreg_amd.network import name2network
    root = str(tmp_path)
    cfg = default_config(output_cache_fn=f'{root}/cache', model_fn=f'{root}/ckpt', base_dir=root, SO3_related_files=None,
                         keynum=int(z['keynum']), bs_GF=50, bs_ET=40, **kw)
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    return cfg, gf, et


def test_engine_carries_the_refinement_and_changes_nothing_else(tmp_path):
    """run_scene with points= / icp=: trans, matches, recalltime and the stage files are what they are without; trans_icp is bitwise what
    icp.refine returns when started from trans."""
    from roreg_amd import icp
    from roreg_amd.engine import RegistrationEngine, StageFileWriter
    z = load_golden('pipeline_mutual_yohoo')
    cfg, gf, et = _cfg_and_nets(tmp_path, z, ET='yohoo')
    keynum = int(z['keynum'])
    ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
    dense = _dense_scene(ds, 8000, 31)
    keys = [ds.get_kps(i) for i in ds.pc_ids]
    opts = dict(max_dist=0.1, max_iter=20)
    runs = {}
    for kind, extra in (('plain', {}), ('icp', dict(points=dense, icp=opts))):
        cfg2 = NS(**{**vars(cfg), 'output_cache_fn': f'{tmp_path}/cache_{kind}'})
        eng = RegistrationEngine(cfg2, gf, et)
        w = StageFileWriter(cfg2, ds.name, keynum)
        np.random.seed(99)
        runs[kind] = eng.run_scene(ds.feats, keys, ds.pair_ids, keynum=keynum, max_iter=1000, keep_matches=True, writer=w, **extra)
        w.close()
    for a, b in zip(runs['plain'], runs['icp']):
        assert (a.id0, a.id1, a.n_match, a.recalltime) == (b.id0, b.id1, b.n_match, b.recalltime)
        assert np.array_equal(a.trans, b.trans, equal_nan=True) and torch.equal(a.matches, b.matches)
        assert a.trans_icp is None and a.icp_iters is None and a.icp_inliers is None and a.icp_rmse is None
    dirs = [f'{tmp_path}/cache_{kind}/{ds.name}/match_{keynum}' for kind in ('plain', 'icp')]
    n_files = 0
    for base, _, files in os.walk(dirs[0]):
        for f in files:
            n_files += 1
            assert filecmp.cmp(os.path.join(base, f), os.path.join(dirs[1] + base[len(dirs[0]):], f), shallow=False), f
    assert n_files >= 3 * len(ds.pair_ids) and sum(len(f) for _, _, f in os.walk(dirs[1])) == n_files
    want = icp.refine([(dense[int(r.id0)], dense[int(r.id1)], r.trans) for r in runs['icp']], **opts)
    for r, w_ in zip(runs['icp'], want):
        print(r.id0, r.id1, r.icp_iters, r.icp_inliers, r.icp_rmse, r.icp_status)
        assert _same_bits(r.trans_icp, w_.T) and (r.icp_iters, r.icp_inliers, r.icp_status) == (w_.iters, w_.inliers, w_.status)
        assert _same_bits(np.float64(r.icp_rmse), np.float64(w_.rmse))
    assert any(r.icp_iters >= 1 for r in runs['icp'])               # the refinement ran (a NaN transform would pass through with 0)
    # the engine built one grid per cloud however many pairs use it
    eng2 = RegistrationEngine(cfg, gf, et)
    np.random.seed(99)
    ready = {}
    eng2.run_scene(ds.feats, keys, ds.pair_ids, keynum=keynum, max_iter=1000, points=dense, icp=opts, ready=ready)
    assert all(len(c.grids) == 1 for c in ready.values()) and len(ready) == len(ds.pc_ids)


def _plane(n, seed, tilt=True):
    rng = np.random.default_rng(seed)
    x = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], 1)
    if tilt:
        x = x @ synth.dense_gt(33.0, (2.0, -1.0, 0.5), (0, 0, 0))[:3, :3].T + np.array([0.3, -0.2, 0.7])
    return x.astype(np.float32)


def test_edge_cases_do_not_fault():
    from roreg_amd import hip, icp
    p0, p1, Tg = synth.make_dense_pair(41, 5000)
    I = np.eye(4)
    # a non-finite T0 (the engine's zero-inlier result) passes through, next to a pair that runs normally
    Tn = np.full((4, 4), np.nan); Tn[3] = [0, 0, 0, 1]
    Ti = Tg.copy(); Ti[1, 3] = np.inf
    start = O.perturb(Tg, 2.0, 0.03, 41)
    r = icp.refine([(p0, p1, Tn), (p0, p1, start), (p0, p1, Ti)], max_dist=0.1, max_iter=10)
    for got, T0 in ((r[0], Tn), (r[2], Ti)):
        assert got.status == 'nonfinite' and got.iters == 0 and got.inliers == 0 and np.isnan(got.rmse) and _same_bits(got.T, T0)
    want = O.icp(p0, p1, start, 0.1, max_iter=10)
    assert r[1].iters == want.iters and r[1].inliers == want.inliers and np.abs(r[1].T - want.T).max() <= 1e-9
    # no target point within d of any source point, inside the target's bounding box: no_support, T unchanged
    slab = np.concatenate([_plane(2000, 1, tilt=False), _plane(2000, 2, tilt=False) + np.float32([0, 0, 2])])
    mid = _plane(1500, 3, tilt=False) + np.float32([0, 0, 1])
    got = icp.refine(slab, mid, I, max_dist=0.05)
    assert got.status == 'no_support' and got.iters == 1 and got.inliers == 0 and np.isnan(got.rmse) and _same_bits(got.T, I)
    # source points far outside the target's bounding box, up to coordinates no cell index can hold
    for shift in (100.0, 1e6, 1e30, 1e300):
        far = Tg.copy(); far[:3, 3] += shift
        got = icp.refine(p0, p1, far, max_dist=0.1)
        assert got.status == 'no_support' and got.iters == 1 and got.inliers == 0 and _same_bits(got.T, far), shift
    # two points: fewer than 3 inliers
    got = icp.refine(p0[:2], p0[:2], I, max_dist=0.1)
    assert got.status == 'no_support' and got.inliers == 2 and got.rmse == 0.0 and _same_bits(got.T, I)
    # collinear inliers: rank(H) = 1
    line = np.stack([np.linspace(0, 1, 50), np.zeros(50), np.zeros(50)], 1).astype(np.float32)
    got = icp.refine(line, line, I, max_dist=0.1)
    assert got.status == 'no_support' and got.inliers == 50 and _same_bits(got.T, I)
    # empty clouds, as a source and as a target
    none = np.zeros((0, 3), np.float32)
    for a, b in ((p0, none), (none, p1), (none, none)):
        got = icp.refine(a, b, Tg, max_dist=0.1)
        assert got.status == 'no_support' and got.iters == 1 and got.inliers == 0 and _same_bits(got.T, Tg)
    # coplanar inliers (rank-2 H) still yield a proper rotation, the oracle's
    q = _plane(4000, 5)
    Tp = O.perturb(I, 2.0, 0.03, 6)
    p = ((q[:3000].astype(np.float64) - Tp[:3, 3]) @ Tp[:3, :3]).astype(np.float32)
    got = icp.refine(q, p, I, max_dist=0.1, max_iter=10)
    want = O.icp(q, p, I, 0.1, max_iter=10)
    R = got.T[:3, :3]
    print('coplanar:', got.iters, got.inliers, got.status, 'det', np.linalg.det(R), 'max |T - T_oracle|', np.abs(got.T - want.T).max())
    assert got.status in ('converged', 'max_iter') and got.inliers > 2000
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
    assert got.iters == want.iters and np.abs(got.T - want.T).max() <= 1e-9
    # a bounding box so large that the cell edge doubles (two stray points 40 m out): the same result as the oracle's
    big = np.concatenate([p0, np.float32([[40, 40, 40], [-40, -40, -40]])])
    g = _grid(big, 0.05)
    assert g.edge > 0.05 and int(g.desc['cells'][0]) <= 2 ** 24
    start = O.perturb(Tg, 1.0, 0.02, 43)
    got = icp.refine(big, p1, start, max_dist=0.05, max_iter=8)
    want = O.icp(big, p1, start, 0.05, max_iter=8)
    assert got.iters == want.iters and got.inliers == want.inliers and np.abs(got.T - want.T).max() <= 1e-9
    # a grid built for another radius serves too (the search walks whatever cells the ball meets)
    T, iters, inl, rmse, status = hip.icp_batch([(_grid(p0, 0.3), _grid(p1, 0.02), _dev(start))], 0.05, max_iter=8)
    want = O.icp(p0, p1, start, 0.05, max_iter=8)
    assert int(iters[0]) == want.iters and int(inl[0]) == want.inliers and np.abs(T[0].cpu().numpy() - want.T).max() <= 1e-9


def test_run_distributed_with_and_without_icp(tmp_path):
    """run_distributed.evaluate at world size 1 on a synthetic dataset with get_pc: without icp= the table and the files are what they
    were; with it the second table's transforms are icp.refine's and the '-icp' block is appended to results.log."""
    from roreg_amd import distributed as D, icp, run_distributed as RD_
    from roreg_amd.engine import RegistrationEngine
    z = load_golden('pipeline_mutual_yohoo')
    opts = dict(max_dist=0.1, max_iter=15)
    outs, cfgs = {}, {}
    for kind in ('plain', 'icp'):
        root = tmp_path / kind
        root.mkdir()
        cfg, gf, et = _cfg_and_nets(root, z, ET='yohoo', testset='synth')
        ds = synth.make_scene(int(z['scene_seed']), n_clouds=int(z['n_clouds']), n_kpts=int(z['n_kpts']), overlap=0.6, name='synth/scene0')
        ds.write_inputs(cfg.output_cache_fn)
        ds.gt_dir = f'{root}/nonexistent/{ds.name}/gt.log'
        dense = _dense_scene(ds, 8000, 31)
        ds.get_pc = lambda i, dense=dense: dense[int(i)]
        datasets = {'wholesetname': 'synth', 'scene0': ds}
        outs[kind] = RD_.evaluate(cfg, datasets, RegistrationEngine(cfg, gf, et), rank=0, world=1, seed=3, **({'icp': opts} if kind == 'icp' else {}))
        cfgs[kind] = cfg
    plain, ref = outs['plain'], outs['icp']
    assert 'icp' not in plain and set(plain) == set(ref) - {'icp'}
    for k in plain:
        assert plain[k] == ref[k] or (np.isnan(plain[k]) and np.isnan(ref[k])), k
    d0, d1 = (f"{cfgs[k].output_cache_fn}/{ds.name}/match_{cfgs[k].keynum}" for k in ('plain', 'icp'))
    sub = f'yohoo/{cfgs["plain"].max_iter}iters'
    files = sorted(os.listdir(f'{d0}/{sub}'))
    assert files == sorted(os.listdir(f'{d1}/{sub}')) and len(files) == len(ds.pair_ids) + 1
    for f in files:
        if f.endswith('.npz'):
            a, b = np.load(f'{d0}/{sub}/{f}'), np.load(f'{d1}/{sub}/{f}')
            assert _same_bits(a['trans'], b['trans']) and int(a['recalltime']) == int(b['recalltime'])
        else:
            assert filecmp.cmp(f'{d0}/{sub}/{f}', f'{d1}/{sub}/{f}', shallow=False)
    assert not os.path.exists(f'{d0}/yohoo_icp')
    log0 = open(f'{cfgs["plain"].base_dir}/results.log').read(); log1 = open(f'{cfgs["icp"].base_dir}/results.log').read()
    assert log1.startswith(log0) and log0.count('-icp') == 0
    block = log1[len(log0):].splitlines()
    assert block[0] == log0.splitlines()[0] + '-icp' and len(block) == 4 and block[3].startswith('registration recall(pointdsc)')
    # the second table: the refinement of the first table's transforms
    coarse = {f[:-4]: np.load(f'{d1}/{sub}/{f}')['trans'] for f in files if f.endswith('.npz')}
    want = icp.refine([(dense[int(a)], dense[int(b)], coarse[f'{a}-{b}']) for a, b in ds.pair_ids], **opts)
    rows = {(r['id0'], r['id1']): r for r in D.unpack_rows(ref['icp']['table'])}
    sub_icp = f'yohoo_icp/{cfgs["icp"].max_iter}iters'
    for (a, b), w in zip(ds.pair_ids, want):
        row = rows[(a, b)]
        assert _same_bits(row['trans'][:3], w.T[:3]) and row['n_match'] == w.inliers and row['recalltime'] == w.iters
        assert _same_bits(np.float64(row['ir']), np.float64(w.rmse))
        f = np.load(f'{d1}/{sub_icp}/{a}-{b}.npz')
        assert _same_bits(f['trans'][:3], w.T[:3]) and int(f['recalltime']) == w.iters and int(f['inliers']) == w.inliers
    assert os.path.exists(f'{d1}/{sub_icp}/pre.log') and ref['icp']['pairs'] == len(ds.pair_ids)
    assert any(w.iters >= 1 for w in want)
