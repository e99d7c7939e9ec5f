"""The farthest-point sampling kernel (csrc/sample.hip, "v6s"), roreg_amd/sample.py and the layers that take its rows (fpfh.match rows0= / rows1=,
fpfh.register / register_scene keypoints=, register.Registrar keypoint_method='farthest') on the device against tests/_fps_oracle.py, on the
families of tests/_fps_cases.py (tests/test_fps_oracle.py checks the families' own conditions on the CPU).  Every comparison of the sampler
is exact: rows and count are integers, dist2 is compared by its bytes."""
import functools

import numpy as np
import pytest
import torch

import _fpfh_cases as FK
import _fps_cases as PC
import _fps_oracle as PO
import _voxel_oracle as VO
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu

KEYPOINTS = 3000


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _assert_equals_oracle(got, want, what):
    rows, dist2, count = (v.cpu().numpy() for v in got)
    assert rows.dtype == np.int32 and dist2.dtype == np.float64 and count.dtype == np.int32
    assert rows.shape == want.rows.shape and dist2.shape == want.dist2.shape and count.shape == (1,)
    assert int(count[0]) == want.count, f'{what}: count {int(count[0])} against {want.count}'
    bad = np.nonzero((rows != want.rows) | (dist2.view(np.int64) != want.dist2.view(np.int64)))[0]
    assert bad.size == 0, (f'{what}: {bad.size} of {rows.shape[0]} steps differ, the first: step {bad[0]}, row {rows[bad[0]]} against {want.rows[bad[0]]}, '
                           f'dist2 {dist2[bad[0]]!r} against {want.dist2[bad[0]]!r}')


def _task(case):
    pts, k, start, stop = PC.case(*case)
    return (_cuda(pts.reshape(-1, 3)), k, start, stop)


@pytest.mark.parametrize('case', PC.CASES, ids=PC.case_id)
def test_rows_dist2_and_count_equal_the_oracle(case):
    """hip.fps alone on every case: the oracle's bytes, and the same bytes on a second run"""
    from roreg_amd import hip
    task = _task(case)
    a, b = hip.fps(*task), hip.fps(*task)
    _assert_equals_oracle(a, PC.reference(*case), PC.case_id(case))
    assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))


def test_one_batch_of_every_case_equals_the_single_calls():
    """one launch that holds every case of every family, all three tiers in it: each task's bytes are the oracle's (which the single calls
    give, above), in the order of the tasks"""
    from roreg_amd import hip
    tiers = {hip.fps_tier(PC.case(*c)[0].shape[0]) for c in PC.CASES}
    assert tiers == {0, 1, 2}
    out = hip.fps_batch([_task(c) for c in PC.CASES])
    assert len(out) == len(PC.CASES)
    for c, got in zip(PC.CASES, out):
        _assert_equals_oracle(got, PC.reference(*c), 'batch ' + PC.case_id(c))
    again = hip.fps_batch([_task(c) for c in reversed(PC.CASES)])
    for got, other in zip(out, reversed(again)):
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(got, other))


def test_both_launch_forms_give_the_oracles_bytes():
    """the per-step launch form (one cloud over many workgroups, k + 1 launches) on every case, the stops and the dead rows included; and the
    persistent form on the clouds that 'auto' hands to the per-step form when a call holds few of them"""
    from roreg_amd import hip
    out = hip.fps_batch([_task(c) for c in PC.CASES], method='steps')
    for c, got in zip(PC.CASES, out):
        _assert_equals_oracle(got, PC.reference(*c), 'steps ' + PC.case_id(c))
    large = [c for c in PC.CASES if hip.fps_tier(PC.case(*c)[0].shape[0]) == 2]
    ns = [PC.case(*c)[0].shape[0] for c in large]
    assert len(large) == 2 and hip.fps_auto_steps(ns)
    for c, got in zip(large, hip.fps_batch([_task(c) for c in large], method='persistent')):
        _assert_equals_oracle(got, PC.reference(*c), 'persistent ' + PC.case_id(c))
    many = large * 3                                             # more large clouds than 'auto' steps through: one persistent launch
    assert not hip.fps_auto_steps(ns * 3)
    for c, got in zip(many, hip.fps_batch([_task(c) for c in many])):
        _assert_equals_oracle(got, PC.reference(*c), 'auto ' + PC.case_id(c))


TIER_CASES = ([('box', (n, n)) for n in (1, 65, 1025, 4097)] + PC.EDGE_CASES + PC.LATTICE_CASES[1:2] + PC.COPIES_CASES + PC.START_CASES[1:] + PC.STOP_CASES[1:2]
              + PC.DEAD_CASES + PC.INPUT_EDGE_CASES)


@pytest.mark.parametrize('tier', ['reg', 'mem'])
def test_a_higher_tier_gives_the_same_bytes(tier):
    """the cases a lower tier serves, run where the running minima stay in registers without LDS and where they live in the workspace: sizes
    below one row per lane, below and above one chunk of rows per lane, and the edges"""
    from roreg_amd import hip
    cases = [c for c in TIER_CASES if hip.fps_tier(PC.case(*c)[0].shape[0]) <= hip.FPS_TIERS.index(tier)]
    out = hip.fps_batch([_task(c) for c in cases], tier=tier)
    for c, got in zip(cases, out):
        _assert_equals_oracle(got, PC.reference(*c), f'tier {tier} ' + PC.case_id(c))
    with pytest.raises(ValueError):
        hip.fps(_cuda(PC.box_case(hip.FPS_TIER_EDGES[0] + 1)), 4, tier='lds')


def test_farthest_of_a_host_cloud_of_its_voxels_and_until_covered():
    from roreg_amd import hip, sample, voxel
    pts = PC.case('raw')[0]
    want = PC.reference('raw')
    res = sample.farthest(pts, 500, start=0)
    assert res.rows.dtype == torch.int64 and np.array_equal(res.rows.cpu().numpy(), want.rows[:500]) and res.points.shape == (40000, 3)
    assert res.dist2.cpu().numpy().tobytes() == want.dist2[:500].tobytes()
    assert sample.coverage_radius(res) == float(np.sqrt(want.dist2[499]))
    # voxel=: the composition by hand, and the oracle on the voxel oracle's centroids
    v = sample.farthest(pts, 300, start=7, voxel=FK.TERRAIN_VOXEL)
    down = voxel.device_downsample(_cuda(pts), FK.TERRAIN_VOXEL)[0]
    rows, dist2, count = hip.fps(down, 300, 7)
    assert int(count) == 300 and torch.equal(v.rows, rows.long()) and torch.equal(v.dist2, dist2) and torch.equal(v.points, down)
    cen = np.ascontiguousarray(VO.downsample(pts, FK.TERRAIN_VOXEL).points, np.float32)
    ref = PO.fps(cen, 300, 7)
    assert np.array_equal(v.points.cpu().numpy(), cen) and np.array_equal(v.rows.cpu().numpy(), ref.rows) and v.dist2.cpu().numpy().tobytes() == ref.dist2.tobytes()
    # outliers= applies before the sampling too
    spec = dict(kind='radius', radius=0.1, min_neighbors=3)
    from roreg_amd import outliers
    kept = outliers.radius(pts[:5000], 0.1, 3).points
    f = sample.farthest(pts[:5000], 50, outliers=spec)
    assert torch.equal(f.points, kept) and np.array_equal(f.rows.cpu().numpy(), PO.fps(kept.cpu().numpy(), 50).rows)
    # k=None, min_dist=r: until covered at r -- every point within r of a sampled one, the sampled ones at least r apart
    r = 0.25
    cov = sample.farthest(cen, None, min_dist=r)
    ref = PO.fps(cen, cen.shape[0], 0, r * r)
    m = ref.count
    assert 1 < m < cen.shape[0] and np.array_equal(cov.rows.cpu().numpy(), ref.rows[:m]) and sample.coverage_radius(cov) >= r
    d2 = PO._d2(PO.widen(cen)[:, None, :], PO.widen(cen)[ref.rows[:m]][None, :, :])
    assert d2.min(1).max() < r * r
    with pytest.raises(ValueError):
        sample.coverage_radius(sample.farthest(np.zeros((0, 3), np.float32), 5))


def test_farthest_many_equals_the_single_calls():
    from roreg_amd import sample
    clouds = [PC.case(*c)[0] for c in (('box', (1025, 1025)), ('edge', PC.EDGE_CASES[3][1]), ('raw', None), ('empty', None), ('dead', ('some', 64, 1)))]
    many = sample.farthest_many(clouds, 200, start=0)
    assert [int(m.rows.shape[0]) for m in many] == [200, 200, 200, 0, 200]
    for c, m in zip(clouds, many):
        one = sample.farthest(c, 200, start=0)
        assert torch.equal(m.rows, one.rows) and torch.equal(m.dist2.view(torch.int64), one.dist2.view(torch.int64)) and torch.equal(m.points.view(torch.int32), one.points.view(torch.int32))
    dev = sample.device_farthest([_cuda(c) for c in clouds[:3]], 200)
    for (rows, dist2, count), m in zip(dev, many):
        assert int(count) == 200 and torch.equal(rows.long(), m.rows) and torch.equal(dist2, m.dist2)
    assert sample.farthest_many([], 5) == []


def test_invalid_arguments_raise_value_error():
    from roreg_amd import hip, sample
    pts = _cuda(PC.box_case(65))
    for args in ((pts, -1), (pts, 2.5), (pts, 3, 65), (pts, 3, -1), (pts, 3, 1.0), (pts, 3, 0, -0.5), (pts, 3, 0, float('nan')), (pts, 3, 0, float('inf')),
                 (pts, 3, 0, 1e200), (pts.double(), 3), (pts[:, :2].contiguous(), 3), (pts.reshape(-1), 3), (pts.cpu(), 3), (pts.t(), 3), (pts.cpu().numpy(), 3)):
        with pytest.raises(ValueError):
            hip.fps(*args)
    with pytest.raises(ValueError):
        hip.fps(pts, 3, tier='fast')
    with pytest.raises(ValueError):
        hip.fps(pts, 3, method='fast')
    with pytest.raises(ValueError):
        hip.fps_batch([(pts, 3), (pts, 3, 65)])
    for kw in (dict(k=-1), dict(k=None), dict(start=65), dict(min_dist=-1.0), dict(voxel=-0.1), dict(outliers=dict(kind='nearest'))):
        args = dict(k=5)
        args.update(kw)
        with pytest.raises(ValueError):
            sample.farthest(pts.cpu().numpy(), **args)
    assert int(hip.fps(pts, 3, 64)[0][0]) == 64                  # the last row is a start


# ---- the layers ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _described(seed):
    """the two terrain views as fpfh.register describes them, and their farthest-point samples (int32 rows, -1 behind the count)"""
    from roreg_amd import fpfh, sample
    p0, p1, _ = FK.terrain_pair(seed)
    d = [fpfh.describe(p, 5.0 * FK.TERRAIN_VOXEL, voxel=FK.TERRAIN_VOXEL) for p in (p0, p1)]
    rows = [r[0] for r in sample.device_farthest([x.points for x in d], KEYPOINTS)]
    return d, rows


def _oracle_mutual(F0, F1, r0, r1):
    """mutual nearest neighbours by the matcher's oracle (oracle.ref_numpy.knn, the float32 search hip.nn_search is pinned to) on the rows r0 /
    r1 of two descriptor tables -> [M,2] rows of the tables, in increasing row of side 0"""
    nn01 = O.knn(F1[r1], F0[r0], 1)[1]
    nn10 = O.knn(F0[r0], F1[r1], 1)[1]
    i = np.arange(r0.shape[0])
    keep = nn10[nn01] == i
    return np.stack([r0[i[keep]], r1[nn01[keep]]], 1)


def test_match_on_given_rows_equals_the_oracle_and_both_methods_agree():
    from roreg_amd import fpfh
    (d0, d1), (s0, s1) = _described(0)
    valid = [x.valid.cpu().numpy() != 0 for x in (d0, d1)]
    shuffled = [s.long()[torch.randperm(s.shape[0], generator=torch.Generator().manual_seed(q)).cuda()] for q, s in enumerate((s0, s1))]     # any order
    got = {m: fpfh.match(d0, d1, method=m, rows0=shuffled[0], rows1=shuffled[1]) for m in ('scan', 'mfma', 'auto')}
    assert torch.equal(got['scan'], got['mfma']) and torch.equal(got['auto'], got['mfma']) and got['mfma'].dtype == torch.int64
    rows = []
    for s, v in zip((s0, s1), valid):
        took = np.zeros(v.shape[0], bool)
        took[s.cpu().numpy()[:KEYPOINTS]] = True
        rows.append(np.nonzero(took & v)[0])
    assert all(KEYPOINTS - 10 < r.shape[0] <= KEYPOINTS for r in rows)
    want = _oracle_mutual(d0.features.cpu().numpy(), d1.features.cpu().numpy(), rows[0], rows[1])
    m = got['mfma'].cpu().numpy()
    assert m.shape[0] > 500 and np.array_equal(m, want) and (np.diff(m[:, 0]) > 0).all()
    # a list on one side only, the -1 padding of a short sample, rows the cloud does not have, a cut
    one = fpfh.match(d0, d1, rows0=torch.cat([shuffled[0][:100], torch.tensor([-1, -1, 10 ** 9]).cuda()]))
    keep = np.zeros(valid[0].shape[0], bool); keep[shuffled[0][:100].cpu().numpy()] = True
    assert np.array_equal(one.cpu().numpy(), _oracle_mutual(d0.features.cpu().numpy(), d1.features.cpu().numpy(), np.nonzero(keep & valid[0])[0], np.nonzero(valid[1])[0]))
    cut = fpfh.match(d0, d1, 100, rows0=s0, rows1=s1)
    assert cut.shape[0] == 100 and set(map(tuple, cut.cpu().numpy().tolist())) <= set(map(tuple, m.tolist()))
    assert tuple(fpfh.match(d0, d1, rows0=torch.zeros(0, dtype=torch.int64).cuda()).shape) == (0, 2)
    # rows=None: what it returns today, the composition of the literal searches over the valid rows
    from roreg_amd import hip
    v0, v1 = (torch.from_numpy(np.nonzero(v)[0]).cuda() for v in valid)
    nn01 = hip.nn_search(d0.features, d1.features, src_rows=v0, tgt_rows=v1)
    nn10 = hip.nn_search(d1.features, d0.features, src_rows=v1, tgt_rows=v0)
    out, cnt = hip.mutual_matches(nn01, nn10, sample0=v0, sample1=v1)
    assert torch.equal(fpfh.match(d0, d1), out[:int(cnt)]) and torch.equal(fpfh.match(d0, d1, rows0=None, rows1=None), out[:int(cnt)])
    pairs = fpfh.match_pairs([d0, d1], [(0, 1), (1, 0)], rows=[s0, s1])
    assert torch.equal(pairs[0], got['mfma']) and torch.equal(pairs[1], fpfh.match(d1, d0, rows0=s1, rows1=s0))
    assert torch.equal(fpfh.match_pairs([d0, d1], [(0, 1)])[0], out[:int(cnt)])


@pytest.mark.parametrize('seed', FK.TERRAIN_SEEDS)
def test_register_from_keypoints_lands_on_the_terrain_pose(seed):
    """fpfh.register(keypoints=3000) within the family's bar of 2 degrees / 5 cm (tests/test_fps_oracle.py: the oracle chain on the same
    sampled rows stays inside it), every matched row a sampled row, and the result bit for bit the composition describe, device_farthest,
    match, sc2.register"""
    from roreg_amd import fpfh, hip, sc2
    p0, p1, Tg = FK.terrain_pair(seed)
    res = fpfh.register(p0, p1, voxel=FK.TERRAIN_VOXEL, keypoints=KEYPOINTS)
    deg, dt = FK.pose_error(res.trans, Tg)
    print(f'terrain seed {seed}, {KEYPOINTS} keypoints: {res.matches.shape[0]} matches, {deg:.3f} degrees / {dt * 100:.2f} cm')
    assert deg <= FK.TERRAIN_DEG and dt <= FK.TERRAIN_T
    (d0, d1), (s0, s1) = _described(seed)
    for side, s in enumerate((s0, s1)):
        rows = s.cpu().numpy()
        assert (rows >= 0).all() and rows.shape == (KEYPOINTS,) and np.array_equal(rows, PO.fps(d0.points.cpu().numpy() if side == 0 else d1.points.cpu().numpy(), KEYPOINTS).rows)
        assert np.isin(res.matches[:, side], rows).all()
    m = fpfh.match(d0, d1, hip.SC2_MAX_M, rows0=s0, rows1=s1)
    by_hand = sc2.register(d0.points, d1.points, m, None, ird=2.0 * FK.TERRAIN_VOXEL)
    assert 300 < res.matches.shape[0] <= KEYPOINTS and np.array_equal(res.matches, m.cpu().numpy())
    assert np.array_equal(res.trans.view(np.int64), by_hand.T.view(np.int64))
    same = fpfh.register(p0, p1, voxel=FK.TERRAIN_VOXEL, keypoints=dict(k=KEYPOINTS, start=0))
    assert np.array_equal(same.matches, res.matches) and np.array_equal(same.trans.view(np.int64), res.trans.view(np.int64))


def test_register_scene_from_keypoints_equals_the_pairs_one_by_one():
    from roreg_amd import fpfh, synth
    p0, p1, _ = FK.terrain_pair(0)
    T2 = synth.dense_gt(-25.0, (0.0, 1.0, 1.0), (-0.2, 0.4, 0.1))
    p2 = ((p0[::2].astype(np.float64) - T2[:3, 3]) @ T2[:3, :3]).astype(np.float32)          # a third view: every other point of view 0, moved
    clouds, pairs = [p0, p1, p2], [(0, 1), (2, 1)]
    kp = dict(k=KEYPOINTS, min_dist=0.06, start=3)
    scene = fpfh.register_scene(clouds, pairs, voxel=FK.TERRAIN_VOXEL, keypoints=kp)
    scan = fpfh.register_scene(clouds, pairs, voxel=FK.TERRAIN_VOXEL, keypoints=kp, match_method='scan')
    for (i, j), got, other in zip(pairs, scene, scan):
        one = fpfh.register(clouds[i], clouds[j], voxel=FK.TERRAIN_VOXEL, keypoints=kp)
        assert np.array_equal(got.matches, one.matches) and 100 < got.matches.shape[0] < KEYPOINTS and np.array_equal(other.matches, one.matches)
        assert np.array_equal(got.trans.view(np.int64), one.trans.view(np.int64)) and np.isfinite(got.trans).all()
        assert np.array_equal(other.trans.view(np.int64), one.trans.view(np.int64))
    plain = fpfh.register_scene(clouds, pairs[:1], voxel=FK.TERRAIN_VOXEL)[0]                 # keypoints=None: every valid row, as before
    assert plain.matches.shape[0] > scene[0].matches.shape[0]


def test_registrar_keypoints():
    """'farthest': the oracle's rows of each cloud (float32 coordinates, start 0), as float64; a given array bypasses it; 'shuffle' (the
    default): the seeded draw it was"""
    from roreg_amd.register import Registrar, draw_keypoint_rows
    clouds = [PC.box_case(1025).astype(np.float64) * 3.0, PC.case('raw')[0][:9000], PC.box_case(63)]
    reg = Registrar(None, None, n_keypoints=500, keypoint_method='farthest')
    given = np.arange(12.0).reshape(4, 3)
    got = reg.keypoints_of(clouds, [None, None, None])
    for c, k in zip(clouds, got):
        want = PO.fps(np.asarray(c, np.float32), 500)
        assert k.dtype == np.float64 and np.array_equal(k, np.asarray(c)[want.rows[:want.count]].astype(np.float64))
    assert [k.shape[0] for k in got] == [500, 500, 63]
    mixed = reg.keypoints_of(clouds, [None, given, None], seed=5)
    assert np.array_equal(mixed[1], given) and np.array_equal(mixed[0], got[0]) and np.array_equal(mixed[2], got[2])
    old = Registrar(None, None, n_keypoints=500).keypoints_of(clouds, seed=11)
    rng = np.random.RandomState(11)
    for c, k in zip(clouds, old):
        assert np.array_equal(k, np.asarray(np.asarray(c)[draw_keypoint_rows(c.shape[0], 500, rng)], np.float64))
