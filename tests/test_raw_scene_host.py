"""Host side of the raw-scene path: the assembly's definition, the default keypoint draw, and run_plan's bookkeeping for a source that
computes its features (no GPU: a host stand-in engine, ranks run in turn through tests/_raw_scene_cases.Mailbox)."""
import numpy as np
import pytest
import torch

import _raw_scene_cases as K
from roreg_amd import distributed as D


@pytest.mark.parametrize('N,R,F,g0', [(1, 1, 32, 59), (5, 3, 16, 0), (7, 12, 32, 48), (3, 60, 4, 0), (4, 7, 8, 53)])
def test_assembly_definition_against_the_triple_loop(N, R, F, g0):
    feats, cuts, nn = K.kernel_case(1, N, R, F)
    a = K.assemble_numpy(feats, cuts, nn, g0, np.full((N, F, 60), K.SENTINEL, np.float32))
    b = K.assemble_loops(feats, cuts, nn, g0, np.full((N, F, 60), K.SENTINEL, np.float32))
    assert a.tobytes() == b.tobytes()
    outside = np.ones(60, bool); outside[g0:g0 + R] = False
    assert (a[:, :, outside] == K.SENTINEL).all() and (a[:, :, ~outside].view(np.uint32) != np.float32(K.SENTINEL).view(np.uint32)).any()
    assert np.array_equal(nn[:, 0], np.zeros(R)) and np.array_equal(nn[:, -1], np.diff(cuts) - 1) and (np.diff(cuts)[::3] == 1).all()


def _dataset(tmp_path, clouds):
    from roreg_amd.dataops.dataset import ThrDMatchPartDataset
    root = tmp_path / 'scene'
    (root / 'PointCloud').mkdir(parents=True)
    (root / 'PointCloud' / 'gt.log').write_text('')
    for k, pc in enumerate(clouds):
        np.savetxt(root / 'PointCloud' / f'cloud_bin_{k}.txt', pc, delimiter=',', fmt='%.17g')
    return ThrDMatchPartDataset(str(root), len(clouds))


def test_default_keypoints_are_get_kps_fallback_under_the_same_stream(tmp_path):
    """Registrar's default keypoints, drawn from RandomState(seed) cloud after cloud, are what dataset.get_kps's fallback draws from the global
    generator seeded alike: more rows than n_keypoints (5000, the fallback's constant), fewer rows, and a given array that bypasses the draw."""
    from roreg_amd.register import Registrar, draw_keypoint_rows
    rng = np.random.default_rng(2)
    clouds = [rng.uniform(-1, 1, (5200, 3)), rng.uniform(-1, 1, (300, 3)), rng.uniform(-1, 1, (40, 3))]
    ds = _dataset(tmp_path, clouds)
    np.random.seed(77)
    want = [ds.get_kps('0'), ds.get_kps('1')]                    # the fallback: no Keypoints/*.txt exist; two draws from one stream
    assert want[0].shape == (5000, 3) and want[1].shape == (300, 3)
    np.random.seed(123)
    state = np.random.get_state()
    reg = Registrar(None, None, n_keypoints=5000)
    given = clouds[2][::-1][:7]
    got = reg.keypoints_of(clouds, [None, None, given], seed=77)
    assert all(g.dtype == np.float64 for g in got)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[2].tobytes() == np.ascontiguousarray(given).tobytes()
    assert not np.array_equal(got[1], clouds[1])                                     # fewer rows than n_keypoints: every row, shuffled
    assert np.array_equal(np.sort(got[1], 0), np.sort(clouds[1], 0))
    now = np.random.get_state()
    assert now[0] == state[0] and np.array_equal(now[1], state[1]) and now[2:] == state[2:]       # the global generator was left alone
    # a given array consumes no draw: the cloud after it gets the draw it would get as the second cloud
    again = reg.keypoints_of([clouds[0], clouds[2], clouds[1]], [None, given, None], seed=77)
    assert again[2].tobytes() == want[1].tobytes()
    # without a seed: the global generator, as the reference
    np.random.seed(77)
    assert reg.keypoints_of(clouds[:2])[1].tobytes() == want[1].tobytes()
    assert np.array_equal(draw_keypoint_rows(9, 4, np.random.RandomState(5)), np.random.RandomState(5).permutation(9)[:4])


# ---- run_plan with a source that computes ---------------------------------------------------------------------------------------------------
class _Cloud:
    def __init__(self, before, eqv, keys):
        self.before, self.eqv, self.keys = before, eqv, keys


class HostEngine:
    """RegistrationEngine's interface as run_plan uses it, on the host: eqv = 2 before; a pair's result is a function of its seed and of its two
    clouds' before and eqv, whoever computed them.  Clouds in `ready` are not extracted again."""
    feat_dtype = torch.float32

    def extract_many(self, feats, keys):
        out = []
        for q in range(len(keys)):
            b = torch.as_tensor(np.asarray(feats[q]), dtype=torch.float32)
            out.append(_Cloud(b, b * 2.0, keys[q]))
        return out

    def alloc_eqv(self, before):
        return torch.full((int(before.shape[0]), 32, 60), float('nan'))

    def cloud_from_eqv(self, before, eqv, keys):
        return _Cloud(torch.as_tensor(np.asarray(before), dtype=torch.float32), eqv, keys)

    def run_scene(self, feats, keys, pair_ids, pair_seeds=None, ready=None, **kw):
        from roreg_amd.engine import PairResult
        have = {} if ready is None else ready
        todo = [i for i in sorted({int(i) for p in pair_ids for i in p}) if i not in have]
        have.update(zip(todo, self.extract_many([feats[i] for i in todo], [keys[i] for i in todo])))
        out = []
        for q, (a, b) in enumerate(pair_ids):
            c0, c1 = have[int(a)], have[int(b)]
            T = np.eye(4)
            T[:3] = np.random.RandomState(pair_seeds[q]).rand(3, 4) + float(c0.before.double().sum()) + 3.0 * float(c1.eqv.double().sum())
            out.append(PairResult(a, b, int(c0.before.shape[0]), T, q))
        return out


class CountingSource:
    """testset.GroupFeatureSource's interface with a host 'backbone': the feature of cloud i is a function of i."""
    computed = True

    def __init__(self, rows):
        self.rows_of, self.runs = rows, {}

    @staticmethod
    def feature(i, n):
        return np.random.default_rng(100 + i).standard_normal((n, 32, 60)).astype(np.float32)

    def like(self, i):
        return torch.empty((self.rows_of[int(i)], 32, 60), device='meta')

    def __getitem__(self, i):
        i = int(i)
        self.runs[i] = self.runs.get(i, 0) + 1
        return torch.from_numpy(self.feature(i, self.rows_of[i]))


def _scene(n_clouds):
    rows = {i: 3 + i for i in range(n_clouds)}
    pairs = [(str(a), str(b)) for a in range(n_clouds) for b in range(a + 1, n_clouds)]
    return rows, pairs, [500 + q for q in range(len(pairs))]


def _run_world(plan, pairs, seeds, rows, computing):
    """Every rank of `plan` in turn -> ({pair: trans}, sources per rank, stats per rank, transfers)."""
    owner, transfers = D.exchange_plan(plan, {'s': pairs})
    order = K.rank_order(plan, 's')
    assert all(order.index(src) < order.index(dst) for _, _, src, dst in transfers)
    box, table, sources, stats = {}, {}, {}, {}
    for rank in order:
        src = CountingSource(rows) if computing else {i: CountingSource.feature(i, rows[i]) for i in rows}
        sources[rank], stats[rank] = src, {}
        inputs = (src, {i: np.zeros((rows[i], 3)) for i in rows}, pairs, seeds)
        for s, a, b, res in D.run_plan(HostEngine(), plan[rank], lambda s: inputs, transfers, rank, exchange=K.Mailbox(rank, box), stats=stats[rank]):
            for r in res:
                assert (r.id0, r.id1) not in table
                table[(r.id0, r.id1)] = r.trans
    return table, sources, stats, (owner, transfers)


@pytest.mark.parametrize('world', [2, 3])            # (3: contiguous thirds -- the ranks run in turn here, so every transfer must go forward)
def test_cut_scene_with_a_computing_source_runs_every_cloud_once(world):
    """A scene cut across ranks: with a source that computes, every (scene, cloud) is computed by exactly one rank -- its owner under
    exchange_plan -- the transfer list is the file-backed plan's, the receivers get `before` beside `eqv`, and the results are those of the
    file-backed pass and of one rank alone."""
    rows, pairs, seeds = _scene(6)
    plan = D.shard_scenes({'s': len(pairs)}, 2, {'s': 6}, pair_lists={'s': pairs}, exchange=True) if world == 2 else [[('s', 5 * r, 5 * r + 5)] for r in range(3)]
    assert sum(1 for r in plan if r) == world
    got, sources, stats, (owner, transfers) = _run_world(plan, pairs, seeds, rows, computing=True)
    ref, _, ref_stats, (_, ref_transfers) = _run_world(plan, pairs, seeds, rows, computing=False)
    alone, one_source, _, _ = _run_world([[('s', 0, len(pairs))]], pairs, seeds, rows, computing=True)
    assert transfers == ref_transfers and len(transfers) > 0
    assert sorted(owner) == [('s', i) for i in range(6)]
    for i in range(6):
        ran = [r for r in sources if sources[r].runs.get(i, 0)]
        assert ran == [owner[('s', i)]] and sources[ran[0]].runs[i] == 1, (i, ran)
    assert all(v == 1 for v in one_source[0].runs.values()) and sorted(one_source[0].runs) == list(range(6))
    assert sorted(got) == sorted(ref) == sorted(alone) == sorted(pairs)
    for p in pairs:
        assert got[p].tobytes() == ref[p].tobytes() == alone[p].tobytes(), p
    for rank in stats:
        sent = sum(rows[i] * 32 * 60 * 4 for _, i, src, _ in transfers if src == rank)
        recv = sum(rows[i] * 32 * 60 * 4 for _, i, _, dst in transfers if dst == rank)
        assert stats[rank]['eqv_bytes_sent'] == ref_stats[rank]['eqv_bytes_sent'] == sent
        assert stats[rank]['eqv_bytes_received'] == ref_stats[rank]['eqv_bytes_received'] == recv
        assert stats[rank].get('before_bytes_sent', 0) == sent and stats[rank].get('before_bytes_received', 0) == recv
        assert set(ref_stats[rank]) == {'eqv_bytes_sent', 'eqv_bytes_received'}                 # a file-backed pass reports what it always did


def test_cloud_cost_shapes_the_plan_and_nothing_else():
    rows, pairs, seeds = _scene(6)
    tables, plans = [], []
    for cost in (9.0, 100.0):
        plan = D.shard_scenes({'s': len(pairs)}, 2, {'s': 6}, cloud_cost=cost, pair_lists={'s': pairs}, exchange=True)
        plans.append(plan)
        tables.append(_run_world(plan, pairs, seeds, rows, computing=True)[0])
    assert plans[0] != plans[1]
    assert all(tables[0][p].tobytes() == tables[1][p].tobytes() for p in pairs)
