"""The float32-score RANSAC kernels (csrc/ransac.hip: np_pairwise_sum_wave, np_sum_f32_of_inliers, both scoring variants, their batched
twins and the F32W refinement) against numpy's own float32 sum at every shape of the reduction: no inlier, the sequential form, one leaf with
and without a tail, the 128 | 129 leaf boundary, the split recursion, the buffer of the small variant exactly full, the same counts
through the large variant, and more than one 8192-element chunk with and without a ballot group carried across the boundary.  The inputs
are tests/_ransac_sum_cases.py's (inlier sets that no rounding can change; tests/test_ransac_sum_cases.py shows on the CPU that they
tell a sequential or a float64 accumulation from np.sum); numpy is the reference.  GPU only (-m gpu).

The 1-, 2-, 3- and 7-inlier refinements go through roreg_amd.test.estimator.refiner().Refine_trans with the float32 score array (it
passes float32 scores on as w_f32 and closes the 3x3 problem with the reference's LAPACK call), as test_refine_rank1_edge_via_host_lapack
does with ones."""
import numpy as np
import pytest
import torch

import _ransac_sum_cases as C
from oracle import ref_numpy as O

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev(name, seed):
    """-> device tensors k0, k1, w (the float32 scores widened to float64, as the kernels take them), Trans"""
    k0, k1, sc, Tr, _ = C.case(name, seed)
    return cu(k0), cu(k1), cu(sc.astype(np.float64)), cu(Tr)


def assert_overlap_bits(ov_dev, want_f32, what):
    """the device's float64 overlaps are numpy's float32 values, widened"""
    ovh = ov_dev if isinstance(ov_dev, np.ndarray) else ov_dev.cpu().numpy()
    assert ovh.dtype == np.float64 and want_f32.dtype == np.float32
    assert np.array_equal(ovh.astype(np.float32).view(np.uint32), want_f32.view(np.uint32)), (what, ovh.astype(np.float32), want_f32)
    assert np.array_equal(ovh.astype(np.float32).astype(np.float64), ovh), what


@pytest.mark.parametrize('name', list(C.CASES))
def test_score_is_numpy_float32_sum(name):
    """Per-pair scoring: masks bitwise the planted groups, overlap bitwise np.sum(float32 scores[inliers]) / M per hypothesis, best the
    first index of the strict maximum."""
    from roreg_amd import hip
    M, counts = C.CASES[name]
    for seed in C.SEEDS[name]:
        k0, k1, w, Tr = dev(name, seed)
        group = C.case(name, seed)[4]
        want, best_want = C.oracle(name, seed)
        ov, best, mask = hip.ransac_score(k0, k1, w, Tr, C.IRD, want_mask=True, w_f32=True)
        assert np.array_equal(mask.cpu().numpy().astype(bool), group[None, :] == np.arange(len(counts))[:, None]), (name, seed)
        assert_overlap_bits(ov, want, (name, seed))
        assert int(best.item()) == best_want, (name, seed)


def test_first_best_under_exact_ties_and_no_inlier_at_all():
    """600 hypotheses drawn from the 26 rows of case S: equal overlaps everywhere; the winner's row sits at p, p + 64, p + 256 and p + 300 only
    (the same thread's stride, other threads, both halves of first_best's tree) and p wins.  A launch whose every hypothesis has no inlier
    gives best = -1, and the refinement from it NaN in all of R and t."""
    from roreg_amd import hip
    seed = C.SEEDS['S'][0]
    k0, k1, w, Tr = dev('S', seed)
    want, win = C.oracle('S', seed)
    assert (np.delete(want, win) < want[win]).all()
    rng = np.random.default_rng(1)
    p = 100
    rows = rng.choice(np.delete(np.arange(len(want)), win), 600)
    rows[[p, p + 64, p + 256, p + 300]] = win
    ov, best, _ = hip.ransac_score(k0, k1, w, Tr, C.IRD, hyp_rows=cu(rows.astype(np.int64)), w_f32=True)
    assert_overlap_bits(ov, want[rows], 'row list')
    assert int(best.item()) == p == C.first_best(want[rows])
    # the greatest of the others, repeated, below a later single winner: '>' keeps the first of equal values only among the greatest
    second = int(np.argsort(want)[-2])
    rows2 = np.full(700, second); rows2[[3, 130, 515]] = [0, 0, 0]; rows2[690] = win
    _, best, _ = hip.ransac_score(k0, k1, w, Tr, C.IRD, hyp_rows=cu(rows2.astype(np.int64)), w_f32=True)
    assert int(best.item()) == 690
    rows2[690] = second
    _, best, _ = hip.ransac_score(k0, k1, w, Tr, C.IRD, hyp_rows=cu(rows2.astype(np.int64)), w_f32=True)
    assert int(best.item()) == 0 == C.first_best(want[rows2])
    # no inlier anywhere
    for M in (4096, 4097):
        k0n, k1n, scn, Trn, group = C.build(M, (0, 0, 0), 0)
        assert (group < 0).all() and C.first_best(np.zeros(3, np.float32)) == -1
        a, b, wn = cu(k0n), cu(k1n), cu(scn.astype(np.float64))
        ov, best, mask = hip.ransac_score(a, b, wn, cu(Trn), C.IRD, want_mask=True, w_f32=True)
        assert np.array_equal(ov.cpu().numpy(), np.zeros(3)) and not mask.any().item() and int(best.item()) == -1
        T, st = hip.refine(a, b, wn, 2 * C.IRD, Trans=cu(Trn), best=best, want_stats=True, w_f32=True)
        assert np.isnan(T.cpu().numpy()[:3]).all(), T
        assert st[15].item() == 0.0


def _as_task(rng, k0, k1, sc, Tr, n_keys=None, rows=None):
    """the pair behind real match lists: its keypoints scattered over larger key arrays -> (task tuple, per-pair tensors)"""
    M = k0.shape[0]
    n_keys = n_keys or M + 100
    r0, r1 = rng.permutation(n_keys)[:M], rng.permutation(n_keys)[:M]
    K0, K1 = rng.uniform(0, 3, (n_keys, 3)), rng.uniform(0, 3, (n_keys, 3))
    K0[r0] = k0; K1[r1] = k1
    d = dict(k0=cu(k0), k1=cu(k1), w=cu(sc.astype(np.float64)), Tr=cu(Tr), rows=cu(rows) if rows is not None else None)
    return (cu(K0), cu(K1), cu(np.stack([r0, r1], 1).astype(np.int64)), d['w'], d['Tr'], d['rows']), d


@pytest.mark.parametrize('with_large', [False, True])
def test_batched_score_and_refinements(with_large):
    """hip.ransac_batch(w_f32=True) on ragged tasks: all with M <= 4096 (batched variant <4, 4096>), and the same tasks beside ones with
    M > 4096 (everything through the batched <2, 8192>).  Per task: the overlaps the batch left in its workspace are numpy's, best is the
    oracle's winner, and T1, T2 and both statistics are bitwise the per-pair float32-score refinements."""
    from roreg_amd import hip
    rng = np.random.default_rng(7)
    names = [('S', C.SEEDS['S'][1]), ('F_4096', C.SEEDS['F_4096'][0]), ('F_2049', C.SEEDS['F_2049'][0])]
    if with_large:
        names += [('L_4097', C.SEEDS['L_4097'][0]), ('C_9000_8200', C.SEEDS['C_9000_8200'][0]), ('C_16385', C.SEEDS['C_16385'][0])]
    tasks, per_pair, wants = [], [], []
    for name, seed in names:
        k0, k1, sc, Tr, _ = C.case(name, seed)
        t, d = _as_task(rng, k0, k1, sc, Tr)
        tasks.append(t); per_pair.append(d); wants.append(C.oracle(name, seed))
    # a 3-match task (two of them inliers of its second hypothesis), and case S again through a row list that repeats rows
    k0, k1, sc, Tr, group = C.build(3, (0, 2), 4)
    t, d = _as_task(rng, k0, k1, sc, Tr, n_keys=40)
    ov3 = np.array([O.overlap_cal(k0, k1, Tr[h], sc, C.IRD) for h in range(2)])
    tasks.insert(1, t); per_pair.insert(1, d); wants.insert(1, (ov3, C.first_best(ov3)))
    k0, k1, sc, Tr, _ = C.case('S', C.SEEDS['S'][2])
    rows = rng.integers(0, len(C.S_COUNTS), 37).astype(np.int64)
    t, d = _as_task(rng, k0, k1, sc, Tr, rows=rows)
    ovS = C.oracle('S', C.SEEDS['S'][2])[0][rows]
    tasks.append(t); per_pair.append(d); wants.append((ovS, C.first_best(ovS)))

    best, T1, st1, T2, st2, ctx = hip.ransac_batch(tasks, C.IRD, w_f32=True, keep=True)
    best, T1, st1, T2, st2 = [x.cpu().numpy() for x in (best, T1, st1, T2, st2)]
    # workspace of roreg_ransac_batch: gathered k0 [total_M, 3], k1 [total_M, 3], overlaps [n_tasks, max_H]
    ws, total_M = ctx[1].cpu().numpy(), ctx[2]
    max_H = max(len(w[0]) for w in wants)
    ov_all = ws[6 * total_M:6 * total_M + len(tasks) * max_H].reshape(len(tasks), max_H)
    for q, (d, (ov_want, best_want)) in enumerate(zip(per_pair, wants)):
        assert_overlap_bits(ov_all[q, :len(ov_want)], ov_want, q)
        assert best[q] == best_want, q
        _, b, _ = hip.ransac_score(d['k0'], d['k1'], d['w'], d['Tr'], C.IRD, hyp_rows=d['rows'], w_f32=True)
        a1, s1 = hip.refine(d['k0'], d['k1'], d['w'], C.IRD * 2.0, Trans=d['Tr'], hyp_rows=d['rows'], best=b, want_stats=True, w_f32=True)
        a2, s2 = hip.refine(d['k0'], d['k1'], d['w'], C.IRD, T_in=a1, want_stats=True, w_f32=True)
        assert int(b.item()) == best_want
        for got, want in ((T1[q], a1), (st1[q], s1), (T2[q], a2), (st2[q], s2)):
            assert np.array_equal(got.reshape(-1), want.cpu().numpy().reshape(-1), equal_nan=True), q
        assert np.isfinite(T2[q]).all(), q


@pytest.mark.parametrize('name', list(C.REFINE_CASES))
def test_refine_normalises_by_numpy_float32_sum(name):
    """Refinement with float32 weights from the planted hypothesis: T within 1e-9 of the oracle's (the tolerance of the golden comparisons
    of refine; the float64 sums differ from numpy's in association only), stats[15] bitwise np.sum of the float32 inlier scores -- the
    sequential sum below 8 inliers, where T comes through the estimator's refiner and the host's LAPACK."""
    from roreg_amd import hip
    from roreg_amd.test.estimator import refiner
    M, counts = C.REFINE_CASES[name]
    k0, k1, sc, Tr, group = C.case(name, C.REFINE_SEED)
    a, b, w = cu(k0), cu(k1), cu(sc.astype(np.float64))
    for h, n in enumerate(counts):
        want = O.refine_trans(k0, k1, Tr[h], sc, C.IRD)
        T4 = np.eye(4); T4[:3] = Tr[h]
        T, st = hip.refine(a, b, w, C.IRD, T_in=cu(T4), want_stats=True, w_f32=True)
        s15 = st.cpu().numpy()[15]
        if n < 8:
            T = refiner().Refine_trans(k0, k1, Tr[h], sc, inlinerdist=C.IRD)
            seq = np.float32(0)
            for v in sc[group == h]:
                seq = np.float32(seq + v)
            assert seq == np.sum(sc[group == h])
        else:
            T = T.cpu().numpy()
        assert np.abs(T - want).max() < 1e-9, (n, np.abs(T - want).max())
        assert s15 == np.float64(np.sum(sc[group == h])) and np.float64(np.float32(s15)) == s15, n
