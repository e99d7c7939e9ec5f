"""The dense pair evaluation's numpy restatement (tests/_dense_eval_oracle.py) and its input families (tests/_dense_eval_cases.py), on the
CPU: the information matrix's closed form and convention, the .info writer, and that every family has the property it is named for."""
import numpy as np
import pytest

import _dense_eval_cases as K
import _dense_eval_oracle as E
import _icp_cases as C
import _icp_oracle as O
from roreg_amd.utils import RR_cal


def test_closed_form_is_the_literal_sum():
    """Lambda from the moments equals sum G^T G formed point by point, within the summation bound; symmetric; Lambda[0,0] = n01."""
    refs = [K.pair_reference(d) for d in K.PAIR_DISTS] + [r for r in K.chunk_reference() if r.n01 > 0]
    assert len(refs) > 10
    for r in refs:
        lit = E.information_literal(r.x)
        assert (np.abs(r.info - lit) <= r.info_bound).all(), np.abs(r.info - lit).max()
        assert np.array_equal(r.info, r.info.T) and r.info[0, 0] == r.n01 and r.x.shape[0] == r.n01
        assert np.array_equal(r.info[:3, :3], r.n01 * np.eye(3))


def test_information_matrix_is_the_mean_squared_displacement_to_first_order():
    """50 seeded perturbations of 0.5 degrees / 5 mm: RR_cal.computeTransformationErr(E, Lambda) within 2 % of the directly computed mean
    squared displacement of the corresponding source points (the second-order term is about the angle, 0.9 %).  The same matrix built
    with factor 1 misses a pure rotation by more than 2 x: this pins the convention."""
    r = K.pair_reference(K.FIRST_ORDER_DIST)
    assert r.n01 == 1486
    worst = 0.0
    for seed in range(K.FIRST_ORDER_DRAWS):
        P = O.perturb(np.eye(4), K.FIRST_ORDER_DEG, K.FIRST_ORDER_SHIFT, seed)
        got, want = RR_cal.computeTransformationErr(P, r.info), E.mean_squared_displacement(r.x, P)
        worst = max(worst, abs(got / want - 1.0))
    print(f'worst relative difference of {K.FIRST_ORDER_DRAWS} draws: {worst:.4%}')
    assert worst <= 0.02
    M = np.zeros((3, 3))
    for (i, j), (v, _) in r.M.items():
        M[i, j] = M[j, i] = v
    half = E.information(r.n01, np.array([v for v, _ in r.sx]), M, factor=1.0)
    for seed in range(K.FIRST_ORDER_DRAWS):
        P = O.perturb(np.eye(4), K.FIRST_ORDER_DEG, 0.0, seed)
        want = E.mean_squared_displacement(r.x, P)
        assert abs(RR_cal.computeTransformationErr(P, r.info) / want - 1.0) <= 0.02
        assert RR_cal.computeTransformationErr(P, half) < 0.5 * want


def test_info_file_round_trip(tmp_path):
    infos = np.stack([K.pair_reference(d).info for d in K.PAIR_DISTS] + [np.zeros((6, 6)), np.full((6, 6), 1.0 / 3.0) * np.arange(36).reshape(6, 6)])
    pairs = [(0, 1), (0, 2), (1, 2), (3, 7), (10, 59)]
    path = tmp_path / 'gt.info'
    RR_cal.write_trajectory_info(str(path), pairs, 60, infos)
    n, back = RR_cal.read_trajectory_info(str(path))
    assert n == 60 and back.dtype == np.float64 and back.shape == infos.shape and back.tobytes() == infos.tobytes()
    lines = open(path).read().splitlines()
    assert len(lines) == 7 * len(pairs) and lines[0].split() == ['0', '1', '60'] and lines[28].split() == ['10', '59', '60']


def test_threshold_family_has_correspondences_at_exactly_max_dist_both_ways():
    d2 = C.THR_DIST * C.THR_DIST
    for (name, a, b), r in zip(K.threshold_pairs(), K.threshold_reference()):
        A, B = E.widen(a), E.widen(b)
        f = np.flatnonzero(r.assign01 >= 0); g = np.flatnonzero(r.assign10 >= 0)
        df = ((A[r.assign01[f]] - B[f]) ** 2).sum(1); dg = ((B[r.assign10[g]] - A[g]) ** 2).sum(1)
        # at exactly max_dist: in, in both directions (168 face queries one way; the other way a lattice target's nearest is a corner query
        # inside the ball, and the 12 tie targets are the ones whose nearest sits at exactly max_dist)
        assert min((df == d2).sum(), (dg == d2).sum()) >= 12 and max((df == d2).sum(), (dg == d2).sum()) >= 160, name
        assert df.max() == d2 and dg.max() == d2
    for base in C.THR_BASES:                     # one step beyond: out, as a source point (first order) and as a target point (swapped)
        _, _, kind = C.threshold_case(base)
        plain, swapped = [r for (n, _, _), r in zip(K.threshold_pairs(), K.threshold_reference()) if n.startswith(f'base{base:g}')]
        beyond = kind == C.KIND_BEYOND
        assert beyond.sum() > 100 and (plain.assign01[beyond] == -1).all() and (swapped.assign10[beyond] == -1).all()
        assert (plain.assign01[kind == C.KIND_FACE] >= 0).all() and (swapped.assign10[kind == C.KIND_FACE] >= 0).all()


def test_chunk_family_sits_at_the_slot_edges_in_both_directions():
    pairs, refs = C.chunk_pairs(), K.chunk_reference()
    src_n = sorted({p.shape[0] for _, _, p, _ in pairs}); tgt_n = sorted({q.shape[0] for _, q, _, _ in pairs})
    for edge in (64, 256, 1024):
        assert {edge - 1, edge, edge + 1} <= set(src_n) | {1023}
    assert {1, 64, 1025} <= set(tgt_n) and {1, 63, 64, 65, 1023, 1024, 1025, 2049} <= set(src_n)
    assert sum(r.n01 > 0 and r.n10 > 0 for r in refs) >= 15
    for (_, q, p, _), r in zip(pairs, refs):
        assert r.assign01.shape[0] == p.shape[0] and r.assign10.shape[0] == q.shape[0]


def test_disjoint_family_has_no_match_either_way():
    for name, a, b, T in K.disjoint_pairs():
        r = E.evaluate(a, b, T, K.DISJOINT_DIST, nn=O.nearest_full)
        assert r.n01 == 0 and r.n10 == 0 and np.isnan(r.rmse01) and np.isnan(r.rmse10) and not r.info.any() and r.overlap0 == 0.0 == r.overlap1, name
    _, slab, mid, _ = K.disjoint_pairs()[1]
    assert (mid.min(0) >= slab.min(0) - 1e-6).all() and (mid.max(0) <= slab.max(0) + 1e-6).all()      # inside the other's bounding box


def test_box_face_family_matches_only_at_exactly_max_dist_across_the_gap():
    a, b = K.box_face_pair()
    d = K.FACE_DIST
    assert float(a[:, 0].max()) + d == float(b[:, 0].min())                    # the boxes are exactly max_dist apart
    r = E.evaluate(a, b, np.eye(4), d, nn=O.nearest_full)
    A, B = E.widen(a), E.widen(b)
    f = np.flatnonzero(r.assign01 >= 0); g = np.flatnonzero(r.assign10 >= 0)
    assert r.n01 == 81 == r.n10
    assert (((A[r.assign01[f]] - B[f]) ** 2).sum(1) == d * d).all() and (((B[r.assign10[g]] - A[g]) ** 2).sum(1) == d * d).all()
    assert r.S01[0] == 81 * d * d == r.S10[0]
    closer = E.evaluate(a, b, np.eye(4), np.nextafter(d, 0.0), nn=O.nearest_full)
    assert closer.n01 == 0 and closer.n10 == 0


def test_bounding_box_filter_keeps_the_box_face_pair_and_drops_the_far_one():
    from roreg_amd.engine import RegistrationEngine
    apart = RegistrationEngine._boxes_apart
    box = lambda p: np.stack([p.min(0), p.max(0)]).astype(np.float64)
    a, b = K.box_face_pair()
    I = np.eye(3)
    assert not apart(box(a), box(b), I, np.zeros(3), K.FACE_DIST) and not apart(box(b), box(a), I, np.zeros(3), K.FACE_DIST)
    assert apart(box(a), box(b), I, np.zeros(3), K.FACE_DIST / 2) and apart(box(a), box(b), I, np.array([0, 5.0, 0]), K.FACE_DIST)
    clouds, poses = K.scene()
    for i in range(6):                           # never drops a pair that has a correspondence
        for j in range(6):
            if i != j:
                T = K.relative(poses, i, j)
                if apart(box(clouds[i]), box(clouds[j]), T[:3, :3], T[:3, 3], K.SCENE_DIST):
                    assert E.evaluate(clouds[i], clouds[j], T, K.SCENE_DIST).n01 == 0
    assert sum(apart(box(clouds[i]), box(clouds[j]), K.relative(poses, i, j)[:3, :3], K.relative(poses, i, j)[:3, 3], K.SCENE_DIST)
               for i in range(6) for j in range(6) if i != j) >= 16


def test_scene_gt_tool_selects_by_the_smaller_directed_overlap_and_refuses_to_overwrite(tmp_path, monkeypatch):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import make_scene_gt as M
    o = np.array([[1, .5, .2, 0], [.4, 1, .05, 0], [.35, .2, 1, np.nan], [0, 0, .9, 1]])
    assert M.select_pairs(o, 0.3, 0.1) == ([(0, 1)], [(0, 2)])                 # (1,2): 0.05 is below both; (2,3): NaN selects nothing
    assert M.select_pairs(np.array([[1, .3], [.3, 1]]), 0.3, 0.1) == ([], [(0, 1)])     # exactly the threshold is low overlap
    (tmp_path / 'gt.info').write_text('keep')
    monkeypatch.setattr(sys, 'argv', ['make_scene_gt.py', '--clouds', 'a.npy', '--poses', 'p.npy', '--out', str(tmp_path), '--max_dist', '0.05'])
    with pytest.raises(SystemExit) as e:
        M.main()
    assert 'gt.info' in str(e.value) and (tmp_path / 'gt.info').read_text() == 'keep'
