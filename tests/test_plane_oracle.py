"""The plane segmentation's definition on the CPU (no GPU): the two numpy forms of tests/_plane_oracle.py agree, every family of
tests/_plane_cases.py meets the condition that names it, the header, the prototypes and the binding's constants agree, bad arguments are refused
before any device call, and csrc/plane_math.h reproduces the oracle's integers and bits in a stand-alone host program under the sanitizers."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _cluster_oracle as CO
import _plane_cases as K
import _plane_oracle as PO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the two forms -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_vectorised_oracle_equals_the_loops(case):
    """labels, n_planes, counts, triples, the raw planes' bits and round 0's hypothesis counts; a case too large for the literal loops is
    compared on a prefix of its rounds, or on the literal counts of a sample of round 0's hypotheses (tests/_plane_cases.py loops_plan)"""
    pts, dist, H, planes, min_inliers, seed = K.case(*case)
    want = K.reference(*case)
    kind, what = K.loops_plan(case)
    if kind == 'rounds':
        labels, n_planes, counts, triples, raw, hyp0 = PO.segment_loops(pts, dist, H, what, min_inliers, seed)
        assert n_planes == min(want.n_planes, what)
        assert np.array_equal(np.array(labels, np.int32), np.where(want.labels < what, want.labels, -1))
        assert counts == want.counts[:what].tolist() and triples == want.triples[:what].tolist()
        assert np.array(raw, np.float64).reshape(-1, 4).tobytes() == want.raw[:what].tobytes()
        if planes:
            assert hyp0 == want.hyp_counts.tolist()
    else:
        assert PO.score_loops(pts, want.hyp_triples[what], dist) == want.hyp_counts[what].tolist()


def test_draws_of_both_forms_and_their_range():
    for seed, r, L in ((0, 0, 3), (1, 5, 729), (2 ** 64 - 1, 63, 2 ** 30), (0x1234567890abcdef, 7, 40000)):
        d = PO.draws(seed, r, 300, L)
        assert d.min() >= 0 and d.max() < L
        assert d.tolist() == [[PO.draw_int(seed, r, h, j, L) for j in range(3)] for h in range(300)]
    assert PO.mix_int(0) == 0xE220A8397B1DCDAF                    # splitmix64's first output from state 0
    assert not np.array_equal(PO.draws(1, 0, 64, 1000), PO.draws(1, 1, 64, 1000))


@pytest.mark.parametrize('name', K.SCORE_CASES)
def test_score_forms_agree(name):
    pts, triples, dist = K.score_case(name)
    assert PO.score_loops(pts, triples, dist) == K.score_reference(name).tolist()


# ---- the families --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_every_label_has_its_count_and_passes_its_triples_test(case):
    pts, dist, H, planes, min_inliers, seed = K.case(*case)
    res = K.reference(*case)
    X = PO.widen(pts)
    assert res.labels.shape == (pts.shape[0],) and res.labels.min(initial=-1) >= -1 and res.labels.max(initial=-1) == res.n_planes - 1
    assert (res.counts[res.n_planes:] == 0).all() and (res.triples[res.n_planes:] == -1).all() and (res.raw[res.n_planes:] == 0).all()
    assert (res.labels[~np.isfinite(X).all(1)] == -1).all()
    for r in range(res.n_planes):
        rows = np.flatnonzero(res.labels == r)
        assert rows.shape[0] == res.counts[r] >= min_inliers
        t = res.triples[r]
        N, q, ok = PO.planes_of(X[t[0:1]], X[t[1:2]], X[t[2:3]])
        assert ok[0] and np.array_equal(N[0], res.raw[r, :3]) and np.isin(t, rows).all()
        assert PO.support(N, X[t[0:1]], PO.threshold(dist, q), X[rows]).all()
        later = np.flatnonzero((res.labels > r) | ((res.labels < 0) & np.isfinite(X).all(1)))
        assert not PO.support(N, X[t[0:1]], PO.threshold(dist, q), X[later]).any()          # every live row that passed was taken
        assert abs(np.sqrt((res.fit[r, :3] ** 2).sum()) - 1.0) <= 1e-15 and (res.fit[r, :3] * res.raw[r, :3]).sum() >= 0.0


def test_families_meet_their_conditions():
    ref = K.reference
    # small: no plane below three rows; three rows are one plane whenever a hypothesis draws them all
    assert [ref(*c).n_planes for c in K.SMALL_CASES] == [0, 0, 0, 1, 1]
    assert ref('small', 3).counts[0] == 3 and sorted(ref('small', 3).triples[0].tolist()) == [0, 1, 2] and (ref('small', 3).hyp_counts == -1).any()
    # tile / hyp: the slab is found first, with about two thirds of the rows
    for c in K.TILE_CASES + K.HYP_CASES[1:]:
        n = K.case(*c)[0].shape[0]
        assert 0.6 * n <= ref(*c).counts[0] <= 0.75 * n, c
    assert K.TILE == 4 * K.THREADS and K.CHUNK == 128
    # caps
    assert ref('caps', 'n_hyp').hyp_counts.shape == (65536,) and ref('caps', 'max_planes').counts.shape == (64,) and ref('caps', 'max_planes').n_planes < 64
    # lattice: the winner's count is shared by a later hypothesis (the lowest h won); the shift changes nothing
    asc, per, far = (ref(*c) for c in K.LATTICE_CASES)
    for res in (asc, per):
        best = np.flatnonzero(res.hyp_counts == res.counts[0])
        assert best.shape[0] >= 2 and np.array_equal(res.hyp_triples[best[0]], res.triples[0])
    assert np.array_equal(asc.labels, far.labels) and np.array_equal(asc.counts, far.counts) and np.array_equal(asc.triples, far.triples)
    assert np.array_equal(asc.raw[:, :3], far.raw[:, :3]) and np.array_equal(asc.hyp_counts, far.hyp_counts)
    assert asc.n_planes == 9 and (asc.labels >= 0).all() and not np.array_equal(asc.triples, per.triples)
    # threshold: rows one layer away are inliers at dist = 1 exactly (equality) and not one float64 step below
    at, below = K.score_reference('axis-at'), K.score_reference('axis-below')
    assert at.tolist() == [243] and below.tolist() == [81]
    X = PO.widen(K.lattice_cloud())
    N, q, _ = PO.planes_of(*(X[[t]] for t in K.AXIS_TRIPLE))
    s = (X - X[K.AXIS_TRIPLE[0]]) @ N[0]
    assert N[0].tolist() == [1.0, 0.0, 0.0] and int((s * s == PO.threshold(1.0, q)[0]).sum()) == 162
    assert ref('threshold', 1.0).counts[0] == 243 and ref('threshold', K.THRESHOLD_BELOW).counts.max() < 243
    # collinear / copies: every hypothesis is invalid
    for c in K.DEGENERATE_CASES:
        assert ref(*c).n_planes == 0 and (ref(*c).hyp_counts == -1).all() and (ref(*c).labels == -1).all()
    # dead rows are never drawn and never counted; two live rows are no plane
    some = ref('dead', 'some')
    assert some.n_planes == 2 and not np.isin(some.hyp_triples, K.DEAD_ROWS).any() and (some.labels[list(K.DEAD_ROWS)] == -1).all()
    assert some.hyp_counts.max() <= 300 - len(K.DEAD_ROWS)
    assert ref('dead', 'few').n_planes == 0 and (ref('dead', 'few').hyp_counts == -1).all()
    # early ends
    e = ref('early', 'min_inliers')
    assert e.n_planes == 0 and 3 <= e.hyp_counts.max() < 301 and (e.labels == -1).all() and (e.triples == -1).all()
    assert ref('early', 'no_planes').n_planes == 0 and ref('early', 'no_planes').counts.shape == (0,)
    room = ref('early', 'room')
    assert 5 <= room.n_planes < 12 and (room.counts[room.n_planes:] == 0).all() and (room.rms[room.n_planes:] == 0).all()
    # seeds
    assert not np.array_equal(ref('seeds', 1).triples, ref('seeds', 2).triples) and not np.array_equal(ref('seeds', 1).hyp_triples, ref('seeds', 2).hyp_triples)
    # score edges: a repeated row, a row of -1, a row of n, a dead row -> -1; valid triples count
    assert K.score_reference('edges').tolist()[:7] == [-1] * 7 and (K.score_reference('edges')[7:] >= 3).all()
    assert K.score_reference('none').shape == (0,) and K.score_reference('empty-cloud').tolist() == [-1]


@pytest.mark.parametrize('case', K.ROOM_CASES + K.EARLY_CASES[2:], ids=K.case_id)
def test_room_planes_are_the_rooms_faces(case):
    """the first five planes within 1 degree of a coordinate axis (the worst of these cases: 0.29 degrees; 0.44 in the objects family), the
    two largest the z faces (floor and ceiling), 540 - 716 rows each; no plane's covariance is near a double eigenvalue"""
    res = K.reference(*case)
    assert res.n_planes >= 5
    axes = []
    for r in range(5):
        deg, axis = PO.axis_angle_deg(res.raw[r, :3])
        assert deg <= 1.0, (r, deg)
        axes.append(axis)
        assert 540 <= res.counts[r] <= 716
    assert sorted(axes[r] for r in np.argsort(-res.counts[:5], kind='stable')[:2]) == [2, 2]
    assert PO.gap_ratio(res.lam[:res.n_planes]).min() >= 1e-3
    fit_deg = np.degrees(np.arccos(np.clip((res.fit[:5, :3] * PO.unit(res.raw[:5])[:, :3]).sum(1), -1, 1)))
    assert fit_deg.max() <= 1.0 and res.rms[:5].max() <= K.ROOM_DIST


@pytest.mark.parametrize('seed', K.OBJ_SEEDS)
def test_objects_fall_apart_once_the_faces_are_gone(seed):
    """the whole view is one cluster of at least 95 % of its rows; off the planes the three largest clusters hold at least 90 % of the rest"""
    pts = K.case('objects', seed)[0]
    whole = CO.dbscan(pts, K.OBJ_EPS, K.OBJ_MIN_POINTS)
    assert whole.sizes.max() >= 0.95 * pts.shape[0]
    res = K.reference('objects', seed)
    assert res.n_planes == 5 and all(PO.axis_angle_deg(res.raw[r, :3])[0] <= 1.0 for r in range(5))
    rest = pts[res.labels < 0]
    parts = CO.dbscan(rest, K.OBJ_EPS, K.OBJ_MIN_POINTS)
    top = np.sort(parts.sizes)[::-1][:3]
    print(f'seed {seed}: one cluster of {whole.sizes.max()} of {pts.shape[0]} rows; off the planes {rest.shape[0]} rows, the three largest clusters {top.tolist()}')
    assert top.sum() >= 0.9 * rest.shape[0] and top.min() >= 1000


# ---- header, prototypes, arguments ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_v6t_entries():
    from ctypes import c_double, c_int, c_size_t, c_uint64
    from roreg_amd import _abi, hip
    raw = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert re.search(r'#define\s+ROREG_ABI_VERSION\s+6\b', raw) and _abi.ABI_VERSION == 6
    assert 'v6t' in raw
    code = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in ('roreg_plane_workspace', 'roreg_plane_segment', 'roreg_plane_score'):
        assert re.search(r'\b' + name + r'\s*\(', code), f'{name} is not declared in roreg_hip.h'
        assert name in _abi.PROTOTYPES
    P = _abi._P
    assert _abi.PROTOTYPES['roreg_plane_workspace'] == (c_size_t, [c_int, c_int])
    assert _abi.PROTOTYPES['roreg_plane_segment'] == (c_int, [P, c_int, c_double, c_int, c_int, c_int, c_uint64, P, P, P, P, P, P, P, P, c_size_t, P])
    assert _abi.PROTOTYPES['roreg_plane_score'] == (c_int, [P, c_int, P, c_int, c_double, P, P])
    define = {k: int(v) for k, v in re.findall(r'#define\s+ROREG_PLANE_(\w+)\s+(\d+)', code)}
    assert (define['THREADS'], define['TILE'], define['HYP_CHUNK'], define['MAX_HYP'], define['MAX_PLANES']) == \
        (hip.PLANE_THREADS, hip.PLANE_TILE, hip.PLANE_HYP_CHUNK, hip.PLANE_MAX_HYP, hip.PLANE_MAX_PLANES)
    assert define['TILE'] % define['THREADS'] == 0 and define['HYP_CHUNK'] <= define['THREADS']
    L = hip.lib()
    assert L.roreg_plane_workspace(-1, 8) == 0 and L.roreg_plane_workspace(10, 0) == 0 and L.roreg_plane_workspace(10, hip.PLANE_MAX_HYP + 1) == 0
    assert L.roreg_plane_workspace((1 << 30) + 1, 8) == 0 and 0 < L.roreg_plane_workspace(0, 1) < L.roreg_plane_workspace(4000, 1024) < L.roreg_plane_workspace(1 << 30, 65536)
    assert L.roreg_plane_workspace(4000, 1024) % 256 == 0


def test_arguments_are_refused_before_any_device_call():
    """(no device here: anything that reached one would raise something else)"""
    import torch
    from roreg_amd import hip, segment
    cloud = np.zeros((5, 3), np.float32)
    for kw in (dict(dist=0.0), dict(dist=-1.0), dict(dist=float('nan')), dict(dist=float('inf')), dict(dist='1'), dict(dist=True), dict(dist=None),
               dict(n_hyp=0), dict(n_hyp=hip.PLANE_MAX_HYP + 1), dict(n_hyp=2.0), dict(n_hyp=True), dict(max_planes=-1), dict(max_planes=hip.PLANE_MAX_PLANES + 1),
               dict(max_planes=1.5), dict(min_inliers=2), dict(min_inliers=3.0), dict(min_inliers=2 ** 31), dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5)):
        args = dict(dist=0.01, max_planes=2, min_inliers=3, n_hyp=16, seed=0)
        args.update(kw)
        with pytest.raises(ValueError):
            segment.check_args(**args)
        for fn in (segment.planes, segment.off_planes, segment.on_planes):
            with pytest.raises(ValueError):
                fn(cloud, **args)
        with pytest.raises(ValueError):
            segment.device_planes(None, **args)
        with pytest.raises(ValueError):
            hip.plane_check_args(args['dist'], args['n_hyp'], args['max_planes'], args['min_inliers'], args['seed'])
    assert segment.check_args(0.01, hip.PLANE_MAX_PLANES, 3, hip.PLANE_MAX_HYP, 2 ** 64 - 1) == (0.01, hip.PLANE_MAX_HYP, hip.PLANE_MAX_PLANES, 3, 2 ** 64 - 1)
    with pytest.raises(ValueError):
        segment.plane(cloud, 0.01, min_inliers=1)
    with pytest.raises(ValueError):
        segment.planes(cloud, 0.01, voxel=-0.1)
    with pytest.raises(ValueError):
        segment.planes(cloud, 0.01, outliers=dict(kind='nearest'))
    host = torch.zeros((5, 3))
    for pts in (host, host.double(), torch.zeros((5, 4)), torch.zeros(15), cloud, None):
        with pytest.raises(ValueError):
            hip.plane_segment(pts, 0.01)
        with pytest.raises(ValueError):
            hip.plane_score(pts, torch.zeros((1, 3), dtype=torch.int32), 0.01)
    from roreg_amd import outliers
    assert outliers.KINDS == ('statistical', 'radius', 'cluster')


# ---- csrc/plane_math.h on the host ---------------------------------------------------------------------------------------------------------------
MATH_CASES = [('small', 3), ('small', 4), ('tile', 65), ('lattice', ('permuted', 0.0)), ('lattice', ('ascending', K.LAT_SHIFT)), ('threshold', 1.0), ('collinear', None),
              ('copies', None), ('dead', 'some'), ('dead', 'few')]


def test_plane_math_header_under_the_sanitizers(tmp_path):
    """csrc/plane_math.h compiled into a stand-alone host program (tests/_plane_math_check.cpp, its own main) with AddressSanitizer and
    UndefinedBehaviorSanitizer: the draws of three rounds, the validity, the raw planes' bits and the counts over the non-dead rows equal the
    oracle's on the small cases."""
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'plane_math_check')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-ffp-contract=off',
                           '-I' + os.path.join(ROOT, 'roreg_amd', 'csrc'), os.path.join(HERE, '_plane_math_check.cpp'), '-o', exe])
    R = 3
    for c in MATH_CASES:
        pts, dist, H, _, _, seed = K.case(*c)
        H = min(H, 64)
        seed = seed + (0xfedcba9876543210 if c[0] == 'lattice' else 0)        # a seed with high bits too
        path = str(tmp_path / 'table.bin')
        with open(path, 'wb') as f:
            f.write(struct.pack('<qqqQd', pts.shape[0], H, R, seed, dist))
            f.write(np.ascontiguousarray(pts, '<f4').tobytes())
        p = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.strip().split('\n')
        X = PO.widen(pts)
        X = X[np.isfinite(X).all(1)]
        L = X.shape[0]
        assert int(lines[-1]) == L
        if L < 3:
            assert len(lines) == 1
            continue
        got = [ln.split() for ln in lines[:-1]]
        assert len(got) == R * H
        for r in range(R):
            idx = PO.draws(seed, r, H, L)
            N, q, ok = PO.planes_of(X[idx[:, 0]], X[idx[:, 1]], X[idx[:, 2]])
            valid = ok & (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
            A = X[idx[:, 0]]
            cnt = np.full(H, -1, np.int64)
            cnt[valid] = PO.counts_of(N[valid], A[valid], PO.threshold(dist, q)[valid], X)
            d = -((N[:, 0] * A[:, 0] + N[:, 1] * A[:, 1]) + N[:, 2] * A[:, 2])
            for h in range(H):
                g = got[r * H + h]
                assert [int(v) for v in g[:6]] == [r, h, idx[h, 0], idx[h, 1], idx[h, 2], int(valid[h])], (c, r, h)
                plane = np.array([N[h, 0], N[h, 1], N[h, 2], d[h]]) if valid[h] else np.zeros(4)
                assert [int(v, 16) for v in g[6:10]] == plane.view(np.uint64).tolist() and int(g[10]) == cnt[h], (c, r, h)
