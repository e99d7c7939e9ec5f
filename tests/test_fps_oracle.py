"""The farthest-point sampling oracle (tests/_fps_oracle.py) against itself, the input families of tests/_fps_cases.py against the conditions
that name them, the declarations of the v6s entries, and the FPFH oracle chain on sampled rows, on the CPU.  tests/test_hip_fps.py runs the
same families on the device."""
import os
import re

import numpy as np
import pytest

import _fpfh_cases as FK
import _fps_cases as PC
import _fps_oracle as PO
import _sc2_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b, m=None):
    m = a.rows.shape[0] if m is None else m
    return (np.array_equal(a.rows[:m], b.rows[:m]) and a.dist2[:m].tobytes() == b.dist2[:m].tobytes() and np.array_equal(a.tied[:m], b.tied[:m]))


@pytest.mark.parametrize('case', PC.CASES, ids=PC.case_id)
def test_the_two_oracle_forms_agree(case):
    """... on every case; the literal double loop of a large case runs to the k that keeps it under PC.LOOPS_MAX_WORK visits, and is then the
    prefix of the vectorised form's result"""
    pts, k, start, stop = PC.case(*case)
    a = PC.reference(*case)
    assert a.rows.dtype == np.int32 and a.dist2.dtype == np.float64 and a.rows.shape == (k,) and a.dist2.shape == (k,)
    kk = min(k, max(1, PC.LOOPS_MAX_WORK // max(pts.shape[0], 1)))
    b = PO.fps_loops(pts, kk, start, PC.stop2_of(stop))
    assert b.count == min(a.count, kk) and _same(a, b, b.count)
    assert (b.rows[b.count:] == -1).all() and (b.dist2[b.count:] == 0).all()


@pytest.mark.parametrize('case', PC.CASES, ids=PC.case_id)
def test_every_result_is_a_sample(case):
    """rows distinct and live, -1 / 0 behind count, dist2 starts at +inf and does not increase, every dist2 is the distance to the rows before"""
    pts, k, start, stop = PC.case(*case)
    r = PC.reference(*case)
    c = r.count
    rows = r.rows[:c]
    assert (r.rows[c:] == -1).all() and (r.dist2[c:] == 0).all() and len(set(rows.tolist())) == c
    p = PO.widen(pts)
    live = np.isfinite(p).all(1)
    assert live[rows].all() and c <= min(k, int(live.sum()))
    if c:
        assert r.dist2[0] == np.inf and (np.diff(r.dist2[:c]) <= 0).all()
        assert rows[0] == (start if live[start] else np.nonzero(live)[0][0])
    for s in sorted({1, c // 2, c - 1} & set(range(1, c))):
        assert r.dist2[s] == PO._d2(p[rows[:s]], p[rows[s]]).min()
    if stop is None and c < k:
        assert c == int(live.sum())                              # it ended because nothing was left


@pytest.mark.parametrize('case', PC.BOX_CASES + PC.EDGE_CASES[:1] + PC.LATTICE_CASES[:1] + PC.DEAD_CASES[:1], ids=PC.case_id)
def test_prefix_property(case):
    pts, k, start, stop = PC.case(*case)
    full = PC.reference(*case)
    for kk in sorted({1, 2, k // 2, k - 1} & set(range(1, k))):
        part = PO.fps(pts, kk, start, PC.stop2_of(stop))
        m = min(kk, full.count)
        assert part.count == m and _same(full, part, m)


def test_box_family():
    for n in PC.BOX_N:
        assert PC.reference('box', (n, n)).count == n == len(set(PC.reference('box', (n, n)).rows.tolist()))     # a full permutation
        assert PC.reference('box', (n, 1)).rows.tolist() == [0]


def test_edge_family_straddles_the_tier_edges():
    from roreg_amd import hip
    assert hip.FPS_TIER_EDGES == (13312, 32768) and hip.FPS_TIERS == ('lds', 'reg', 'mem')
    ns = [c[1] for c in PC.EDGE_CASES]
    assert [hip.fps_tier(n) for n in ns] == [0, 0, 1, 1, 1, 2]
    assert all(PC.reference(*c).count == PC.EDGE_K for c in PC.EDGE_CASES)


def test_lattice_family_is_decided_by_the_lowest_row():
    asc, perm, far = (PC.reference(*c) for c in PC.LATTICE_CASES)
    for r in (asc, perm, far):
        assert r.count == PC.LAT_N and (r.tied[1:] >= 2).sum() > PC.LAT_N // 2          # most steps hold tied candidates
        assert r.dist2[-1] == 1.0
    assert np.array_equal(asc.rows, far.rows) and asc.dist2.tobytes() == far.dist2.tobytes()     # the shift changes no d2: all are exact
    order = np.random.default_rng(0x1a7).permutation(PC.LAT_N)                            # perm's row i is asc's row order[i]
    assert not np.array_equal(order[perm.rows], asc.rows)                                 # the lowest ROW wins, not a point
    pts = PO.widen(PC.lattice_case('ascending', PC.LAT_SHIFT))
    assert (pts == np.round(pts)).all() and pts.max() == PC.LAT_SHIFT + PC.LAT_SIDE - 1


def test_copies_family_is_excluded_by_flag_not_by_distance():
    tiled = PC.reference('copies', 'tiled')
    base, times = PC.COPIES_BASE, PC.COPIES_TIMES
    assert tiled.count == base * times and (tiled.dist2[base:] == 0).all() and (tiled.dist2[:base] > 0).all()
    assert sorted(tiled.rows[:base] % base) == list(range(base))                          # first one copy of every point ...
    left = np.setdiff1d(np.arange(base * times), tiled.rows[:base])
    assert np.array_equal(tiled.rows[base:], left)                                        # ... then the rest in ascending order, each at D = 0
    one = PC.reference('copies', 'one')
    assert one.rows.tolist() == [5] + [i for i in range(PC.COPIES_ONE) if i != 5] and (one.dist2[1:] == 0).all()


def test_start_family():
    got = [PC.reference(*c) for c in PC.START_CASES]
    assert [int(r.rows[0]) for r in got] == [0, 1, PC.START_N - 1] and all(r.count == PC.START_K for r in got)
    assert not np.array_equal(got[0].rows, got[1].rows)


def test_stop_family():
    at, above, far = (PC.reference(*c) for c in PC.STOP_CASES)
    free = PC.reference('lattice', ('ascending', 0.0))
    assert PC.stop2_of(1.0) == 1.0 < PC.stop2_of(PC.STOP_ABOVE)
    assert at.count == PC.LAT_N and _same(at, free)                                       # D == stop2 is still selected
    first_one = int(np.nonzero(free.dist2 == 1.0)[0][0])
    assert 1 < first_one < PC.LAT_N and above.count == first_one and _same(above, free, first_one)
    assert (above.rows[first_one:] == -1).all() and (above.dist2[first_one:] == 0).all()
    assert far.count == 1 and far.rows[0] == 0


def test_dead_family():
    pts = PC.dead_case('some')
    assert sorted(np.nonzero(~np.isfinite(pts).all(1))[0].tolist()) == list(PC.DEAD_ROWS)
    whole, dead_start, live_start, none = (PC.reference(*c) for c in PC.DEAD_CASES)
    assert whole.count == PC.DEAD_N - len(PC.DEAD_ROWS) and whole.rows[0] == 2 and not set(whole.rows.tolist()) & set(PC.DEAD_ROWS)
    assert dead_start.rows[0] == 2 and live_start.rows[0] == 7 and dead_start.count == live_start.count == 64
    assert none.count == 0 and (none.rows == -1).all() and (none.dist2 == 0).all()
    clean = PO.fps(pts[np.isfinite(pts).all(1)], PC.DEAD_N, 0)                            # the dead rows are never used: the live rows alone
    live = np.nonzero(np.isfinite(pts).all(1))[0]
    assert np.array_equal(live[clean.rows[:clean.count]], whole.rows[:whole.count]) and clean.dist2[:clean.count].tobytes() == whole.dist2[:whole.count].tobytes()


def test_edges_of_the_input():
    e, k0, over = PC.reference('empty'), PC.reference('k0'), PC.reference('over')
    assert e.count == 0 and e.rows.tolist() == [-1] * 5 and e.dist2.tolist() == [0.0] * 5
    assert k0.count == 0 and k0.rows.shape == (0,) and k0.dist2.shape == (0,)
    assert over.count == 65 and over.rows[0] == 3 and (over.rows[65:] == -1).all() and over.rows.shape == (100,)


def test_raw_family():
    r = PC.reference('raw')
    pts = PC.case('raw')[0]
    assert pts.shape == (40000, 3) and r.count == PC.RAW_K
    d = np.sqrt(r.dist2[-1])
    assert 0.03 < d < 0.2, d                                     # 2000 samples of a 2.8 m x 3 m surface: a spacing of about 6.5 cm


def test_header_declares_the_v6s_entries():
    """include/roreg_hip.h declares the entries (marked v6s, additions under version 6), roreg_amd/_abi.py has their prototypes and the task's
    layout, the binding's constants are the header's"""
    from ctypes import c_int, c_size_t
    from roreg_amd import _abi, hip
    raw = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    assert re.search(r'#define\s+ROREG_ABI_VERSION\s+6\b', raw) and _abi.ABI_VERSION == 6
    assert 'v6s' in raw
    code = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in ('roreg_fps_workspace', 'roreg_fps_batch', 'roreg_fps_steps_workspace', 'roreg_fps_steps'):
        assert re.search(r'\b' + name + r'\s*\(', code), f'{name} is not declared in roreg_hip.h'
        assert name in _abi.PROTOTYPES
    assert _abi.PROTOTYPES['roreg_fps_workspace'] == (c_size_t, [c_int])
    assert _abi.PROTOTYPES['roreg_fps_batch'] == (c_int, [_abi._P, c_int, _abi._P, c_size_t, _abi._P])
    struct = re.search(r'typedef struct \{([^}]*)\}\s*roreg_fps_task;', code).group(1)
    fields = [name for decl in struct.split(';') if decl.strip() for name in re.findall(r'(\w+)\s*(?:,|$)', decl.strip())]
    assert fields == list(_abi._FPS_TASK.names), fields
    assert _abi._FPS_TASK.itemsize == 64 and [_abi._FPS_TASK.fields[f][1] for f in _abi._FPS_TASK.names] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]
    define = {k: int(v) for k, v in re.findall(r'#define\s+ROREG_FPS_(\w+)\s+(\d+)', code)}
    assert (define['LDS_MAX_N'], define['REG_MAX_N']) == hip.FPS_TIER_EDGES and define['THREADS'] == hip.FPS_THREADS
    assert [define['TIER_' + t.upper()] for t in hip.FPS_TIERS] == [0, 1, 2]
    assert define['LDS_MAX_N'] % define['THREADS'] == 0 and define['REG_MAX_N'] % define['THREADS'] == 0 and define['LDS_MAX_N'] * 12 < 163840
    L = hip.lib()
    assert L.roreg_fps_workspace(0) == 0 and L.roreg_fps_workspace(1) == 256 and L.roreg_fps_workspace(33) == 512 and L.roreg_fps_workspace(-1) == 0
    assert L.roreg_fps_workspace(1 << 30) == 8 << 30
    assert L.roreg_fps_steps_workspace(-1) == 0 and L.roreg_fps_steps_workspace(1) == 3 * 256 and L.roreg_fps_steps_workspace(1 << 30) == (8 << 30) + 16384 + 8192
    assert hip.FPS_METHODS == ('auto', 'persistent', 'steps')
    assert hip.fps_auto_steps([40000]) and hip.fps_auto_steps([130581] * 7) and not hip.fps_auto_steps([130581] * 8) and not hip.fps_auto_steps([])
    assert hip.fps_auto_steps([32769, 40000]) and not hip.fps_auto_steps([32769, 40000] * 3)


def test_arguments_are_refused_before_any_device_call():
    """(no device here: anything that reached one would raise something else)"""
    import torch
    from roreg_amd import fpfh, sample
    from roreg_amd.register import Registrar
    for kw in (dict(k=-1), dict(k=2.5), dict(k=True), dict(k='3'), dict(k=None), dict(start=-1), dict(start=1.0), dict(min_dist=-0.1),
               dict(min_dist=float('nan')), dict(min_dist=float('inf')), dict(min_dist='x')):
        args = dict(k=5, start=0, min_dist=None)
        args.update(kw)
        with pytest.raises(ValueError):
            sample.check_args(**args)
        with pytest.raises(ValueError):
            sample.device_farthest(None, **args)
        with pytest.raises(ValueError):
            sample.farthest(np.zeros((5, 3), np.float32), **args)
    sample.check_args(None, 0, 0.1)
    for bad in (-1, 2.5, dict(k=5, radius=1.0), dict(start=1), dict(k=5, min_dist=-1.0), 'many'):
        with pytest.raises(ValueError):
            fpfh.register(np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), 0.05, keypoints=bad)
        with pytest.raises(ValueError):
            fpfh.register_scene([np.zeros((5, 3), np.float32)] * 2, [(0, 1)], 0.05, keypoints=bad)
    with pytest.raises(ValueError):
        Registrar(None, None, keypoint_method='iss')
    assert Registrar(None, None).keypoint_method == 'shuffle'
    host = torch.zeros((5, 3))
    from roreg_amd import hip
    for task in ((host, 3), (host.double(), 3), (torch.zeros((5, 4)), 3), (torch.zeros(15), 3), (np.zeros((5, 3), np.float32), 3), (host,), 7):
        with pytest.raises(ValueError):
            hip.fps_batch([task])
    with pytest.raises(ValueError):
        hip.fps_batch([], tier='fast')
    with pytest.raises(ValueError):
        hip.fps_batch([], method='fast')
    assert hip.fps_batch([]) == []


def _mutual(F0, F1):
    """test_fpfh_oracle.py's: mutual nearest neighbours of two float32 descriptor tables, the first index among equal distances"""
    a, b = F0.astype(np.float64), F1.astype(np.float64)
    d = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    n01, n10 = d.argmin(1), d.argmin(0)
    i = np.arange(a.shape[0])
    keep = n10[n01] == i
    return np.stack([i[keep], n01[keep]], 1)


CHAIN_K = (3000, 2000, 1000)


@pytest.mark.parametrize('seed', FK.TERRAIN_SEEDS)
def test_oracle_chain_registers_the_terrain_from_sampled_rows(seed):
    """tests/test_fpfh_oracle.py's chain (voxel oracle at 0.05, normals at 0.1, FPFH at 0.25, mutual nearest neighbours, the spatial-
    compatibility oracle at tau = 0.1, the hypothesis with most inliers within one voxel) with the matcher restricted to the farthest-point
    sample of each downsampled view (start = 0) intersected with the valid rows: K = 3000 stays within the family's bar of 2 degrees / 5 cm;
    K = 2000 and 1000 are printed.  Seeds 0..3 at K = 3000: 0.45 degrees / 1.0 cm on 909 mutual matches, 0.91 / 1.4 on 867, 0.63 / 0.8 on 916,
    0.46 / 0.5 on 959; at 2000: 0.21 / 0.9, 1.51 / 1.4, 0.74 / 0.6, 1.36 / 1.4; at 1000: 0.84 / 1.5, 0.91 / 1.0, 0.93 / 2.0, 0.73 / 0.6."""
    Tg = FK.terrain_pair(seed)[2]
    views = [FK.terrain_view(seed, w) for w in (0, 1)]
    refs = [FK.terrain_reference(seed, w) for w in (0, 1)]
    samples = [PO.fps(v[0], CHAIN_K[0], 0) for v in views]
    errs = {}
    for K in CHAIN_K:
        rows = []
        for r, s in zip(refs, samples):
            took = np.zeros(r[4].shape[0], bool)
            took[s.rows[:min(K, s.count)]] = True                # (the prefix property: the first K rows of the 3000-sample are the K-sample)
            rows.append(np.nonzero(took & (r[4] != 0))[0])
        mm = _mutual(refs[0][3][rows[0]], refs[1][3][rows[1]])
        P = views[0][0][rows[0][mm[:, 0]]].astype(np.float64); Q = views[1][0][rows[1][mm[:, 1]]].astype(np.float64)
        hyp = SO.hypotheses(P, Q, FK.TERRAIN_TAU).Trans
        res = np.sqrt((((Q @ hyp[:, :, :3].transpose(0, 2, 1)) + hyp[:, None, :, 3] - P[None]) ** 2).sum(2))
        best = int((res <= FK.TERRAIN_INLIER).sum(1).argmax())
        T = np.eye(4); T[:3] = hyp[best]
        errs[K] = FK.pose_error(T, Tg)
        print(f'terrain seed {seed}, K = {K}: {rows[0].shape[0]} / {rows[1].shape[0]} sampled valid rows of {views[0][0].shape[0]} / {views[1][0].shape[0]}, '
              f'{mm.shape[0]} mutual matches, {errs[K][0]:.2f} degrees, {errs[K][1] * 100:.1f} cm')
    assert errs[CHAIN_K[0]][0] <= FK.TERRAIN_DEG and errs[CHAIN_K[0]][1] <= FK.TERRAIN_T
