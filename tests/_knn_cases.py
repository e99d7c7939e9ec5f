"""Seeded input families of the nearest-neighbour searches' tests (roreg_amd/csrc/nn_search.hip: nn_search, knn_search, knn_search_seg, pdist,
mutual_matches).  tests/test_knn_cases.py asserts on the CPU that each family meets the condition it is named for, tests/test_hip_knn.py runs the
same families on the device against oracle/ref_numpy.py.  numpy only, no GPU imports; every array returned is read-only.

  randn      -- ordinary data at the edge sizes;
  duplicates -- exact duplicate target rows placed BY INDEX under the host code's slice geometry (restated below): both copies inside one
                slice, across a slice boundary, in the first and the last slice, and k+3 copies followed by an unrelated closer row;
  lattice    -- a permuted integer grid (all arithmetic exact): distinct targets at exactly equal distances, more of them than a list holds;
  root_ties  -- targets on a shell of radius 1(1 + a few 1e-7) about sources of norm ~1e-8: radicands an ulp or two apart whose correctly
                rounded roots coincide, so that 'L2' (first index among equal roots) and 'SquareL2' (smallest radicand) disagree;
                as 'root_shrink' with radii decreasing by index, which puts the equal roots inside one slice;
  overflow   -- rows of magnitude 1e20: every distance of such a source is +inf; targets of which only some stay finite;
  nan        -- randn with one source row and one target row holding a NaN."""
import functools

import numpy as np

f32 = np.float32
BIG = 1e20                                    # (1e20)^2 overflows float32


def _rng(*key):
    return np.random.default_rng([sum(str(k).encode()) if isinstance(k, str) else int(k) for k in key])


def _ro(*arrays):
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, f32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def _cdiv(a, b):
    return -(-a // b)


# ---- the slice geometry of the host code (csrc/nn_search.hip), restated ---------------------------------------------------------------------
def nn_geometry(m, n):
    """roreg_nn_search_ex at F = 3 / 32: -> (targets per slice, slices = grid.y).  About 2048 workgroups, never more slices than targets."""
    gx = _cdiv(m, 256)
    slices = min(_cdiv(2048, gx), n)
    per = _cdiv(n, slices)
    return per, _cdiv(n, per)


def knn_slices(m, n):
    """knn_slices(): about 512 workgroups, at least 32 targets per slice; 1 = the single-pass kernel."""
    gx = _cdiv(m, 256)
    return max(1, min(_cdiv(512, gx), _cdiv(n, 32)))


def knn_geometry(m, n):
    """roreg_knn_search_ex at F = 3 / 32, k <= 8: -> (targets per slice, grid.y); (n, 1) is the single-pass kernel."""
    s = knn_slices(m, n)
    if s == 1:
        return n, 1
    per = _cdiv(n, s)
    return per, _cdiv(n, per)


def seg_geometry(sizes, n):
    """roreg_knn_search_seg on clouds of `sizes` points: -> (targets per slice, slices holding any) of a cloud of n points.  grid.y comes from
    the LARGEST cloud; every cloud cuts its own n into that many slices, the trailing ones possibly empty."""
    gx = _cdiv(max(sizes), 256)
    slices = max(1, min(_cdiv(2048, gx * len(sizes)), _cdiv(max(sizes), 32)))
    per = _cdiv(n, slices)
    return per, _cdiv(n, per)


def slice_of(j, per):
    return j // per


# ---- randn ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def randn(F, m, n, seed=0):
    rng = _rng('randn', F, m, n, seed)
    return _ro(rng.standard_normal((m, F)), rng.standard_normal((n, F)))


# ---- duplicates -----------------------------------------------------------------------------------------------------------------------------
def duplicate_plan(per, slices, n, k):
    """Where the copies go, given the geometry: {'inside': (a, b), 'boundary': (a, b), 'ends': (a, b), 'group': (first, count, closer)} with
    a < b target indices holding the same row; `group`: `count` = k+3 consecutive copies and the index `closer` > all of them of an unrelated
    row that lies closer to the sources aimed at the group.  Kinds the geometry has no room for are left out."""
    plan, used = {}, set()

    def take(*idx):
        if len(set(idx)) == len(idx) and all(0 <= j < n for j in idx) and not used & set(idx):
            used.update(idx)
            return True
        return False
    if slices >= 2:
        s = (slices - 1) // 2                                      # a boundary in the middle
        if take(s * per + per - 1, (s + 1) * per):
            plan['boundary'] = (s * per + per - 1, (s + 1) * per)
        if take(0, n - 1):
            plan['ends'] = (0, n - 1)
    if per >= 2:
        s = slices // 3
        a = s * per + (1 if per >= 4 else 0)
        if a + 1 < min((s + 1) * per, n) and take(a, a + 1):
            plan['inside'] = (a, a + 1)
    g = k + 3
    for first in list(range(n // 3, n - g)) + list(range(0, min(n // 3, n - g))):
        later = [j for j in range(first + g, n) if j not in used]
        if later and not used & set(range(first, first + g)):
            plan['group'] = (first, g, later[len(later) // 2])
            break
    return plan


@functools.lru_cache(maxsize=None)
def duplicates(F, m, n, k, per, slices, seed=0):
    """-> (source [m,F], target [n,F], plan, aimed): randn targets with the copies of duplicate_plan(per, slices, n, k); aimed[name] are the
    source rows lying 0.02 +- 1e-3 from that plan entry's row (so the copies are their nearest targets, tied exactly) -- every len(plan)+1-th
    source takes a turn, the others stay randn."""
    rng = _rng('duplicates', F, m, n, k, per, slices, seed)
    S, T = rng.standard_normal((m, F)), rng.standard_normal((n, F)).astype(f32)
    plan = duplicate_plan(per, slices, n, k)
    names = sorted(plan)
    aimed = {name: [] for name in names}
    u = rng.standard_normal(F); u /= np.linalg.norm(u)
    for name in names:
        if name == 'group':
            first, g, closer = plan[name]
            T[first:first + g] = T[first]
            T[closer] = (T[first] + 0.02 * u).astype(f32)         # the aimed sources sit around this row, 0.02 from the copies
        else:
            a, b = plan[name]
            T[b] = T[a]
    for i in range(m):
        turn = (i + seed) % (len(names) + 1)
        if turn < len(names):
            name = names[turn]
            S[i] = T[plan[name][0]] + 0.02 * u + 1e-3 * rng.standard_normal(F)
            aimed[name].append(i)
    S, T = _ro(S, T)
    return S, T, plan, {name: np.array(v, np.int64) for name, v in aimed.items()}


# ---- lattice --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(F, m=None, side=7, seed=0):
    """-> (source [m,F], target [side^3,F]).  Targets: the integer grid {0..side-1}^3 in a seeded order.  Sources: the grid points and the
    (side-1)^3 cell centres (half-integers), in a seeded order, the first m of them (default: all).  F > 3: the grid occupies channels 0..2, the
    others hold small integers -- one pattern for all targets, and per source that pattern plus 0 or 1 per channel -- so every distance is the
    grid's plus a per-source integer and every sum stays exact in float32."""
    rng = _rng('lattice', F, side, seed)
    ax = np.arange(side)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3).astype(np.float64)
    cx = np.arange(side - 1) + 0.5
    cells = np.stack(np.meshgrid(cx, cx, cx, indexing='ij'), -1).reshape(-1, 3)
    T3 = grid[rng.permutation(len(grid))]
    S3 = np.concatenate([grid, cells])[rng.permutation(len(grid) + len(cells))]
    if m is not None:
        assert m <= len(S3), (m, len(S3))
        S3 = S3[:m]
    if F < 3:
        raise ValueError('lattice needs F >= 3')
    T, S = np.zeros((len(T3), F)), np.zeros((len(S3), F))
    T[:, :3], S[:, :3] = T3, S3
    if F > 3:
        pattern = (np.arange(F - 3) % 5) - 2.0
        T[:, 3:] = pattern
        S[:, 3:] = pattern + rng.integers(0, 2, (len(S3), F - 3))
    return _ro(S, T)


# ---- root ties ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def root_ties(F, m, n, jitter=4e-7, shrinking=False, seed=0):
    """-> (source [m,F], target [n,F]).  Targets: random directions times 1 + j, j uniform in +-jitter (radicands within a few float32 ulps
    of 1); sources: 1e-8-level noise about the origin, the shell's centre.  shrinking: the radii decrease with the index, so that the
    targets of one SLICE are each other's nearest rivals (the smallest radicand has equal roots before it in its own slice; in seeded
    order the rivals of a slice of three lie in other slices, and the merge by radicand bits hides how the slice compared them)."""
    rng = _rng('root_ties', F, m, n, seed)
    d = rng.standard_normal((n, F))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    j = rng.uniform(-jitter, jitter, (n, 1))
    T = d * (1.0 + (-np.sort(-j, axis=0) if shrinking else j))
    S = 1e-8 * rng.standard_normal((m, F))
    return _ro(S, T)


# ---- non-finite distances -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def overflow(F, m, n, finite='third', seed=0):
    """-> (source [m,F], target [n,F]).  Every 4th source row (0, 4, ..) is 1e20 * randn with channel 0 at +1e20 (1 + |randn|): all its
    distances are +inf.  Targets: 1e20 * randn with channel 0 at -1e20 (1 + |randn|), except the finite ones -- finite='third': every j with
    j % 3 == 2; finite='two': rows n // 2 and n - 1 only (fewer than a list of 5 holds, and none of them first).  (Channel 0 keeps two large
    rows at least 2e20 apart: a difference of two 1e20 * randn can stay below 1.8e19, whose square is finite.)"""
    rng = _rng('overflow', F, m, n, finite, seed)
    S, T = rng.standard_normal((m, F)), rng.standard_normal((n, F))
    S[0::4] *= BIG
    S[0::4, 0] = BIG * (1 + np.abs(S[0::4, 0] / BIG))
    T0 = -(1 + np.abs(T[:, 0]))
    keep = np.zeros(n, bool)
    if finite == 'third':
        keep[2::3] = True
    elif finite == 'two':
        keep[[n // 2, n - 1]] = True
    else:
        raise KeyError(finite)
    T[~keep] *= BIG
    T[~keep, 0] = BIG * T0[~keep]
    return _ro(S, T)


NAN_SOURCE_ROW, NAN_TARGET_ROW = 1, 2


@functools.lru_cache(maxsize=None)
def nan(F, m, n, seed=0):
    """-> (source, target): randn with a NaN in the last channel of source row 1 and in channel 0 of target row 2 (m >= 2, n >= 3)."""
    rng = _rng('nan', F, m, n, seed)
    S, T = rng.standard_normal((m, F)), rng.standard_normal((n, F))
    S[NAN_SOURCE_ROW, F - 1] = np.nan
    T[NAN_TARGET_ROW, 0] = np.nan
    return _ro(S, T)


# ---- row lists and mutual-check inputs ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_lists(m, n, seed=0):
    """-> (src_rows, tgt_rows) int64: shorter than the arrays, permuted, with repeats (a repeated target row is an exact duplicate)."""
    rng = _rng('rows', m, n, seed)
    ms, ns = max(1, m - 3), max(1, n - 2)
    r0, r1 = rng.permutation(m)[:ms], rng.permutation(n)[:ns]
    if ms > 4:
        r0[ms // 2] = r0[0]
    if ns > 4:
        r1[ns - 1] = r1[1]
    r0.setflags(write=False); r1.setflags(write=False)
    return r0.astype(np.int64), r1.astype(np.int64)


UNSET = (-1, None, 4294967295)                 # None stands for "the other side's length": one past the last valid index


@functools.lru_cache(maxsize=None)
def mutual_inputs(m, n, seed=0):
    """-> (nn01 int64 [m], nn10 int64 [n]): about half the sources mutually matched, and every 5th entry of either array one of the values
    no search sets: -1, the other side's length, 4294967295 (nn_search's unset row)."""
    rng = _rng('mutual', m, n, seed)
    nn01, nn10 = rng.integers(0, n, m), rng.integers(0, m, n)
    for i in np.where(rng.random(m) < 0.5)[0]:
        nn10[nn01[i]] = i
    for arr, other in ((nn01, n), (nn10, m)):
        for c, j in enumerate(range(seed % 5, len(arr), 5)):
            v = UNSET[c % 3]
            arr[j] = other if v is None else v
    nn01 = nn01.astype(np.int64); nn10 = nn10.astype(np.int64)
    nn01.setflags(write=False); nn10.setflags(write=False)
    return nn01, nn10


def mutual_in_range(nn01, nn10):
    """oracle.mutual_check restricted to in-range entries: keep i with 0 <= nn01[i] < n and nn10[nn01[i]] == i, increasing i."""
    n = nn10.shape[0]
    ok = (nn01 >= 0) & (nn01 < n)
    i = np.where(ok)[0]
    i = i[nn10[nn01[i]] == i]
    return np.stack([i, nn01[i]], 1).astype(np.int64)


# ---- the cases both test modules walk -------------------------------------------------------------------------------------------------------
# nn_search: (family, F, m, n).  m around the 256-row block; n = 1, 2, 300 (one target per slice), 4100 with m <= 256 (three per slice, the
# last slice short: 4100 = 1366 * 3 + 2), m = 2305 with n = 500 (gx = 10: 205 slices asked, three targets per slice, 167 slices, the last short)
NN_SIZES = ((1, 1), (1, 2), (255, 2), (256, 300), (257, 300), (256, 4100), (2305, 500))
NN_CASES = tuple(('randn', F, m, n) for F in (3, 32) for m, n in NN_SIZES) + (('randn', 7, 257, 300), ('randn', 7, 1, 2))
NN_CASES += tuple(('duplicates', F, m, n) for F in (3, 32) for m, n in ((257, 300), (256, 4100), (2305, 500))) + (('duplicates', 7, 257, 300),)
NN_CASES += tuple(('lattice', F, m, 343) for F in (3, 32) for m in (559, 255)) + (('lattice', 7, 257, 343),)
NN_CASES += tuple(('root_ties', F, m, n) for F in (3, 32) for m, n in ((257, 300), (256, 4100))) + (('root_ties', 7, 257, 300),)
# ... and with shrinking radii where a slice holds three targets: equal roots INSIDE the winner's slice
NN_CASES += tuple(('root_shrink', F, m, n) for F in (3, 32) for m, n in ((256, 4100), (2305, 500)))

# knn_search, tuned forms (F = 3, 32; k <= 8): (family, F, m, n, k).  n = k, 32 (single pass), 33 (two slices: 17 + 16), 100, 1000
KNN_KS, KNN_MS = (1, 2, 5, 8), (1, 255, 256, 257)


def _knn_randn():
    out, c = [], 0
    for k in KNN_KS:
        for n in (k, 32, 33, 100, 1000):
            out.append((KNN_MS[c % 4], n, k)); c += 1
    return tuple(out)


KNN_SIZES = _knn_randn()
KNN_CASES = tuple(('randn', F, m, n, k) for F in (3, 32) for m, n, k in KNN_SIZES)
KNN_CASES += tuple(('duplicates', F, m, n, k) for F in (3, 32) for m, n, k in ((256, 32, 5), (257, 33, 8), (255, 100, 2), (257, 1000, 5), (257, 1000, 1)))
KNN_CASES += tuple(('lattice', F, m, n, k) for F in (3, 32) for m, n, k in ((559, 343, 5), (257, 343, 8), (256, 343, 1), (35, 27, 5)))
KNN_CASES += tuple(('root_ties', F, m, n, k) for F in (3, 32) for m, n, k in ((257, 300, 5), (257, 1000, 8), (257, 33, 2), (256, 32, 5)))
# the generic kernel: any width, k <= 32
GENERIC_FS, GENERIC_KS = (1, 2, 7, 33, 64), (9, 12, 32)
KNN_GENERIC_CASES = tuple(('randn', F, KNN_MS[(a + b) % 4], (k, 33, 100)[(a + b) % 3], k) for a, F in enumerate(GENERIC_FS) for b, k in enumerate(GENERIC_KS))
KNN_GENERIC_CASES += (('randn', 3, 257, 100, 9), ('randn', 32, 255, 33, 32), ('lattice', 7, 257, 343, 12), ('duplicates', 7, 257, 100, 9),
                      ('root_ties', 7, 257, 300, 12), ('lattice', 3, 559, 343, 32))

ROOT_JITTER = {32: 5e-8, 33: 5e-8}             # few targets: a thinner shell keeps their radicands within an ulp or two of each other


def make(family, F, m, n, k=1, form='nn'):
    """-> (source, target) of one entry of the tables above; form 'nn' / 'knn': whose slice geometry the duplicates follow."""
    if family == 'randn':
        return randn(F, m, n)
    if family == 'duplicates':
        per, slices = (nn_geometry if form == 'nn' else knn_geometry)(m, n)
        return duplicates(F, m, n, k, per, slices)[:2]
    if family == 'lattice':
        side = round(n ** (1 / 3))
        assert side ** 3 == n
        return lattice(F, m, side)
    if family == 'root_ties':
        return root_ties(F, m, n, ROOT_JITTER.get(n, 4e-7))
    if family == 'root_shrink':
        return root_ties(F, m, n, 2e-6 if F == 3 else 4e-7, shrinking=True)
    raise KeyError(family)


# knn_search_seg: clouds of these sizes in this order (the smallest and the largest both first and last: grid.y follows the largest, and
# the small ones cut their few targets into that many slices, most of them empty); 343 is the lattice, 257 carries the duplicates
def seg_sizes(k):
    return (k, 1000, 31, 32, 33, 343, 255, 256, 257, 1000, k)


@functools.lru_cache(maxsize=None)
def seg_clouds(F, k):
    sizes = seg_sizes(k)
    clouds = []
    for c, n in enumerate(sizes):
        if n == 343:
            clouds.append(lattice(F, None, 7)[1])
        elif n == 257:
            clouds.append(duplicates(F, 1, n, k, *seg_geometry(sizes, n), seed=c)[1])
        else:
            clouds.append(randn(F, 1, n, seed=c)[1])
    return sizes, tuple(clouds)


PDIST_MS, PDIST_NS = (1, 3, 4, 5), (1, 63, 64, 65)          # the kernel's tiles are 4 x 64
MUTUAL_MS = (1023, 1024, 1025, 2049)                       # one workgroup of 1024 threads walks the sources
# (F, m, n) and (F, m, n, k) of the overflow family's runs: one target per slice and three; single pass, slices and the generic kernel
OVERFLOW_NN = ((3, 261, 40), (32, 261, 40), (3, 5, 4100), (32, 5, 4100), (7, 261, 40))
OVERFLOW_KNN = ((3, 261, 40, 5), (32, 261, 40, 5), (3, 9, 32, 5), (32, 9, 32, 8), (3, 257, 100, 1), (32, 257, 100, 2), (3, 261, 40, 9), (7, 261, 40, 5),
                (32, 9, 33, 32))
