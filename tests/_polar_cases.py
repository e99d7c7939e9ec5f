"""Seeded inputs of the Kabsch closes' tests (tests/test_polar_oracle.py on the host, tests/test_hip_kabsch_edges.py on the device): 3x3
matrices U diag(sigma) V^T by family, and correspondence sets for the float64 reduction of refine_body.  Everything is a pure function of
its arguments; the mpmath references are computed once per process."""
import functools
from fractions import Fraction

import numpy as np

import _polar_oracle as PO

DECADES = tuple(range(-6, 7))
N_GPU, N_CPU = 40, 150
SMALL_S3 = (1e-6, 1e-9, 1.1e-10, 0.9e-10, 1e-12)
SWITCH_S3 = (1.1e-10, 0.9e-10, 1e-12)                              # either side of hip.stats_rank_deficient_many's sigma3 <= 1e-10 sigma1
POW2 = (200, -200, 500, -500)


def _orthogonal(rng, det):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) * det < 0:
        Q[:, 2] = -Q[:, 2]
    return Q


def _usv(rng, sigma, det=None):
    """U diag(sigma) V^T; det: the sign of det(U V^T) (None: either)"""
    U = _orthogonal(rng, 1.0)
    V = _orthogonal(rng, (1.0 if rng.random() < 0.5 else -1.0) if det is None else det)
    return (U * np.asarray(sigma, np.float64)) @ V.T


def _scale(j, exact=False):
    """the j-th matrix's scale: the decades in turn; exact: a power of two in place of a negative decade (10^-k is no float64: the product
    would round and an exact rank would be lost)"""
    k = DECADES[j % len(DECADES)]
    return float(2.0 ** (3 * k)) if exact and k < 0 else 10.0 ** k


def _planar(rng, n=6):
    """n integer points of an integer plane through the origin"""
    p, q = rng.integers(-4, 5, 3), rng.integers(-4, 5, 3)
    while not np.any(np.cross(p, q)):
        q = rng.integers(-4, 5, 3)
    xy = rng.integers(-5, 6, (n, 2))
    while np.linalg.matrix_rank(xy) < 2:
        xy = rng.integers(-5, 6, (n, 2))
    return xy[:, :1] * p + xy[:, 1:] * q


@functools.lru_cache(maxsize=None)
def families(n):
    """-> {name: H [m,3,3]} with m ~ n per family, every matrix times its scale (the decades 1e-6 .. 1e6 in turn)"""
    rng = np.random.default_rng(0x9014)
    out = {}

    def fill(name, make, count=n, exact=False):
        out[name] = np.stack([make(j) * _scale(j, exact) for j in range(count)])

    fill('generic', lambda j: _usv(rng, np.sort(rng.uniform(0.05, 1.0, 3))[::-1]))
    fill('ones', lambda j: _usv(rng, (1.0, 1.0, 1.0)))
    fill('s1=s2', lambda j: _usv(rng, (1.0, 1.0, 0.3)))
    fill('s2=s3', lambda j: _usv(rng, (1.0, 0.3, 0.3)))
    per = max(n // len(SMALL_S3), len(DECADES))
    for s in SMALL_S3:
        fill(f'small-{s:g}', lambda j: _usv(rng, (1.0, 0.5, s)), per)
    fill('two-small', lambda j: _usv(rng, (1.0, 1e-5, 1e-6)))
    refl = ((1.0, 0.6, 0.2), (1.0, 0.5, 1e-6), (1.0, 1e-3, 0.9e-3))
    for q, sig in enumerate(refl):
        fill(f'reflect-{q}', lambda j: _usv(rng, sig, det=-1.0), max(n // 3, len(DECADES)))

    def signed(j):
        sig = np.sort(rng.uniform(0.05, 1.0, 3))[::-1] * rng.choice([-1.0, 1.0], 3)
        P = np.eye(3)[rng.permutation(3)] if j % 2 else np.eye(3)
        return P * sig                                             # one non-zero per row and column: every column pair is orthogonal exactly

    fill('signed', signed)

    def rank2(j):
        a, b = _planar(rng), _planar(rng)
        return (a.T @ b).astype(np.float64)                        # integers: exact, and rank 2 exactly

    fill('rank2', rank2, exact=True)

    def rank1(j):
        a, b = rng.integers(-9, 10, 3), rng.integers(-9, 10, 3)
        a[0] = a[0] or 1; b[2] = b[2] or 1
        return np.outer(a, b).astype(np.float64)

    fill('rank1', rank1, max(n // 4, 4), exact=True)
    out['zero'] = np.zeros((2, 3, 3)); out['zero'][1] *= -1.0
    nan = np.stack([_usv(rng, (1.0, 0.5, 0.2)) for _ in range(9)])
    for q in range(9):
        nan[q].reshape(-1)[q] = np.nan
    out['nan'] = nan
    return out


ACCURACY_UVT = ('generic', 'ones', 's1=s2', 's2=s3') + tuple(f'small-{s:g}' for s in SMALL_S3) + ('two-small', 'reflect-0', 'reflect-1', 'reflect-2', 'signed')
DEGENERATE = ('rank1', 'zero', 'nan')


def pow2_members(n):
    """(name, H, k): a well- and an ill-conditioned member, to be scaled by 2^k"""
    f = families(n)
    return [(name, f[name][6 % f[name].shape[0]], k) for name in ('generic', 'small-1e-09') for k in POW2]


@functools.lru_cache(maxsize=None)
def reference(n):
    """{name: [PO.polar(H) per matrix]} for the families with finite entries and rank >= 2"""
    f = families(n)
    return {name: [PO.polar(H) for H in f[name]] for name in f if name not in DEGENERATE}


def exactly_rank2(H):
    """from the input alone, in exact rationals: det == 0 and some 2x2 minor != 0"""
    F = [[Fraction(float(v)) for v in row] for row in H]
    det = (F[0][0] * (F[1][1] * F[2][2] - F[1][2] * F[2][1]) - F[0][1] * (F[1][0] * F[2][2] - F[1][2] * F[2][0])
           + F[0][2] * (F[1][0] * F[2][1] - F[1][1] * F[2][0]))
    minors = any(F[a][c] * F[b][d] - F[a][d] * F[b][c] != 0 for a in range(3) for b in range(a + 1, 3) for c in range(3) for d in range(c + 1, 3))
    return det == 0 and minors


def first_pair_orthogonal(H):
    """from the input alone: columns 0 and 1 have a float64 dot product of exactly zero as the header sums it (the first `gamma == 0` skip)"""
    g = 0.0
    for r in range(3):
        g += H[r, 0] * H[r, 1]
    return g == 0.0 and bool(np.isfinite(H).all()) and bool(np.any(H))


# ---- the reduction of refine_body -------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 5000)
PATTERNS = ('all', 'last', 'from256', 'every256', 'per-wave', 'none')
WEIGHTS = ('uniform', 'span', 'zeros')
FORMS = ('f64', 'f32', 'none')                                    # float64 weights / float32 scores (w_f32) / the batch's w = None
OFFSET = np.array([1e3, -2e3, 5e2])
DIST = 0.05


def motion(seed=3):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = _orthogonal(rng, 1.0); T[:3, 3] = [0.2, -0.4, 0.1]
    return T


def inlier_rows(M, pattern):
    rows = np.arange(M)
    return {'all': rows, 'last': rows[-1:], 'from256': rows[256:], 'every256': rows[::256], 'per-wave': rows[::64], 'none': rows[:0]}[pattern]


def reduction_case(M, pattern, weights, form, offset, seed=0):
    """-> dict k0, k1 [M,3], w [M] float64 (float32 values under form 'f32'; None under 'none'), rows (the inliers under T at DIST), T.
    Inliers are k0 = R k1 + t + noise of 1e-3 (so that H is no exact multiple of R); every other row sits metres away."""
    rng = np.random.default_rng([seed, M, PATTERNS.index(pattern), WEIGHTS.index(weights), FORMS.index(form), int(offset)])
    T = motion()
    k1 = rng.uniform(-1.5, 1.5, (M, 3)) + (OFFSET if offset else 0.0)
    k0 = k1 @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 1e-3, (M, 3))
    rows = inlier_rows(M, pattern)
    out = np.ones(M, bool); out[rows] = False
    k0[out] += rng.choice([-1.0, 1.0], (int(out.sum()), 3)) * rng.uniform(3.0, 9.0, (int(out.sum()), 3))
    if form == 'none':
        w = None
    else:
        w = {'uniform': np.full(M, 0.37), 'span': 10.0 ** rng.uniform(-6, 0, M), 'zeros': rng.uniform(0.1, 1.0, M)}[weights]
        if weights == 'zeros':
            w[1::3] = 0.0
            if rows.size and not w[rows].any():
                w[rows[0]] = 0.5
        if form == 'f32':
            w = w.astype(np.float32).astype(np.float64)
    return dict(k0=k0, k1=k1, w=w, rows=rows, T=T, M=M, pattern=pattern, weights=weights, form=form, offset=offset)


def reduction_cases():
    """Every (M, pattern) once; the weight form, the weight kind and the offset turn with the two indices so that every (pattern, kind),
    (pattern, form), (M, form), (kind, form) and (pattern, offset) combination occurs (tests/test_polar_oracle.py asserts it)."""
    out = []
    for im, M in enumerate(SIZES):
        for ip, pattern in enumerate(PATTERNS):
            out.append((M, pattern, WEIGHTS[(im // 3 + ip) % 3], FORMS[(im + ip) % 3], (im + ip // 2) % 2))
    return out


def effective_weights(case):
    """the normalised weights the sums run over, as float64, and whether they still have to be divided by their sum: 'f32' normalises in
    float32 (numpy's float32 sum of the compacted inlier scores, one float32 division per weight)"""
    rows, w = case['rows'], case['w']
    if w is None:
        return np.ones(rows.size), True, None
    if case['form'] == 'f32':
        w32 = w[rows].astype(np.float32)
        S32 = np.sum(w32)
        return (w32 / S32).astype(np.float64), False, float(S32)
    return w[rows], True, None


@functools.lru_cache(maxsize=None)
def reduction_reference(key):
    case = reduction_case(*key)
    if case['rows'].size == 0:
        return None
    wn, normalise, _ = effective_weights(case)
    w_full = np.zeros(case['M']); w_full[case['rows']] = wn
    return PO.kabsch(case['k0'], case['k1'], w_full, case['rows'], normalise=normalise)


def reduction_bars(case, ref):
    """(bar on H [3,3], bar on c0 [3], bar on c1 [3]) of the issue: gamma eps (sum w'|a_i||b_j| + |c0_i| sum w'|b_j| + |c1_j| sum w'|a_i|) and
    gamma eps sum w'|k|, gamma = ceil(M / 256) + 16, w' the normalised weights, a, b the centred coordinates."""
    rows = case['rows']
    wn, normalise, _ = effective_weights(case)
    if normalise:
        wn = wn / wn.sum()
    a, b = np.abs(case['k0'][rows] - ref['c0']), np.abs(case['k1'][rows] - ref['c1'])
    g = (-(-case['M'] // 256) + 16) * PO.EPS
    wa, wb = wn @ a, wn @ b
    H = g * (np.einsum('n,ni,nj->ij', wn, a, b) + np.abs(ref['c0'])[:, None] * wb[None, :] + wa[:, None] * np.abs(ref['c1'])[None, :])
    return H, g * (wn @ np.abs(case['k0'][rows])), g * (wn @ np.abs(case['k1'][rows]))


def numpy_two_pass(case):
    """the same two-pass formula in numpy float64: (H, c0, c1)"""
    rows = case['rows']
    wn, normalise, _ = effective_weights(case)
    if normalise:
        wn = wn / np.sum(wn)
    c0, c1 = wn @ case['k0'][rows], wn @ case['k1'][rows]
    return ((case['k0'][rows] - c0) * wn[:, None]).T @ (case['k1'][rows] - c1), c0, c1


# ---- the 1..7-inlier path in exact rationals ----------------------------------------------------------------------------------------------
def _rn(x):
    """a Fraction rounded once to float64, as a Fraction"""
    return Fraction(float(x))                                      # float(Fraction) rounds to nearest even


def few_inlier_model(k0, k1, w, rows, f32):
    """refine_body's n_inl <= 7 statement with every step rounded once: sequential weight sum, one division per weight, sequential centroid sums
    of k * s, then acc = fma((k0 - c0) * s, k1 - c1, acc) in k order -> (H [3,3], c0, c1) float64.  f32: the float32 score form."""
    n = len(rows)
    if f32:
        s32 = np.float32(0)
        for i in rows:
            s32 = np.float32(s32 + np.float32(w[i]))
        sk = [Fraction(float(np.float32(np.float32(w[i]) / s32))) for i in rows]
    else:
        tot = Fraction(0)
        for i in rows:
            tot = _rn(tot + Fraction(float(w[i])))
        sk = [_rn(Fraction(float(w[i])) / tot) for i in rows]
    c0, c1 = [Fraction(0)] * 3, [Fraction(0)] * 3
    for q, i in enumerate(rows):
        for d in range(3):
            pa, pb = _rn(Fraction(float(k0[i, d])) * sk[q]), _rn(Fraction(float(k1[i, d])) * sk[q])
            c0[d] = pa if q == 0 else _rn(c0[d] + pa)
            c1[d] = pb if q == 0 else _rn(c1[d] + pb)
    H = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            acc = Fraction(0)
            for q, i in enumerate(rows):
                x = _rn(_rn(Fraction(float(k0[i, r])) - c0[r]) * sk[q])
                y = _rn(Fraction(float(k1[i, c])) - c1[c])
                acc = _rn(x * y + acc)                              # fused: one rounding
            H[r, c] = float(acc)
    return H, np.array([float(v) for v in c0]), np.array([float(v) for v in c1]), n


# ---- point sets whose cross-covariance is a family's matrix ----------------------------------------------------------------------------------
def closing_points(A, M=300, seed=0, coord_scale=1.0):
    """k1: M points whitened so that sum (1/M)(k1 - c1)(k1 - c1)^T = I to rounding; k0 = k1 A^T + t: H = A to rounding.  T = [A | t] selects
    every row at any distance.  coord_scale multiplies both clouds (H by its square)."""
    rng = np.random.default_rng([0xc105, seed])
    b = rng.normal(size=(M, 3))
    b -= b.mean(0)
    L = np.linalg.cholesky(b.T @ b / M)
    b = b @ np.linalg.inv(L).T
    t = np.array([0.3, -0.2, 0.1])
    k1 = (b + np.array([0.05, 0.02, -0.04])) * coord_scale
    k0 = k1 @ A.T + t * coord_scale
    T = np.eye(4); T[:3, :3] = A; T[:3, 3] = t * coord_scale
    return k0, k1, T


# ---- spatial-compatibility sets -----------------------------------------------------------------------------------------------------------
SC2_ILL_POSED = 1e-6                                               # a row is ill posed: sigma2 < 1e-6 sigma1, or sigma2 - sigma3 < 1e-6 sigma1 under a reflection
SC2_SKIP_CAP = 0.10


@functools.lru_cache(maxsize=None)
def sc2_near_planar_case(M=193, noise=1e-6):
    """60 % of the correspondences follow one rigid motion of a plane whose z carries noise of 1e-6, and so do their images: sigma3 of every
    all-inlier consensus set is ~1e-12 sigma1 and the sign of det(U V^T) is the noise's, so a good share of the rows have a reflection to fix -- at a
    gap sigma2 - sigma3 ~ sigma2: the proper rotation is well posed."""
    import _sc2_cases as SC
    for attempt in range(20):
        rng = np.random.default_rng([0x91a, attempt])
        Q = np.concatenate([rng.uniform(0, 3, (M, 2)), rng.normal(0, noise, (M, 1))], 1)
        T = SC.ground_truth()
        P = Q @ T[:3, :3].T + T[:3, 3] + rng.normal(0, noise, (M, 3))
        wrong = rng.random(M) < 0.4
        P[wrong] = rng.uniform(-2, 4, (int(wrong.sum()), 3))
        case = SC._finish(f'near-planar-M{M}+{attempt}', P, Q, np.ones(M), SC.TAU, 1000, 20)
        if case.margin >= SC.MARGIN:
            return case
    raise AssertionError('no seed keeps the threshold margin')


def sc2_cases():
    import _sc2_cases as SC
    return [SC.synth_case(11, 257, 0.6), SC.synth_case(11, 1500, 0.9, max_seeds=70, K=64), SC.tied_case(), SC.duplicates_case(), sc2_near_planar_case()]


def sc2_posedness(S, det):
    """(ill posed, gap): gap = sigma2 + det sigma3"""
    gap = S[1] + det * S[2]
    return bool(S[1] < SC2_ILL_POSED * S[0] or (det < 0 and gap < SC2_ILL_POSED * S[0])), gap
