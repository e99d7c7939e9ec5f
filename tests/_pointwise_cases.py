"""Seeded input families of the per-keypoint streaming kernels' tests (roreg_amd/csrc/pointwise.hip: gf_finalize, det_score, inv_descriptor,
quat_to_trans).  tests/test_pointwise_oracle.py asserts on the CPU that each family meets the condition it is named for,
tests/test_hip_pointwise.py runs the same families on the device.  numpy only, no GPU imports.

  gf      -- [B,32,60] float32 raw descriptors: randn at the block tails (4 waves per block), per-keypoint scales 10^-12..10^12, 1e-25 (every
             square underflows), column norms on both sides of the 1e-4 clamp, zero keypoints / columns, means over g that cancel to 1e-3 of
             the values, float32 subnormals, one +inf and one NaN keypoint in a block of finite ones;
  ties    -- columns whose normalised float32 value is EXACTLY a bfloat16 rounding tie (low 16 bits 0x8000), by the clamp (norm < 1e-4: v / 1e-4f)
             and with a norm of exactly 1;
  det     -- [B,16,60] encodings: randn, scaled, concentrated on one group element, nearly rotation-invariant, one dead column;
  inv     -- [N,32,60] descriptors on which the ORDER of the 60-term float32 sum decides the bits;
  quat    -- un-normalised quaternions over 10^-15..10^15, every anchor, indoor and outdoor keys, optional row lists."""
import functools

import numpy as np

f32 = np.float32
F, G = 32, 60
TAILS = (1, 3, 4, 5, 257)                     # keypoints per launch around the 4-wave block
CLAMP = f32(1e-4)


def _rng(*key):
    return np.random.default_rng([sum(str(k).encode()) if isinstance(k, str) else int(k) for k in key])


# ---- gf_finalize ------------------------------------------------------------------------------------------------------------------------
NEAR_CLAMP_FACTORS = (0.5, 0.9, 0.99, 0.9999, 1 - 1e-6, 1 + 1e-6, 1.0001, 1.01, 1.1, 2.0)
GF_VALUE_CASES = ('scaled', 'underflow', 'near_clamp', 'zeros', 'cancel', 'subnormal')
ZERO_KEYPOINTS, ZERO_COLUMNS = (0, 5, 63), ((1, 0), (2, 59), (7, 31), (62, 17))       # all-zero keypoints; all-zero (keypoint, g) columns


@functools.lru_cache(maxsize=None)
def gf(name, B=64):
    """-> float32 [B,32,60], read-only."""
    rng = _rng('gf', name, B)
    x = rng.standard_normal((B, F, G))
    if name == 'randn':
        pass
    elif name == 'scaled':                    # |v| <= 6 * 1e12 < 1e18: the sum of 32 squares stays finite in float32
        x *= 10.0 ** np.linspace(-12, 12, B)[:, None, None]
    elif name == 'underflow':                 # v * v = 1e-50: zero in float32, the clamp takes over
        x *= 1e-25
    elif name == 'near_clamp':                # column norms of 1e-4 times NEAR_CLAMP_FACTORS, in turn
        fac = np.array(NEAR_CLAMP_FACTORS)[np.arange(B * G) % len(NEAR_CLAMP_FACTORS)].reshape(B, 1, G)
        x *= 1e-4 * fac / np.sqrt((x * x).sum(1, keepdims=True))
    elif name == 'zeros':
        x[list(ZERO_KEYPOINTS)] = 0.0
        for b, g in ZERO_COLUMNS:
            x[b, :, g] = 0.0
    elif name == 'cancel':                    # mean over g about 1e-3 of the values
        x -= x.mean(-1, keepdims=True)
        x += 1e-3 * rng.standard_normal((B, F, 1))
    elif name == 'subnormal':                 # bit patterns below 2^k, k = 1..23 by keypoint: every input subnormal, outputs (x 1e4) subnormal below 840
        k = 1 + np.arange(B) % 23
        bits = rng.integers(1, (1 << k)[:, None, None], (B, F, G)).astype(np.uint32)
        bits |= rng.integers(0, 2, (B, F, G)).astype(np.uint32) << np.uint32(31)
        x = bits.view(f32)
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, f32)
    x.setflags(write=False)
    return x


POISON_INF, POISON_NAN = (1, 3, 7), (3, 10, 59)            # (keypoint, channel, g) of the +inf and of the NaN


def gf_poisoned():
    """-> (clean, poisoned) float32 [5,32,60]: one block and a tail; `poisoned` differs in keypoints 1 (one +inf) and 3 (one NaN) only."""
    clean = gf('randn', 5)
    bad = clean.copy()
    bad[POISON_INF] = np.inf
    bad[POISON_NAN] = np.nan
    return clean, bad


# ---- bfloat16 rounding ties ----------------------------------------------------------------------------------------------------------------
def tie_candidates(n, seed):
    """n float32 values whose low 16 bits are 0x8000, 0.05 < |T| < 1, both signs."""
    rng = _rng('tie', seed)
    u = rng.uniform(0.05, 1.0, 2 * n).astype(f32)
    bits = (u.view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    t = bits.view(f32)
    t = t[(np.abs(t) > 0.05) & (np.abs(t) < 1.0)][:n]
    assert t.shape[0] == n
    return (t * rng.choice(np.array([-1, 1], f32), n)).astype(f32)


def _place(cols, chans, vals, B):
    """Columns (b, g) in row-major order, one planted column each: x[b, chans[i][j], g] = vals[i][j]."""
    x = np.zeros((B, F, G), f32)
    b, g = np.divmod(np.arange(cols), G)
    for j in range(chans.shape[1]):
        x[b, chans[:, j], g] = vals[:, j]
    return x, b, g


@functools.lru_cache(maxsize=None)
def ties_clamp(B=16):
    """-> (x [B,32,60], (b, f, g) of the planted values, T): every column is [.., v, ..] with v = fl(T 1e-4f) in one channel, kept where
    fl(v / 1e-4f) == T.  The column's norm |v| is below 1e-4, so the kernel's output there is fl(v / 1e-4f) = T."""
    n = B * G
    t = tie_candidates(2 * n, 1)
    v = (t * CLAMP).astype(f32)
    keep = (v / CLAMP).astype(f32) == t
    t, v = t[keep][:n], v[keep][:n]
    assert t.shape[0] == n
    ch = _rng('tie', 'clamp').integers(0, F, (n, 1))
    x, b, g = _place(n, ch, v[:, None], B)
    x.setflags(write=False)
    return x, (b, ch[:, 0], g), t


@functools.lru_cache(maxsize=None)
def ties_unit(B=16):
    """-> (x, (b, f, g), T): every column holds T and b in two channels, b within 4 ulps of sqrt(1 - T T) with fl(fl(T T) + fl(b b)) == 1.0f:
    the norm is exactly 1 (the zero channels add exactly, in any order), so the output is T."""
    n = B * G
    t = tie_candidates(2 * n, 2)
    b0 = np.sqrt(1.0 - t.astype(np.float64) ** 2).astype(f32)
    tt = (t * t).astype(f32)
    best = np.full(t.shape, np.nan, f32)
    cand = [b0]
    for _ in range(4):
        cand = [np.nextafter(cand[0], f32(0))] + cand + [np.nextafter(cand[-1], f32(2))]
    for c in sorted(cand, key=lambda c: float(np.abs(c.astype(np.float64) - b0).max())):
        ok = np.isnan(best) & ((tt + (c * c).astype(f32)).astype(f32) == f32(1))
        best[ok] = c[ok]
    keep = ~np.isnan(best)
    t, bb = t[keep][:n], best[keep][:n]
    assert t.shape[0] == n
    rng = _rng('tie', 'unit')
    fa = rng.integers(0, F, n)
    fb = (fa + rng.integers(1, F, n)) % F
    x, b, g = _place(n, np.stack((fa, fb), 1), np.stack((t, bb), 1), B)
    x.setflags(write=False)
    return x, (b, fa, g), t


def tie_census(t):
    """-> {(parity of bit 16, sign): count}."""
    bits = t.view(np.uint32)
    par, neg = (bits >> np.uint32(16)) & np.uint32(1), bits >> np.uint32(31)
    return {(int(p), int(s)): int(((par == p) & (neg == s)).sum()) for p in (0, 1) for s in (0, 1)}


# ---- det_score ----------------------------------------------------------------------------------------------------------------------------
DET_SIZES = (1, 3, 5, 203)
DET_VALUE_CASES = ('scaled', 'onehot', 'invariant')


@functools.lru_cache(maxsize=None)
def det(name, B=64):
    """-> float32 [B,16,60], read-only."""
    rng = _rng('det', name, B)
    x = rng.standard_normal((B, 16, G))
    if name == 'randn':
        pass
    elif name == 'scaled':
        x *= 10.0 ** np.linspace(-12, 12, B)[:, None, None]
    elif name == 'onehot':                    # one group element 1e6 times the others
        x *= 1e-3
        x[np.arange(B), :, np.arange(B) % G] *= 1e6
    elif name == 'invariant':
        x = 1.0 + 1e-3 * x
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, f32)
    x.setflags(write=False)
    return x


DEAD = (2, 17)                                # (keypoint, g): its 16 channels are zero there


def det_dead():
    """-> (clean, dead) [4,16,60]: one block; `dead` has keypoint 2's column g = 17 zeroed (0 / 0 in the normalisation)."""
    clean = det('randn', 4)
    dead = clean.copy()
    dead[DEAD[0], :, DEAD[1]] = 0.0
    return clean, dead


# ---- inv_descriptor -------------------------------------------------------------------------------------------------------------------------
INV_SIZES = (1, 3, 5, 257)
INV_VALUE_CASES = ('spread', 'cancel', 'channels', 'zeros')
INV_ZERO_KEYPOINTS = (0, 2, 63)


@functools.lru_cache(maxsize=None)
def inv(name, N=64):
    """-> float32 [N,32,60], read-only."""
    rng = _rng('inv', name, N)
    x = rng.standard_normal((N, F, G))
    if name == 'spread':                      # magnitudes over 2^-20..2^20 inside every row of 60
        x *= 2.0 ** rng.integers(-20, 21, (N, F, G))
    elif name == 'cancel':                    # +-2^e (1 + 0.02 randn), e = 0..23 by neighbouring pair, signs alternating: neighbours nearly cancel
        e = np.repeat(rng.integers(0, 24, (N, F, G // 2)), 2, -1)       # (0.02: the spread survives the rounding to bfloat16)
        x = 2.0 ** e * (1.0 + 0.02 * x) * np.where(np.arange(G) % 2, -1.0, 1.0)
    elif name == 'channels':                  # channels 1, 2^12, 2^24 apart, in turn (the 32 squares then differ by 2^24 and 2^48); 2^-10..2^10 inside a row
        x *= 2.0 ** (12 * (np.arange(F) % 3))[None, :, None] * 2.0 ** rng.integers(-10, 11, (N, F, G))
    elif name == 'zeros':
        x *= 2.0 ** rng.integers(-20, 21, (N, F, G))
        x[[k for k in INV_ZERO_KEYPOINTS if k < N]] = 0.0
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, f32)
    x.setflags(write=False)
    return x


def bf16_values(x):
    """float32 -> the float32 values of its bfloat16 rounding (to nearest even), by integer arithmetic."""
    b = np.ascontiguousarray(x, f32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(f32)


# ---- quat_to_trans -----------------------------------------------------------------------------------------------------------------------------
QUAT_SIZES = (1, 255, 257)
QUAT_TABLE = 300                              # keypoints per cloud when row lists are used


@functools.lru_cache(maxsize=None)
def quat(M, rows=False):
    """-> dict: q [M,4] float32 over 10^-15..10^15 (about half with w < 0), anchor [M] int64 (all 60 where M >= 60), keys0 / keys1 float64
    (even rows indoor 0..3, odd rows outdoor +-1e3), rows0 / rows1 int64 [M] into tables of QUAT_TABLE rows (with repeats, shuffled) or None."""
    rng = _rng('quat', M, int(rows))
    q = (rng.standard_normal((M, 4)) * 10.0 ** rng.uniform(-15, 15, (M, 1))).astype(f32)
    anchor = rng.permutation(np.arange(M) % 60).astype(np.int64)
    K = QUAT_TABLE if rows else M
    keys = []
    for _ in range(2):
        k = rng.uniform(0, 3, (K, 3))
        k[1::2] = rng.uniform(-1e3, 1e3, k[1::2].shape)
        keys.append(np.ascontiguousarray(k))
    r0 = r1 = None
    if rows:
        r0, r1 = rng.integers(0, K, M).astype(np.int64), rng.integers(0, K, M).astype(np.int64)
        r0[-1] = r0[0]; r1[0] = K - 1                           # a certain repeat; the table's last row
    return dict(q=q, anchor=anchor, keys0=keys[0], keys1=keys[1], rows0=r0, rows1=r1)
