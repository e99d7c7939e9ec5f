"""References of the per-keypoint streaming kernels (roreg_amd/csrc/pointwise.hip), written from the formulas of oracle/ref_numpy.py
(gf_forward's closing lines, rd_scores_from_encoding, inv_descriptor, rt_pre): float64 evaluations for the kernels held to a tolerance, the same
formulas in numpy float32 (whose own error against float64 sets each tolerance), and float32 MODELS, operation by operation, where the kernel
claims the reference's bits.  numpy only."""
import numpy as np

f32, f64 = np.float32, np.float64
G = 60
CLAMP = f32(1e-4)
FLOOR = 2.0 ** -22                            # of the output scale: gf_finalize's outputs are <= 1


# ---- gf_finalize ----------------------------------------------------------------------------------------------------------------------------
def _gf(x, clamp):
    with np.errstate(all='ignore'):
        inv = x.mean(-1)
        eqv = x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), clamp)
        inv = inv / np.maximum(np.sqrt((inv * inv).sum(1, keepdims=True)), clamp)
    return eqv, inv


def gf_finalize_f64(x):
    """x / max(||x||_channels, 1e-4) and the same of the un-normalised mean over g -> (eqv [B,32,60], inv [B,32]) float64.  The clamp is the
    float32 constant, as the kernel and the reference (a float32 tensor clamped at 1e-4) hold it."""
    return _gf(np.asarray(x, f64), f64(CLAMP))


def gf_finalize_f32(x):
    """The same formula with every operation in numpy float32 (oracle/ref_numpy.py gf_forward): NOT the kernel's summation order; its error
    against gf_finalize_f64 is the yardstick of the kernel's."""
    x = np.asarray(x)
    assert x.dtype == f32
    eqv, inv = _gf(x, CLAMP)
    assert eqv.dtype == f32 and inv.dtype == f32
    return eqv, inv


def bar(err_f32):
    """4 x the float32 formula's own maximum error, never below 2^-22 of the output scale."""
    return max(4.0 * float(err_f32), FLOOR)


def max_err(got, want):
    return float(np.abs(np.asarray(got, f64) - want).max())


def bf16_bits(x):
    """float32 -> uint16 bfloat16 bit patterns, round to nearest even, by integer arithmetic (finite values)."""
    b = np.ascontiguousarray(x, f32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_bits_truncated(x):
    return (np.ascontiguousarray(x, f32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


# ---- det_score -------------------------------------------------------------------------------------------------------------------------------
def det_score_f64(enc, P):
    """network/rot_detect.py:47-52 in float64, no final cast: normalise the 16 channels at every g (no epsilon), c[a] = sum_f sum_b
    f[f,P[a,b]] f[f,b], unbiased std over the 60 a."""
    f = np.asarray(enc, f64)
    with np.errstate(all='ignore'):
        f = f / np.sqrt((f * f).sum(1, keepdims=True))
    c = np.empty((f.shape[0], G))
    for a in range(G):
        c[:, a] = (f[:, :, P[a]] * f).sum((1, 2))
    d = c - c.mean(1, keepdims=True)
    return np.sqrt((d * d).sum(1) / (G - 1))


# ---- inv_descriptor --------------------------------------------------------------------------------------------------------------------------
def _sum_f32(a, order):
    """float32 sum over the last axis (8 <= n <= 128), every addition rounded: 'pairwise' = numpy's contiguous reduction (eight strided
    partial sums, a fixed tree, the tail), 'sequential' = left to right."""
    a = np.asarray(a)
    assert a.dtype == f32
    n = a.shape[-1]
    if order == 'sequential':
        s = a[..., 0].copy()
        for i in range(1, n):
            s = s + a[..., i]
        return s
    assert order == 'pairwise' and 8 <= n <= 128
    r = [a[..., j].copy() for j in range(8)]
    nb = n - n % 8
    for i in range(8, nb, 8):
        for j in range(8):
            r[j] = r[j] + a[..., i + j]
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(nb, n):
        s = s + a[..., i]
    assert s.dtype == f32
    return s


def inv_descriptor_model(eqv, order='pairwise', divide='f64'):
    """test/matcher.py:69-72 operation by operation in float32, as inv_descriptor_kernel states it: the sum of the 60 in `order`, the mean by
    `divide` ('f64': float64 quotient by 60 cast back, what np.mean does; 'f32': a correctly rounded float32 division; 'recip': times
    float32(1/60)), the 32 squares summed pairwise, sqrt, + 1e-5f, divide."""
    s = _sum_f32(np.asarray(eqv, f32), order)
    if divide == 'f64':
        m = (s.astype(f64) / 60.0).astype(f32)
    elif divide == 'f32':
        m = s / f32(60)
    else:
        assert divide == 'recip'
        m = s * f32(1.0 / 60.0)
    nrm = np.sqrt(_sum_f32(m * m, 'pairwise')) + f32(1e-5)
    out = m / nrm[..., None]
    assert out.dtype == f32
    return out


# ---- quat_to_trans ---------------------------------------------------------------------------------------------------------------------------
def quat_normalize_model(q):
    """The kernel's stated order in float32: ((w w + x x) + y y) + z z, sqrt, four divides."""
    q = np.asarray(q)
    assert q.dtype == f32
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    n = np.sqrt(((w * w + x * x) + y * y) + z * z)
    out = q / n[:, None]
    assert out.dtype == f32
    return out


def quat_to_trans_model(qn, anchor, R_f32, keys0, keys1):
    """quat_to_trans_body after the normalisation, in numpy: utils/r_eval.py:90-106 in float32 left to right, R = m @ Rgroup[a] and
    t = k0 - k1 @ R^T in float64 with sums of three taken in order -> [M,3,4] float64."""
    qn = np.asarray(qn)
    assert qn.dtype == f32 and R_f32.dtype == f32
    w, x, y, z = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
    one = f32(1)

    def two(a, b):
        return (f32(2) * a) * b
    m = np.stack([(one - two(y, y)) - two(z, z), two(x, y) - two(z, w), two(x, z) + two(y, w),
                  two(x, y) + two(z, w), (one - two(x, x)) - two(z, z), two(y, z) - two(x, w),
                  two(x, z) - two(y, w), two(y, z) + two(x, w), (one - two(x, x)) - two(y, y)], 1)
    assert m.dtype == f32
    m = m.astype(f64).reshape(-1, 3, 3)
    A = R_f32[np.asarray(anchor)].astype(f64)
    out = np.empty((qn.shape[0], 3, 4))
    for r in range(3):
        for c in range(3):
            out[:, r, c] = (m[:, r, 0] * A[:, 0, c] + m[:, r, 1] * A[:, 1, c]) + m[:, r, 2] * A[:, 2, c]
        rot = (keys1[:, 0] * out[:, r, 0] + keys1[:, 1] * out[:, r, 1]) + keys1[:, 2] * out[:, r, 2]
        out[:, r, 3] = keys0[:, r] - rot
    return out


def trans_bar(keys0, keys1):
    """8 double ulps at magnitude max(1, |k0|, |k1|) per correspondence -> [M,1,1]: the rotation's entries are sums of three products that are
    exact in float64 (float32 x float32), the translation a sum of three rounded products of size <= |k1| and one subtraction."""
    m = np.maximum(1.0, np.maximum(np.linalg.norm(keys0, axis=1), np.linalg.norm(keys1, axis=1)))
    return (8.0 * 2.0 ** -52 * m)[:, None, None]
