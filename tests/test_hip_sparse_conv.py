"""The sparse-convolution kernels and the FCGF backbone on the device (csrc/sparse_conv.hip "v6j", roreg_amd/backbone/fcgf.py) against their
numpy definition (tests/_sparse_conv_oracle.py): the maps integer for integer, every layer shape within the float32 summation bound
gamma_{n+2} sum |x||w| of the float64 oracle, the epilogue, the whole network within 4 x the float32 oracle's own error, and an item's
features bit for bit whatever it is batched with."""
import numpy as np
import pytest
import torch

import _sparse_conv_oracle as O
from test_sparse_conv_oracle import NARROW, random_coords

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def block(lo, hi, item=0):
    r = np.arange(lo, hi)
    z, y, x = np.meshgrid(r, r, r, indexing='ij')
    return np.stack([np.full(x.size, item), x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)


def map_cases():
    line = np.stack([np.zeros(40), np.arange(-20, 20), np.full(40, 3), np.full(40, -5)], 1).astype(np.int32)
    one = random_coords(21, 100, -5, 7)
    cases = {'one voxel': np.array([[0, 5, -3, 2]], np.int32), 'full 3^3 block': block(-1, 2), '2x2x2 across the origin': block(-1, 1), 'line': line,
             'two coincident items': np.concatenate([one, one + np.array([1, 0, 0, 0], np.int32)])}
    for n in (63, 64, 65, 257):
        cases[f'{n} random voxels'] = random_coords(n, n, -6, 6)
    return cases


CASES = map_cases()


def device_levels(coords):
    """-> per level (coords, cuts) on the host, parents; through hip.sparse_stride_map at tensor strides 1, 2, 4."""
    from roreg_amd import hip
    lv, cuts, parents = [dev(coords)], [dev(O.item_cuts(coords))], []
    for l in range(3):
        sm = hip.sparse_stride_map(lv[-1], cuts[-1], 1 << l)
        lv.append(sm.coords); cuts.append(sm.cuts); parents.append(sm.parent.cpu().numpy())
    return lv, cuts, parents


@pytest.mark.parametrize('name', list(CASES))
def test_maps_equal_the_oracle(name):
    from roreg_amd import hip
    coords = CASES[name]
    C, P = O.ResUNetBN2C({}).levels(coords)
    lv, cuts, parents = device_levels(coords)
    for l in range(4):
        assert np.array_equal(lv[l].cpu().numpy(), C[l]), (name, l)
        assert np.array_equal(cuts[l].cpu().numpy(), O.item_cuts(C[l])), (name, l)
        if l < 3:
            assert np.array_equal(parents[l], P[l]), (name, l)
    for l in range(4):
        for k in (3, 5, 7) if l == 0 else (3,):
            assert np.array_equal(hip.sparse_kernel_map(lv[l], lv[l], k, 1 << l).cpu().numpy(), O.kernel_map(C[l], C[l], k, 1 << l)), (name, l, k)
    for l in range(3):
        assert np.array_equal(hip.sparse_kernel_map(lv[l], lv[l + 1], 3, 1 << l).cpu().numpy(), O.kernel_map(C[l], C[l + 1], 3, 1 << l)), (name, l, 'stride 2')
        assert np.array_equal(hip.sparse_kernel_map(lv[l + 1], lv[l], 3, -(1 << l)).cpu().numpy(), O.transposed_map(C[l + 1], C[l], 1 << l)), (name, l, 'transposed')


@pytest.mark.parametrize('bad', [[0, 1 << 15, 0, 0], [0, 0, -(1 << 15) - 1, 0], [1 << 15, 0, 0, 1]])
def test_a_key_out_of_range_raises_and_the_next_call_is_correct(bad):
    from roreg_amd import hip
    good = CASES['65 random voxels']
    coords = np.concatenate([good, np.asarray([bad], np.int32)]) if bad[0] else np.concatenate([good[:30], np.asarray([bad], np.int32), good[30:]])
    cuts = dev(np.array([0, coords.shape[0]], np.int32))
    with pytest.raises(hip.HipError, match='outside'):
        hip.sparse_stride_map(dev(coords), cuts, 1)
    with pytest.raises(hip.HipError, match='outside'):
        hip.sparse_kernel_map(dev(coords), dev(good), 3, 1)
    # the largest coordinates that fit do, and a neighbour query past them is simply absent
    edge = np.array([[0, (1 << 15) - 1, -(1 << 15), 0], [0, (1 << 15) - 2, -(1 << 15), 0]], np.int32)
    assert np.array_equal(hip.sparse_kernel_map(dev(edge), dev(edge), 3, 1).cpu().numpy(), O.kernel_map(edge, edge, 3, 1))
    sm = hip.sparse_stride_map(dev(good), dev(np.array([0, 65], np.int32)), 1)
    want, parent = O.stride_map(good, 1)
    assert np.array_equal(sm.coords.cpu().numpy(), want) and np.array_equal(sm.parent.cpu().numpy(), parent)
    assert np.array_equal(hip.sparse_kernel_map(dev(good), dev(good), 3, 1).cpu().numpy(), O.kernel_map(good, good, 3, 1))


# ---- one convolution per layer shape of the network: 257 voxels (five 64-row tiles, the last one ragged) -------------------------------------
C257 = CASES['257 random voxels']
LAYERS = [(1, 32, 5, 'same', False), (1, 32, 7, 'same', False), (32, 32, 3, 'same', False), (32, 64, 3, 'down', False), (256, 128, 3, 'up', False),
          (256, 64, 3, 'up', False), (96, 64, 1, 'same', False), (64, 32, 1, 'same', True)]


def layer_map(kind, k):
    coarse, _ = O.stride_map(C257, 1)
    if kind == 'same':
        return O.kernel_map(C257, C257, k, 1), 257
    if kind == 'down':
        return O.kernel_map(C257, coarse, 3, 1), 257
    return O.transposed_map(coarse, C257, 1), coarse.shape[0]


@pytest.mark.parametrize('cin,cout,k,kind,bias', LAYERS)
def test_convolution_per_layer_shape(cin, cout, k, kind, bias):
    from roreg_amd import hip
    rng = np.random.default_rng([cin, cout, k])
    M, n_in = layer_map(kind, k)
    x = rng.standard_normal((n_in, cin)).astype(np.float32)
    W = (rng.standard_normal((k ** 3, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if bias else None
    got = hip.sparse_conv(dev(x), dev(W), dev(M), shift=dev(b) if bias else None).cpu().numpy()
    want = O.conv(x, W, M, np.float64)
    S, terms = O.conv_bound(x, W, M)
    if bias:
        want, S, terms = want + b.astype(np.float64), S + np.abs(b.astype(np.float64)), terms + 1
    bound = O.gamma(terms + 2)[:, None] * S
    err = np.abs(got.astype(np.float64) - want)
    print(f'({cin},{cout},{k ** 3} {kind}): max err {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, terms up to {terms.max()}')
    assert got.shape == want.shape and (err <= bound).all()
    assert np.abs(want).max() > 0.5                                       # a wrong neighbour or weight index misses the bound by orders of magnitude


def test_map_and_first_layer_with_more_than_2_31_map_entries():
    """A full 185^3 grid under a 7^3 kernel: 6,331,625 rows x 343 offsets = 2.17e9 map entries, past 2^31 (the index on n_out K must be 64-bit in
    the lookup and in the first layer's kernel).  The expected map is analytic: row = x + 185 y + 185^2 z; checked on the first, the last and
    random rows, where a 32-bit index would have written (or read) entries of other rows."""
    from roreg_amd import hip
    side, k, lo = 185, 7, -90
    n = side ** 3
    assert n * k ** 3 > 2 ** 31
    r = np.arange(side, dtype=np.int32) + lo
    z, y, x = np.meshgrid(r, r, r, indexing='ij')
    coords = np.stack([np.zeros(n, np.int32), x.ravel(), y.ravel(), z.ravel()], 1)
    cd = dev(coords)
    M = hip.sparse_kernel_map(cd, cd, k, 1)
    assert tuple(M.shape) == (n, k ** 3)
    rng = np.random.default_rng(2)
    rows = np.unique(np.concatenate([np.arange(40), np.arange(n - 40, n), rng.integers(0, n, 300), (2 ** 31 // k ** 3) + np.arange(-20, 20)]))
    off = O.offsets(k)
    p = coords[rows, 1:].astype(np.int64)[:, None, :] - lo + off[None]                          # [rows, K, 3] grid positions of the neighbours
    inside = ((p >= 0) & (p < side)).all(2)
    want = np.where(inside, p[..., 0] + side * p[..., 1] + side * side * p[..., 2], -1).astype(np.int32)
    assert np.array_equal(M[dev(rows)].cpu().numpy(), want)
    xs = rng.standard_normal((n, 1)).astype(np.float32)
    W = rng.standard_normal((k ** 3, 1, 32)).astype(np.float32)
    got = hip.sparse_conv(dev(xs), dev(W), M)[dev(rows)].cpu().numpy()
    del M
    xn = np.where(want >= 0, xs[np.maximum(want, 0), 0], 0).astype(np.float64)                   # [rows, K]; an absent neighbour is no term
    y64, S = xn @ W[:, 0].astype(np.float64), np.abs(xn) @ np.abs(W[:, 0].astype(np.float64))
    assert (np.abs(got - y64) <= O.gamma((want >= 0).sum(1) + 2)[:, None] * S).all() and np.abs(y64).max() > 10


def test_epilogue_and_column_windows():
    """scale, shift, residual, relu; x, residual and out as column windows of wider buffers whose other columns stay bit-identical."""
    from roreg_amd import hip
    rng = np.random.default_rng(8)
    M = O.kernel_map(C257, C257, 3, 1)
    cin, cout = 32, 64
    xw = rng.standard_normal((257, 50)).astype(np.float32); x = xw[:, 11:11 + cin]
    rw = rng.standard_normal((257, 70)).astype(np.float32); r = rw[:, 3:3 + cout]
    W = (rng.standard_normal((27, cin, cout)) / np.sqrt(cin)).astype(np.float32)
    scale, shift = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    xd, rd, Wd, Md = dev(xw), dev(rw), dev(W), dev(M)
    raw = hip.sparse_conv(xd[:, 11:11 + cin], Wd, Md)
    assert torch.equal(raw, hip.sparse_conv(dev(x), Wd, Md))                                   # a window of x is x
    y = raw.cpu().numpy().astype(np.float64)
    for use_scale, use_res, relu in [(True, False, False), (True, True, True), (False, True, False), (False, False, True), (True, True, False)]:
        buf = rng.standard_normal((257, 100)).astype(np.float32)
        bd = dev(buf)
        out = hip.sparse_conv(xd[:, 11:11 + cin], Wd, Md, scale=dev(scale) if use_scale else None, shift=dev(shift) if use_scale else None,
                              residual=rd[:, 3:3 + cout] if use_res else None, relu=relu, out=bd[:, 20:20 + cout])
        assert out.data_ptr() == bd[:, 20:].data_ptr()
        got = bd.cpu().numpy()
        keep = np.ones(100, bool); keep[20:20 + cout] = False
        assert got[:, keep].tobytes() == buf[:, keep].tobytes()
        s, b = (scale.astype(np.float64), shift.astype(np.float64)) if use_scale else (1.0, 0.0)
        res = r.astype(np.float64) if use_res else 0.0
        want = y * s + b + res
        bound = O.gamma(3) * (np.abs(y * s) + np.abs(b) + np.abs(res))                          # three roundings at most: fmaf, the residual add
        want = np.maximum(want, 0) if relu else want                                          # relu is 1-Lipschitz
        assert (np.abs(got[:, 20:20 + cout] - want) <= bound).all(), (use_scale, use_res, relu)
        assert (got[:, 20:20 + cout] >= 0).all() == relu


def test_l2norm():
    from roreg_amd import hip
    x = np.random.default_rng(4).standard_normal((300, 32)).astype(np.float32)
    got = hip.sparse_l2norm(dev(x)).cpu().numpy()
    want = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    assert np.abs(got - want).max() <= O.gamma(32 + 3)


# ---- the whole network -------------------------------------------------------------------------------------------------------------------
def device_model(sd, k1, **kw):
    from roreg_amd.backbone import fcgf
    model = fcgf.ResUNetBN2C(1, 32, normalize_feature=True, conv1_kernel_size=k1, **kw)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model.cuda().eval()


def check_network(model, sd, k1, coords, what):
    maps = O.ResUNetBN2C(sd, True, k1).maps(coords)
    o64 = O.ResUNetBN2C(sd, True, k1, np.float64).forward(coords, maps)
    o32 = O.ResUNetBN2C(sd, True, k1, np.float32).forward(coords, maps)
    got = model(dev(coords), O.item_cuts(coords)).cpu().numpy()
    e32, e_dev = np.abs(o32 - o64).max(), np.abs(got - o64).max()
    print(f'{what}: {coords.shape[0]} voxels, E32 = max|oracle_f32 - oracle_f64| = {e32:.3e}, max|device - oracle_f64| = {e_dev:.3e}')
    assert got.shape == o64.shape and got.dtype == np.float32 and np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-5
    assert e_dev <= 4 * e32


def test_narrow_network_on_257_voxels():
    sd = O.random_state_dict(11, conv1_kernel_size=5, **NARROW)
    check_network(device_model(sd, 5, **NARROW), sd, 5, C257, 'narrow network')


def test_full_width_network_on_a_cloud():
    from roreg_amd import synth, voxel
    from roreg_amd.backbone import fcgf
    p0, _, _ = synth.make_dense_pair(7, 4000)
    vc = voxel.downsample(p0, 0.05, mode='first')
    coords = np.concatenate([np.zeros((vc.coords.shape[0], 1), np.int32), vc.coords], 1)
    assert 1000 < coords.shape[0] <= 4000
    model = fcgf.ResUNetBN2C(1, 32, normalize_feature=True, conv1_kernel_size=5)
    sd = {k: v.numpy() for k, v in synth.seeded_state_dict(model, 5).items()}
    assert np.abs(sd['norm3.bn.running_mean']).max() > 0.01 and np.abs(sd['norm3.bn.running_var'] - 1).max() > 0.1           # statistics not trivial
    check_network(model.cuda().eval(), sd, 5, coords, 'full-width network')


# ---- an item's result does not depend on its batch -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_cloud():
    from roreg_amd import synth
    p0, _, _ = synth.make_dense_pair(3, 2000)
    kps = p0[np.random.default_rng(1).choice(2000, 64, replace=False)].astype(np.float64)
    return p0.astype(np.float64), kps


def test_three_rotations_in_one_batch_equal_each_alone(small_cloud):
    from roreg_amd import synth, testset
    from roreg_amd.backbone import fcgf
    from roreg_amd.group import tables
    pts, _ = small_cloud
    R = tables().R
    full = fcgf.ResUNetBN2C(conv1_kernel_size=5)
    synth.seeded_state_dict(full, 9)
    for model in (device_model(O.random_state_dict(12, conv1_kernel_size=3, **NARROW), 3, **NARROW), full.cuda().eval()):
        vox = [testset._voxelise((pts @ R[g].T).astype(np.float32), 0.05) for g in (0, 17, 42)]
        c4, cuts = testset._batch_coords([c for _, c in vox])
        together = model(c4, cuts)
        for i in range(3):
            alone = model(*testset._batch_coords([vox[i][1]]))
            assert alone.shape[0] == cuts[i + 1] - cuts[i] > 300
            assert torch.equal(alone.view(torch.int32), together[int(cuts[i]):int(cuts[i + 1])].view(torch.int32)), i


def test_batched_extraction_equals_the_plugin_path_bitwise(small_cloud):
    from roreg_amd import testset
    pts, kps = small_cloud
    sd = O.random_state_dict(12, conv1_kernel_size=3, **NARROW)
    model = device_model(sd, 3, **NARROW)
    batched = testset.extract_group_features(model, pts, kps, voxel_size=0.05, rot_batch=3)
    plugin = testset.assemble_group_features(testset.FCGFBackbone(model, 0.05), pts, kps)
    assert batched.shape == (64, 32, 60) and batched.dtype == np.float32 and np.isfinite(batched).all()
    assert np.array_equal(batched.view(np.uint8), plugin.view(np.uint8))
    assert np.abs(batched[:, :, 0] - batched[:, :, 7]).max() > 1e-3                             # the columns are different rotations' features
