"""CPU half of the sparse-convolution / FCGF backbone tests: the numpy oracle (tests/_sparse_conv_oracle.py, dictionary lookups on integer
coordinates) against an independent restatement through torch's dense conv3d / conv_transpose3d on a zero-filled grid sampled at the active
sites, which also settles the weight-index convention kappa <-> W[:, :, z, y, x]; the map properties; the state-dict names; the interface."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import _sparse_conv_oracle as O
from conftest import ROOT

V6J = ('roreg_sparse_map_workspace', 'roreg_sparse_stride_map', 'roreg_sparse_kernel_map', 'roreg_sparse_conv', 'roreg_sparse_l2norm')


def random_coords(seed, n, lo, hi, items=1):
    """n distinct voxels per item in [lo, hi)^3, shuffled: int32 [items n, 4], items contiguous."""
    rng = np.random.default_rng(seed)
    side = hi - lo
    rows = []
    for b in range(items):
        flat = rng.choice(side ** 3, size=n, replace=False)
        xyz = np.stack([flat % side, flat // side % side, flat // (side * side)], 1) + lo
        rows.append(np.concatenate([np.full((n, 1), b), xyz], 1))
    return np.concatenate(rows).astype(np.int32)


# ---- the dense restatement: one item, coordinates in [-h, h)^3, level grid of tensor stride ts has 2h / ts sites per axis ----------------------
def to_dense(x, coords, h, ts):
    g = 2 * h // ts
    d = torch.zeros((1, x.shape[1], g, g, g), dtype=torch.float64)
    i = (np.asarray(coords)[:, 1:].astype(np.int64) + h) // ts
    d[0, :, i[:, 2], i[:, 1], i[:, 0]] = torch.from_numpy(np.asarray(x, np.float64)).T
    return d


def sample(d, coords, h, ts):
    i = (np.asarray(coords)[:, 1:].astype(np.int64) + h) // ts
    return d[0, :, i[:, 2], i[:, 1], i[:, 0]].T.numpy()


def torch_weight(W, k):
    """[K, Cin, Cout], kappa = kx + k ky + k^2 kz -> [Cout, Cin, kz, ky, kx]."""
    W = torch.from_numpy(np.asarray(O.as_kernel(W), np.float64))
    return W.reshape(k, k, k, W.shape[1], W.shape[2]).permute(4, 3, 0, 1, 2).contiguous()


def dense_conv(x, W, coords_in, coords_out, h, ts_in, k, kind):
    d = to_dense(x, coords_in, h, ts_in)
    w = torch_weight(W, k)
    if kind == 'same':
        return sample(TF.conv3d(d, w, padding=k // 2), coords_out, h, ts_in)
    if kind == 'down':
        return sample(TF.conv3d(d, w, stride=2, padding=1), coords_out, h, 2 * ts_in)
    return sample(TF.conv_transpose3d(d, w.permute(1, 0, 2, 3, 4), stride=2, padding=1, output_padding=1), coords_out, h, ts_in // 2)


def close(a, b, tol=1e-12):
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize('k', [3, 5, 7])
def test_stride1_equals_dense_conv3d(k):
    rng = np.random.default_rng(k)
    c = random_coords(10 + k, 150, -4, 4)
    x, W = rng.standard_normal((150, 3)), rng.standard_normal((k ** 3, 3, 5))
    M = O.kernel_map(c, c, k, 1)
    assert (M >= 0).sum() > 150 and (M < 0).any() and (M[:, k ** 3 // 2] == np.arange(150)).all()
    assert close(O.conv(x, W, M), dense_conv(x, W, c, c, 4, 1, k, 'same'))


def test_stride2_and_transposed_equal_dense():
    rng = np.random.default_rng(2)
    c = random_coords(3, 120, -4, 4)
    assert (c[:, 1:] < 0).any() and (c[:, 1:] == -1).any()
    coarse, parent = O.stride_map(c, 1)
    assert (coarse[:, 1:] % 2 == 0).all() and coarse[:, 1:].min() == -4                   # a floor: -1 and -2 share the coarse voxel -2
    assert np.array_equal(coarse[parent][:, 1:], np.floor(c[:, 1:] / 2).astype(np.int32) * 2)
    x, W = rng.standard_normal((120, 3)), rng.standard_normal((27, 3, 4))
    Md = O.kernel_map(c, coarse, 3, 1)
    assert close(O.conv(x, W, Md), dense_conv(x, W, c, coarse, 4, 1, 3, 'down'))
    xc, Wt = rng.standard_normal((coarse.shape[0], 4)), rng.standard_normal((27, 4, 2))
    Mt = O.transposed_map(coarse, c, 1)
    assert ((Mt >= 0).sum(1) <= 8).all() and ((Mt >= 0).sum(1) >= 1).all()
    assert close(O.conv(xc, Wt, Mt), dense_conv(xc, Wt, coarse, c, 4, 2, 3, 'up'))
    # at tensor stride 2 the offsets are in units of 2
    c2, _ = O.stride_map(coarse, 2)
    assert close(O.conv(xc, Wt, O.kernel_map(coarse, c2, 3, 2)), dense_conv(xc, Wt, coarse, c2, 4, 2, 3, 'down'))
    assert close(O.conv(xc, Wt, O.kernel_map(coarse, coarse, 3, 2)), dense_conv(xc, Wt, coarse, coarse, 4, 2, 3, 'same'))


def test_transposed_map_is_the_swapped_strided_map():
    c = random_coords(5, 200, -6, 6, items=2)
    coarse, _ = O.stride_map(c, 1)
    Mf, Mt = O.kernel_map(c, coarse, 3, 1), O.transposed_map(coarse, c, 1)
    pairs_f = {(u, k, v) for u, k in zip(*np.nonzero(Mf >= 0)) for v in [Mf[u, k]]}
    pairs_t = {(Mt[v, k], k, v) for v, k in zip(*np.nonzero(Mt >= 0))}
    assert pairs_f == pairs_t and len(pairs_f) >= 400


def test_coarse_numbering_and_contiguous_items():
    c = random_coords(7, 90, -8, 8, items=3)
    C, parents = O.ResUNetBN2C({}).levels(c)
    for l in range(3):
        first = np.full(C[l + 1].shape[0], -1)
        for i in range(C[l].shape[0] - 1, -1, -1):
            first[parents[l][i]] = i
        assert (np.diff(first) > 0).all() and first[0] == 0                                # ascending lowest fine row
        assert np.array_equal(C[l + 1][:, 0], C[l][first, 0])
        assert len({tuple(r) for r in C[l + 1].tolist()}) == C[l + 1].shape[0]             # unique per item
    for l in range(4):
        cuts = O.item_cuts(C[l])                                                           # asserts ascending = contiguous
        assert cuts.shape[0] == 4 and cuts[-1] == C[l].shape[0] and (np.diff(cuts) > 0).all()
        assert (C[l][:, 1:] % (1 << l) == 0).all()
    # two items with the same coordinates do not see each other
    two = np.concatenate([c[:90], c[:90] + np.array([1, 0, 0, 0], np.int32)])
    M = O.kernel_map(two, two, 3, 1)
    assert (M[:90] < 90).all() and (M[90:][M[90:] >= 0] >= 90).all() and np.array_equal(M[:90], np.where(M[90:] >= 0, M[90:] - 90, -1))


NARROW = dict(channels=(None, 4, 8, 8, 16), tr_channels=(None, 8, 8, 8, 16))


def dense_network(sd, coords, k1, normalize):
    """ResUNetBN2C restated with dense convolutions; BatchNorm through torch's own eval-mode batch_norm on the sampled rows."""
    h = 8
    C, _ = O.ResUNetBN2C({}).levels(coords)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))

    def bn(y, name):
        return TF.batch_norm(t(y), t(sd[f'{name}.bn.running_mean']), t(sd[f'{name}.bn.running_var']), t(sd[f'{name}.bn.weight']), t(sd[f'{name}.bn.bias']),
                             False, 0.1, 1e-5).numpy()

    def block(x, name, l):
        y = np.maximum(bn(dense_conv(x, sd[f'{name}.conv1.kernel'], C[l], C[l], h, 1 << l, 3, 'same'), f'{name}.norm1'), 0)
        return np.maximum(bn(dense_conv(y, sd[f'{name}.conv2.kernel'], C[l], C[l], h, 1 << l, 3, 'same'), f'{name}.norm2') + x, 0)

    out = block(bn(dense_conv(np.ones((C[0].shape[0], 1)), sd['conv1.kernel'], C[0], C[0], h, 1, k1, 'same'), 'norm1'), 'block1', 0)
    skip = [out]
    for l in (2, 3, 4):
        out = block(bn(dense_conv(out, sd[f'conv{l}.kernel'], C[l - 2], C[l - 1], h, 1 << (l - 2), 3, 'down'), f'norm{l}'), f'block{l}', l - 1)
        skip.append(out)
    for l in (4, 3, 2):
        out = block(bn(dense_conv(out, sd[f'conv{l}_tr.kernel'], C[l - 1], C[l - 2], h, 1 << (l - 1), 3, 'up'), f'norm{l}_tr'), f'block{l}_tr', l - 2)
        out = np.concatenate([out, skip[l - 2]], 1)
    out = np.maximum(out @ O.as_kernel(sd['conv1_tr.kernel'])[0].astype(np.float64), 0)
    out = out @ O.as_kernel(sd['final.kernel'])[0].astype(np.float64) + sd['final.bias'].astype(np.float64)
    return out / np.linalg.norm(out, axis=1, keepdims=True) if normalize else out


@pytest.mark.parametrize('k1', [3, 5])
def test_narrow_network_equals_dense_restatement(k1):
    sd = O.random_state_dict(11, conv1_kernel_size=k1, **NARROW)
    c = random_coords(13, 300, -8, 8)
    for normalize in (False, True):
        got = O.ResUNetBN2C(sd, normalize, k1).forward(c)
        assert got.shape == (300, 32) and np.isfinite(got).all() and np.abs(got).max() > 1e-3
        assert close(got, dense_network(sd, c, k1, normalize))
    # float32 products and sums stay close to float64; a flat [Cin, Cout] kernel of size 1 is the same layer
    f32 = O.ResUNetBN2C(sd, True, k1, np.float32).forward(c)
    assert f32.dtype == np.float32 and np.abs(f32 - got).max() < 1e-4
    flat = dict(sd, **{n: sd[n][0] for n in ('conv1_tr.kernel', 'final.kernel')})
    assert np.array_equal(O.ResUNetBN2C(flat, True, k1).forward(c), got)


# written out by hand from backbone/fcgf/resunet.py (ResUNetBN2C, in 1, out 32, conv1_kernel_size 5) and residual_block.py
def _bn_names(n, c):
    return {f'{n}.bn.weight': (c,), f'{n}.bn.bias': (c,), f'{n}.bn.running_mean': (c,), f'{n}.bn.running_var': (c,), f'{n}.bn.num_batches_tracked': ()}


def _block_names(n, c):
    return {f'{n}.conv1.kernel': (27, c, c), **_bn_names(f'{n}.norm1', c), f'{n}.conv2.kernel': (27, c, c), **_bn_names(f'{n}.norm2', c)}


HAND = {
    'conv1.kernel': (125, 1, 32), **_bn_names('norm1', 32), **_block_names('block1', 32),
    'conv2.kernel': (27, 32, 64), **_bn_names('norm2', 64), **_block_names('block2', 64),
    'conv3.kernel': (27, 64, 128), **_bn_names('norm3', 128), **_block_names('block3', 128),
    'conv4.kernel': (27, 128, 256), **_bn_names('norm4', 256), **_block_names('block4', 256),
    'conv4_tr.kernel': (27, 256, 128), **_bn_names('norm4_tr', 128), **_block_names('block4_tr', 128),
    'conv3_tr.kernel': (27, 256, 64), **_bn_names('norm3_tr', 64), **_block_names('block3_tr', 64),
    'conv2_tr.kernel': (27, 128, 64), **_bn_names('norm2_tr', 64), **_block_names('block2_tr', 64),
    'conv1_tr.kernel': (1, 96, 64), 'final.kernel': (1, 64, 32), 'final.bias': (1, 32),
}


def test_state_dict_names_and_strict_loading():
    from roreg_amd.backbone import fcgf
    assert fcgf.load_model('ResUNetBN2C') is fcgf.ResUNetBN2C and fcgf.load_model('nope') is None
    model = fcgf.ResUNetBN2C(1, 32, normalize_feature=True, conv1_kernel_size=5)
    have = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert have == HAND and list(have) == list(HAND)
    assert O.state_dict_spec() == HAND
    for flat in (False, True):
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in O.random_state_dict(3, k1_flat=flat).items()}
        assert sd['final.kernel'].dim() == (2 if flat else 3)
        model.load_state_dict(sd, strict=True)
        assert torch.equal(model.final.kernel[0], sd['final.kernel'].reshape(64, 32)) and torch.equal(model.block3_tr.norm2.bn.running_var, sd['block3_tr.norm2.bn.running_var'])
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in sd.items() if k != 'conv3.kernel'}, strict=True)
    narrow = fcgf.ResUNetBN2C(conv1_kernel_size=3, **NARROW)
    assert {k: tuple(v.shape) for k, v in narrow.state_dict().items()} == O.state_dict_spec(conv1_kernel_size=3, **NARROW)


def test_v6j_names_in_header_abi_and_library():
    from roreg_amd import _abi, hip
    raw = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    assert 'v6j' in raw and _abi.ABI_VERSION == 6
    assert int(re.search(r'#define\s+ROREG_ABI_VERSION\s+(\d+)', header).group(1)) == 6
    L = hip.lib()
    for name in V6J:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _abi.PROTOTYPES and hasattr(L, name)
        assert hasattr(hip, name[len('roreg_'):]) or name.endswith('workspace')
    assert L.roreg_abi_version() == 6
    assert L.roreg_sparse_map_workspace(1000) > 0 and L.roreg_sparse_map_workspace(-1) == 0
    assert len(_abi.PROTOTYPES['roreg_sparse_conv'][1]) == 17
