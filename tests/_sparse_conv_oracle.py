"""numpy restatement of the sparse convolutions and of the FCGF backbone built from them (include/roreg_hip.h "v6j"; roreg_amd/csrc/sparse_conv.hip,
roreg_amd/backbone/fcgf.py): what the device must compute.  Written from the definitions of MinkowskiEngine 0.5.2 (kernel_region.hpp's offset
order, coordinate_map_manager.cpp's stride and transposed maps) and of ResUNetBN2C (backbone/fcgf/resunet.py), with dictionary lookups on
integer coordinates; `dtype` is the precision of every product and sum.

  coordinates : a sparse tensor at tensor stride ts is int32 [m,4] rows (item, x, y, z), x, y, z multiples of ts, an item's rows contiguous.
  stride 2    : coarse coordinate = floor(c / (2 ts)) * (2 ts) per axis (a floor: -1 -> -2); coarse rows are numbered in ascending order of their
                lowest fine row (this project's rule; ME's own order is a property of its hash map).
  offsets     : odd k, kappa = kx + k ky + k^2 kz (x fastest), offset (k_axis - k // 2) * step per axis.
  map         : M[u, kappa] = the input row at out[u] + offset(kappa) of the same item, or -1.  Stride 1: in = out, step = ts.  Stride 2:
                in = fine, out = coarse, step = ts_fine.  Transposed: in = coarse, out = fine, step = -ts_fine (the strided map with in and out
                swapped: v = u + offset(kappa) ts_fine).
  convolution : y[u] = sum over kappa ascending, over the rows that exist, of x[M[u, kappa]] @ W[kappa]; W [K, Cin, Cout]."""
import numpy as np

CHANNELS = (None, 32, 64, 128, 256)
TR_CHANNELS = (None, 64, 64, 64, 128)
BN_EPS = 1e-5


def offsets(k):
    """-> int64 [k^3, 3] (x, y, z) in units of the step, row kappa = kx + k ky + k^2 kz."""
    assert k % 2 == 1 and k >= 1
    out = np.empty((k ** 3, 3), np.int64)
    for kap in range(k ** 3):
        out[kap] = (kap % k - k // 2, kap // k % k - k // 2, kap // (k * k) - k // 2)
    return out


def stride_map(coords, ts):
    """coords int [n,4] at tensor stride ts -> (coarse int32 [m,4] at 2 ts, parent int32 [n])."""
    coords = np.asarray(coords, np.int64)
    number, coarse, parent = {}, [], np.empty(coords.shape[0], np.int32)
    for i, (b, x, y, z) in enumerate(coords.tolist()):
        key = (b, x // (2 * ts) * (2 * ts), y // (2 * ts) * (2 * ts), z // (2 * ts) * (2 * ts))          # python's // is a floor
        if key not in number:
            number[key] = len(coarse)
            coarse.append(key)
        parent[i] = number[key]
    return np.asarray(coarse, np.int32).reshape(-1, 4), parent


def item_cuts(coords):
    """Segment starts [B+1] of the items 0..B-1 (contiguous, ascending); asserts that they are."""
    items = np.asarray(coords)[:, 0]
    assert items.size and (np.diff(items) >= 0).all() and items[0] >= 0
    B = int(items[-1]) + 1
    return np.searchsorted(items, np.arange(B + 1)).astype(np.int32)


def kernel_map(coords_in, coords_out, k, step):
    """-> int32 [n_out, k^3]: the input row at out + offset(kappa) * step of the same item, -1 where there is none."""
    row = {tuple(c): i for i, c in enumerate(np.asarray(coords_in, np.int64).tolist())}
    off = offsets(k) * step
    out = np.asarray(coords_out, np.int64)
    M = np.full((out.shape[0], k ** 3), -1, np.int32)
    for u, (b, x, y, z) in enumerate(out.tolist()):
        for kap in range(k ** 3):
            M[u, kap] = row.get((b, x + off[kap, 0], y + off[kap, 1], z + off[kap, 2]), -1)
    return M


def transposed_map(coords_coarse, coords_fine, ts_fine, k=3):
    return kernel_map(coords_coarse, coords_fine, k, -ts_fine)


def as_kernel(W):
    """[K,Cin,Cout], or [Cin,Cout] for kernel size 1 -> [K,Cin,Cout]."""
    W = np.asarray(W)
    return W[None] if W.ndim == 2 else W


def conv(x, W, M, dtype=np.float64):
    """y [n_out, Cout]: kappa ascending, a missing neighbour is a term left out."""
    W = as_kernel(W).astype(dtype)
    x = np.asarray(x).astype(dtype)
    y = np.zeros((M.shape[0], W.shape[2]), dtype)
    for kap in range(W.shape[0]):
        has = M[:, kap] >= 0
        if has.any():
            y[has] += x[M[has, kap]] @ W[kap]
    return y


def conv_bound(x, W, M):
    """-> (S [n_out,Cout] = sum |x| |w| in float64, terms int [n_out]): the scale and the length of every output element's sum."""
    S = conv(np.abs(np.asarray(x, np.float64)), np.abs(as_kernel(W).astype(np.float64)), M)
    return S, (M >= 0).sum(1) * as_kernel(W).shape[1]


def gamma(m):
    """Standard bound of float32 summation of m terms in any order: m u / (1 - m u), u = 2^-24."""
    u = 2.0 ** -24
    return m * u / (1.0 - m * u)


def state_dict_spec(in_channels=1, out_channels=32, conv1_kernel_size=5, channels=None, tr_channels=None, k1_flat=False):
    """name -> shape of every parameter and buffer of ResUNetBN2C under MinkowskiEngine's names, in module order."""
    C, T = channels or CHANNELS, tr_channels or TR_CHANNELS
    spec = {}

    def bn(name, c):
        spec[f'{name}.bn.weight'] = (c,); spec[f'{name}.bn.bias'] = (c,)
        spec[f'{name}.bn.running_mean'] = (c,); spec[f'{name}.bn.running_var'] = (c,); spec[f'{name}.bn.num_batches_tracked'] = ()

    def block(name, c):
        spec[f'{name}.conv1.kernel'] = (27, c, c); bn(f'{name}.norm1', c)
        spec[f'{name}.conv2.kernel'] = (27, c, c); bn(f'{name}.norm2', c)

    spec['conv1.kernel'] = (conv1_kernel_size ** 3, in_channels, C[1]); bn('norm1', C[1]); block('block1', C[1])
    for l in (2, 3, 4):
        spec[f'conv{l}.kernel'] = (27, C[l - 1], C[l]); bn(f'norm{l}', C[l]); block(f'block{l}', C[l])
    cin = C[4]
    for l in (4, 3, 2):
        spec[f'conv{l}_tr.kernel'] = (27, cin, T[l]); bn(f'norm{l}_tr', T[l]); block(f'block{l}_tr', T[l])
        cin = T[l] + C[l - 1]
    spec['conv1_tr.kernel'] = (cin, T[1]) if k1_flat else (1, cin, T[1])
    spec['final.kernel'] = (T[1], out_channels) if k1_flat else (1, T[1], out_channels)
    spec['final.bias'] = (1, out_channels)
    return spec


def random_state_dict(seed, **kw):
    """Weights of a plausible scale (fan-in normalised kernels, non-trivial BatchNorm statistics) for `state_dict_spec(**kw)`."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in state_dict_spec(**kw).items():
        if name.endswith('num_batches_tracked'):
            sd[name] = np.asarray(100, np.int64)
        elif name.endswith('running_var'):
            sd[name] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif name.endswith('bn.weight'):
            sd[name] = rng.uniform(0.7, 1.3, shape).astype(np.float32)
        elif name.endswith('kernel'):
            fan = shape[-2] * (shape[0] if len(shape) == 3 else 1)
            sd[name] = (rng.standard_normal(shape) * np.sqrt(2.0 / min(fan, 8 * shape[-2]))).astype(np.float32)
        else:
            sd[name] = (rng.standard_normal(shape) * 0.2).astype(np.float32)
    return sd


class ResUNetBN2C:
    """The network in eval mode on a state dict of numpy arrays; forward(coords int [m,4]) -> features [m, out_channels] in `dtype`."""

    def __init__(self, state_dict, normalize_feature=True, conv1_kernel_size=5, dtype=np.float64):
        self.sd = {k: np.asarray(v) for k, v in state_dict.items()}
        self.normalize_feature, self.k1, self.dtype = normalize_feature, conv1_kernel_size, dtype

    def levels(self, coords):
        """-> ([C1..C4] coordinates at tensor strides 1, 2, 4, 8, [parent of every row of C1..C3])."""
        C, parents = [np.asarray(coords, np.int32)], []
        for l in range(3):
            coarse, parent = stride_map(C[-1], 1 << l)
            C.append(coarse); parents.append(parent)
        return C, parents

    def _bn(self, y, name):
        t = self.dtype
        g, b = self.sd[f'{name}.bn.weight'].astype(t), self.sd[f'{name}.bn.bias'].astype(t)
        m, v = self.sd[f'{name}.bn.running_mean'].astype(t), self.sd[f'{name}.bn.running_var'].astype(t)
        return (y - m) / np.sqrt(v + t(BN_EPS)) * g + b

    def _block(self, x, name, M):
        h = np.maximum(self._bn(conv(x, self.sd[f'{name}.conv1.kernel'], M, self.dtype), f'{name}.norm1'), 0)
        return np.maximum(self._bn(conv(h, self.sd[f'{name}.conv2.kernel'], M, self.dtype), f'{name}.norm2') + x, 0)

    def maps(self, coords):
        """Every kernel map of the network for these coordinates (integers only: one set serves every dtype)."""
        C, _ = self.levels(coords)
        return {'n': C[0].shape[0], 'conv1': kernel_map(C[0], C[0], self.k1, 1), 'same': [kernel_map(C[l], C[l], 3, 1 << l) for l in range(4)],
                'down': {l: kernel_map(C[l - 2], C[l - 1], 3, 1 << (l - 2)) for l in (2, 3, 4)},
                'up': {l: transposed_map(C[l - 1], C[l - 2], 1 << (l - 2)) for l in (4, 3, 2)}}

    def forward(self, coords, maps=None):
        t = self.dtype
        M = maps or self.maps(coords)
        same = M['same']
        x = np.ones((M['n'], self.sd['conv1.kernel'].shape[1]), t)
        skip = []
        out = self._block(self._bn(conv(x, self.sd['conv1.kernel'], M['conv1'], t), 'norm1'), 'block1', same[0])
        skip.append(out)
        for l in (2, 3, 4):
            out = self._block(self._bn(conv(out, self.sd[f'conv{l}.kernel'], M['down'][l], t), f'norm{l}'), f'block{l}', same[l - 1])
            skip.append(out)
        for l in (4, 3, 2):
            out = self._block(self._bn(conv(out, self.sd[f'conv{l}_tr.kernel'], M['up'][l], t), f'norm{l}_tr'), f'block{l}_tr', same[l - 2])
            out = np.concatenate([out, skip[l - 2]], 1)
        ident = np.arange(M['n'], dtype=np.int32)[:, None]
        out = np.maximum(conv(out, self.sd['conv1_tr.kernel'], ident, t), 0)
        out = conv(out, self.sd['final.kernel'], ident, t) + self.sd['final.bias'].astype(t).reshape(1, -1)
        if self.normalize_feature:
            out = out / np.sqrt((out * out).sum(1, keepdims=True, dtype=t))
        return out
