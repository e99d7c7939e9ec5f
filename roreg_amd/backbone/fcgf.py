"""The FCGF backbone on the device: ResUNetBN2C (reference: backbone/fcgf/resunet.py on MinkowskiEngine) composed from the sparse-convolution
kernels of csrc/sparse_conv.hip (include/roreg_hip.h "v6j"; tests/_sparse_conv_oracle.py is the definition in numpy).

    model = ResUNetBN2C(1, 32, normalize_feature=True, conv1_kernel_size=5)
    model.load_state_dict(torch.load(ckpt)['state_dict'], strict=True)         # parameter and buffer names are MinkowskiEngine's
    feats = model.cuda().eval()(coords, item_cuts)                              # coords int32 [m,4] (item, x, y, z), item_cuts [items + 1]

Inference only (eval-mode BatchNorm, folded once to scale and shift).  The input feature is ones [m, in_channels], as testset.py feeds it.
Every sum is a float32 fmaf chain of a fixed order: an item's features do not depend on the items it is batched with.  Coarse rows are
numbered in ascending order of their lowest fine row (this project's rule; nothing downstream of the network depends on it).
Limits (the 63-bit key of the maps): items < 2^15, voxel coordinates in [-2^15, 2^15); outside them a HipError, never an alias."""
import numpy as np
import torch
from torch import nn

from .. import hip

CHANNELS = (None, 32, 64, 128, 256)
TR_CHANNELS = (None, 64, 64, 64, 128)
BN_EPS = 1e-5


class SparseConvolution(nn.Module):
    """Holds MinkowskiConvolution's parameters: kernel [K, Cin, Cout] (a checkpoint's [Cin, Cout] for kernel size 1 loads too), bias [1, Cout]."""

    def __init__(self, cin, cout, kernel_size, bias=False):
        super().__init__()
        self.kernel_size = int(kernel_size)
        self.kernel = nn.Parameter(torch.zeros(self.kernel_size ** 3, cin, cout))
        self.bias = nn.Parameter(torch.zeros(1, cout)) if bias else None

    def _load_from_state_dict(self, state_dict, prefix, *args):
        k = state_dict.get(prefix + 'kernel')
        if k is not None and k.dim() == 2 and self.kernel.shape[0] == 1:
            state_dict[prefix + 'kernel'] = k[None]
        super()._load_from_state_dict(state_dict, prefix, *args)


class BatchNorm(nn.Module):
    """MinkowskiBatchNorm's layout: the statistics live in `.bn`."""

    def __init__(self, c, momentum=0.1):
        super().__init__()
        self.bn = nn.BatchNorm1d(c, eps=BN_EPS, momentum=momentum)

    def folded(self):
        """-> (scale, shift) float32 [C]: gamma / sqrt(var + eps) and beta - mean scale, computed in float64 and rounded once."""
        bn = self.bn
        scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        return scale.float().contiguous(), (bn.bias.double() - bn.running_mean.double() * scale).float().contiguous()


class BasicBlockBN(nn.Module):
    def __init__(self, c, momentum=0.1):
        super().__init__()
        self.conv1 = SparseConvolution(c, c, 3); self.norm1 = BatchNorm(c, momentum)
        self.conv2 = SparseConvolution(c, c, 3); self.norm2 = BatchNorm(c, momentum)


class ResUNetBN2C(nn.Module):
    CHANNELS = CHANNELS
    TR_CHANNELS = TR_CHANNELS

    def __init__(self, in_channels=1, out_channels=32, normalize_feature=True, conv1_kernel_size=5, channels=None, tr_channels=None, bn_momentum=0.1, D=3):
        super().__init__()
        if D != 3 or conv1_kernel_size not in (1, 3, 5, 7):
            raise ValueError(f'ResUNetBN2C: D = 3 and an odd conv1_kernel_size up to 7, got D = {D}, conv1_kernel_size = {conv1_kernel_size}')
        C, T = tuple(channels or self.CHANNELS), tuple(tr_channels or self.TR_CHANNELS)
        self.channels, self.tr_channels, self.in_channels = C, T, int(in_channels)
        self.normalize_feature, self.conv1_kernel_size = bool(normalize_feature), int(conv1_kernel_size)
        self.conv1 = SparseConvolution(in_channels, C[1], conv1_kernel_size); self.norm1 = BatchNorm(C[1], bn_momentum); self.block1 = BasicBlockBN(C[1], bn_momentum)
        for l in (2, 3, 4):
            setattr(self, f'conv{l}', SparseConvolution(C[l - 1], C[l], 3)); setattr(self, f'norm{l}', BatchNorm(C[l], bn_momentum))
            setattr(self, f'block{l}', BasicBlockBN(C[l], bn_momentum))
        cin = C[4]
        for l in (4, 3, 2):
            setattr(self, f'conv{l}_tr', SparseConvolution(cin, T[l], 3)); setattr(self, f'norm{l}_tr', BatchNorm(T[l], bn_momentum))
            setattr(self, f'block{l}_tr', BasicBlockBN(T[l], bn_momentum))
            cin = T[l] + C[l - 1]
        self.conv1_tr = SparseConvolution(cin, T[1], 1)
        self.final = SparseConvolution(T[1], out_channels, 1, bias=True)
        self._folded = None

    # the folded BatchNorm constants are derived from the parameters once; whatever replaces or moves the parameters drops them
    def load_state_dict(self, *args, **kw):
        self._folded = None
        return super().load_state_dict(*args, **kw)

    def _apply(self, fn, *args, **kw):
        self._folded = None
        return super()._apply(fn, *args, **kw)

    def _fold(self):
        if self._folded is None:
            with torch.no_grad():
                self._folded = {name: m.folded() for name, m in self.named_modules() if isinstance(m, BatchNorm)}
        return self._folded

    def _block(self, x, name, M, out):
        blk, F = getattr(self, name), self._fold()
        h = hip.sparse_conv(x, blk.conv1.kernel, M, *F[f'{name}.norm1'], relu=True)
        return hip.sparse_conv(h, blk.conv2.kernel, M, *F[f'{name}.norm2'], residual=x, relu=True, out=out)

    @torch.no_grad()
    def forward(self, coords, item_cuts):
        """coords int32 [m,4] rows (item, x, y, z) at tensor stride 1, unique, items contiguous and ascending; item_cuts [items + 1] their
        segment starts -> float32 [m, out_channels] on the device."""
        if self.training:
            raise hip.HipError('ResUNetBN2C: inference only (call .eval()); BatchNorm is evaluated from its running statistics')
        dev = self.conv1.kernel.device
        coords = torch.as_tensor(coords, dtype=torch.int32).to(dev).contiguous()
        cuts = torch.as_tensor(np.asarray(item_cuts.cpu() if torch.is_tensor(item_cuts) else item_cuts), dtype=torch.int32).to(dev).contiguous()
        C, T, F = self.channels, self.tr_channels, self._fold()
        lv, lc = [coords], [cuts]
        for l in range(3):
            sm = hip.sparse_stride_map(lv[-1], lc[-1], 1 << l)
            lv.append(sm.coords); lc.append(sm.cuts)
        m = [int(c.shape[0]) for c in lv]
        same = [hip.sparse_kernel_map(lv[l], lv[l], 3, 1 << l) for l in range(4)]
        # the three concatenations [decoder, encoder] are column windows of one buffer per level: both producers write in place
        cat = {l: torch.empty((m[l - 1], T[l + 1] + C[l]), dtype=torch.float32, device=dev) for l in (1, 2, 3)}
        x = torch.ones((m[0], self.in_channels), dtype=torch.float32, device=dev)
        M1 = same[0] if self.conv1_kernel_size == 3 else hip.sparse_kernel_map(lv[0], lv[0], self.conv1_kernel_size, 1)
        t = hip.sparse_conv(x, self.conv1.kernel, M1, *F['norm1'])
        del M1
        out = self._block(t, 'block1', same[0], cat[1][:, T[2]:])
        for l in (2, 3, 4):
            down = hip.sparse_kernel_map(lv[l - 2], lv[l - 1], 3, 1 << (l - 2))
            t = hip.sparse_conv(out, getattr(self, f'conv{l}').kernel, down, *F[f'norm{l}'])
            out = self._block(t, f'block{l}', same[l - 1], cat[l][:, T[l + 1]:] if l < 4 else None)
        for l in (4, 3, 2):
            up = hip.sparse_kernel_map(lv[l - 1], lv[l - 2], 3, -(1 << (l - 2)))
            t = hip.sparse_conv(out, getattr(self, f'conv{l}_tr').kernel, up, *F[f'norm{l}_tr'])
            self._block(t, f'block{l}_tr', same[l - 2], cat[l - 1][:, :T[l]])
            out = cat[l - 1]
        ident = torch.arange(m[0], dtype=torch.int32, device=dev)[:, None].contiguous()
        out = hip.sparse_conv(out, self.conv1_tr.kernel, ident, relu=True)
        out = hip.sparse_conv(out, self.final.kernel, ident, shift=self.final.bias.reshape(-1))
        return hip.sparse_l2norm(out) if self.normalize_feature else out


MODELS = {'ResUNetBN2C': ResUNetBN2C}


def load_model(name):
    """The model class of that name, or None (the reference's backbone.fcgf.load_model; ResUNetBN2C is the variant its checkpoints use)."""
    return MODELS.get(name)


def from_checkpoint(path, device='cuda'):
    """A reference checkpoint ({'config': ..., 'state_dict': ...}, as testset.py reads it) -> the model on the device in eval mode."""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    cfg = ck['config']
    get = cfg.get if isinstance(cfg, dict) else lambda k, d=None: getattr(cfg, k, d)
    Model = load_model(get('model', 'ResUNetBN2C'))
    if Model is None:
        raise ValueError(f"{path}: model {get('model')!r} is not one of {sorted(MODELS)}")
    model = Model(1, get('model_n_out', 32), bn_momentum=0.05, normalize_feature=get('normalize_feature', True), conv1_kernel_size=get('conv1_kernel_size', 5), D=3)
    model.load_state_dict(ck['state_dict'], strict=True)
    return model.to(device).eval()
