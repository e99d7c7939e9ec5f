"""Record what the split-product kernels outside the irrep GEMM family return, bit for bit: the group convolutions and the dense layer
(csrc/group_conv.hip), the group Fourier transforms (ft_nonlin_kernel, csrc/fourier.hip) and the mutual matcher (csrc/mfma_match.hip), so
that a restructuring of what they share -- the split product, the accumulator row map, the host launch -- can be shown to change nothing.

    python tools/record_conv_bits.py [--out tests/golden/conv_parent_bits.npz]

The companion of tools/record_gemm_bits.py (same fixture format, same refusal outside a clean checkout): one sha1 digest per returned
tensor and the hash of the commit whose kernels produced them.  Operands come from seeded numpy generators; the packed convolution's input
words are made on the host with the host split rule (_f16_split2) and hip.bound_exp, so no other kernel stands between the seed and the
operand.  tests/test_hip_fourier.py::test_refactor_keeps_the_parents_conv_bits recomputes run_cases() and compares every digest.

The case set (the smallest shapes at which the shared pieces can go wrong):
  group_conv_split_kernel   Cin 16 (a single chunk: the look-ahead never fires) and 48; Cout 256 and 512; (Lin, Lout) = (48, 13) with 45 live
                            columns; B = 1 (nkp_max clamps to B), 10 (130 columns: a second tile with 2) and 37 (keypoints straddle tile
                            edges); bf16 x 3, fp16 x 2 (with the output row maximum) and the packed-word form; with and without BatchNorm;
                            with and without an lds_order at stride 53
  dense_split_kernel        (B, K, O) = (1, 16, 4), (130, 128, 4), (128, 32, 256) (with a residual: the interior-tile path), (77, 256, 512);
                            both splits; with and without scale / shift; no residual, residual stride 1 and 13
  group_conv_kernel         one case per branch of dispatch() (the split-K shape KS 13, Lout 1 among them), Cin 32, B 3, with and without residual
  ft_nonlin_kernel          forward, inverse and inverse to the group domain, bf16 x 3 and fp16 x 2, C 32, B = 32 (one column tile) and 36
  mutual matcher            the default form on the task list of test_mutual_match_batch_equals_oracle_and_per_pair_calls plus one pair smaller
                            than a tile: every task's pairs and the counts
(The matcher's env-selected forms need a process of their own: tests/test_hip_kernels.py pins them to the default form.)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from record_gemm_bits import _digest, clean_commit, load, save           # noqa: E402,F401  (load: for the test)

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'conv_parent_bits.npz')
LIN, LOUT, LIVE = 48, 13, 45
CONV_B = (1, 10, 37)
DENSE = [(1, 16, 4), (130, 128, 4), (128, 32, 256), (77, 256, 512)]
# (KS, Lin, Lout, Cout): one per branch of csrc/group_conv.hip's dispatch(), in its order
F32_CONV = [(13, 60, 60, 128), (13, 60, 60, 64), (13, 60, 60, 32), (13, 48, 13, 256), (13, 48, 13, 128), (13, 48, 13, 32), (13, 45, 13, 128), (13, 45, 13, 32),
            (13, 13, 1, 256), (13, 13, 1, 32), (1, 1, 1, 128), (1, 1, 1, 32)]


def _conv_cases(out):
    import torch

    from roreg_amd import hip
    from roreg_amd._hip_fourier import _f16_split2
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(4813)
    gather = np.stack([rng.permutation(LIVE)[:13] for _ in range(LOUT)]).astype(np.int32)
    order = np.full(LIN, -1, np.int32); order[:LIVE] = rng.permutation(53)[:LIVE]
    gd = cu(gather)
    orders = {'order0': None, 'order53': (cu(order), 53)}
    for Cin in (16, 48):
        for Cout in (256, 512):
            rng = np.random.default_rng(100 * Cin + Cout)
            W = (rng.standard_normal((Cout, Cin, 1, 13)) / np.sqrt(13 * Cin)).astype(np.float32); bias = rng.standard_normal(Cout).astype(np.float32)
            bn = [rng.uniform(0.5, 1.5, Cin), 0.1 * rng.standard_normal(Cin), 0.1 * rng.standard_normal(Cin), rng.uniform(0.5, 1.5, Cin)]
            layers = {'bn0': hip.ConvLayer(torch.from_numpy(W), torch.from_numpy(bias)),
                      'bn1': hip.ConvLayer(torch.from_numpy(W), torch.from_numpy(bias), [torch.from_numpy(t.astype(np.float32)) for t in bn])}
            for B in CONV_B:
                x = (rng.standard_normal((B, Cin, LIN)) * np.exp(rng.standard_normal((B, Cin, 1)))).astype(np.float32)
                x[:, :, LIVE:] = 0
                xd = cu(x); rmax = cu(np.abs(x).max((1, 2)))
                # the packed form's operand: ReLU(x) under the block scale of its own row maximum, split on the host
                a = np.maximum(x, 0.0)
                bound = torch.from_numpy(a.max((1, 2)))
                e = hip.bound_exp(bound).numpy().astype(np.int32)
                hi, lo = _f16_split2(a, e[:, None, None])
                words = cu((hi.astype(np.uint32) | (lo.astype(np.uint32) << 16)).view(np.int32)); bd = bound.cuda()
                for on, od in orders.items():
                    key = f'conv/{Cin}x{Cout}/B{B}/{on}'
                    for bname, layer in layers.items():
                        out[f'{key}/{bname}/bf16x3'] = _digest(hip.group_conv(xd, layer, gather=gd, split=True, lds_order=od))
                        y, m = hip.group_conv(xd, layer, gather=gd, in_rowmax=rmax, want_rowmax=True, lds_order=od)
                        out[f'{key}/{bname}/f16x2'], out[f'{key}/{bname}/f16x2/rowmax'] = _digest(y), _digest(m)
                    y, m = hip.group_conv_packed(words, layers['bn0'], bd, gd, want_rowmax=True, lds_order=od)
                    out[f'{key}/packed'], out[f'{key}/packed/rowmax'] = _digest(y), _digest(m)


def _dense_cases(out):
    import torch

    from roreg_amd import hip
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for B, K, Oc in DENSE:
        rng = np.random.default_rng(10000 * B + 10 * K + Oc)
        W = (rng.standard_normal((Oc, K)) / np.sqrt(K)).astype(np.float32); bias = rng.standard_normal(Oc).astype(np.float32)
        sc = rng.uniform(0.5, 1.5, K).astype(np.float32); sh = rng.standard_normal(K).astype(np.float32)
        x = (rng.standard_normal((B, K)) * np.exp(rng.standard_normal((B, 1)))).astype(np.float32)
        res = {'res0': (None, 1), 'res1': (cu(rng.standard_normal((B, Oc)).astype(np.float32)), 1), 'res13': (cu(rng.standard_normal((B, Oc, 13)).astype(np.float32)), 13)}
        xd = cu(x); rmax = cu(np.abs(x).max(1))
        for aname, layer in (('act0', hip.DenseSplitLayer(W, bias)), ('act1', hip.DenseSplitLayer(W, bias, sc, sh))):
            for rname, (r, stride) in res.items():
                key = f'dense/{B}x{K}x{Oc}/{aname}/{rname}'
                out[f'{key}/bf16x3'] = _digest(hip.dense_split(xd, layer, residual=r, residual_stride=stride))
                y, m = hip.dense_split(xd, layer, residual=r, in_rowmax=rmax, want_rowmax=True, residual_stride=stride)
                out[f'{key}/f16x2'], out[f'{key}/f16x2/rowmax'] = _digest(y), _digest(m)


def _f32_conv_cases(out):
    import torch

    from roreg_amd import hip
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    B, Cin = 3, 32
    for KS, Lin, Lout, Cout in F32_CONV:
        rng = np.random.default_rng(1000 * Lin + Cout)
        W = (rng.standard_normal((Cout, Cin, 1, KS)) / np.sqrt(KS * Cin)).astype(np.float32); bias = rng.standard_normal(Cout).astype(np.float32)
        bn = [rng.uniform(0.5, 1.5, Cin), 0.1 * rng.standard_normal(Cin), 0.1 * rng.standard_normal(Cin), rng.uniform(0.5, 1.5, Cin)]
        layer = hip.ConvLayer(torch.from_numpy(W), torch.from_numpy(bias), [torch.from_numpy(t.astype(np.float32)) for t in bn])
        live = min(Lin, LIVE)
        gather = None if Lin == 60 else cu(np.stack([rng.permutation(live)[:KS] for _ in range(Lout)]).astype(np.int32))
        x = cu(rng.standard_normal((B, Cin, Lin)).astype(np.float32)); r = cu(rng.standard_normal((B, Cout, Lout)).astype(np.float32))
        for rname, res in (('res0', None), ('res1', r)):
            out[f'conv32/KS{KS}/L{Lin}-{Lout}/O{Cout}/{rname}'] = _digest(hip.group_conv(x, layer, gather=gather, residual=res))


def _ft_cases(out):
    import torch

    from roreg_amd import hip
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    C = 32

    def coefs(t, B):
        """the columns of the B real keypoints of a coefficient buffer (the pad keypoints' are not part of the contract)"""
        Bp = hip.coef_pitch(B)
        return torch.cat([v[:, hip._keypoint_of_columns(d, Bp) < B].reshape(-1) for d, v in zip((1, 3, 3, 4, 5), hip.coef_views(t, C, B))])

    for B in (32, 36):
        rng = np.random.default_rng(600 + B)
        Bp = hip.coef_pitch(B)
        x = (rng.standard_normal((B, C, 60)) * np.exp(rng.standard_normal((B, 1, 1)))).astype(np.float32)
        X = rng.standard_normal(hip.coef_size(C, B)).astype(np.float32)
        bias = cu(rng.standard_normal(C).astype(np.float32))
        bn = (cu(rng.uniform(0.5, 1.5, C).astype(np.float32)), cu(rng.standard_normal(C).astype(np.float32)))
        gmap = np.full(60, -1, np.int32); gmap[rng.permutation(60)[:LIVE]] = np.arange(LIVE)
        xb = np.zeros(Bp, np.float32); xb[:B] = 8.0 * np.abs(x).max((1, 2))                     # sqrt(60) max |x[b]| bounds every coefficient of FT(x[b])
        yb = np.zeros(Bp, np.float32); yb[:B] = 64.0 * (1.5 * (8.0 * np.abs(X).max() + 4.0) + 4.0)   # 60 |scale| (sqrt(60) max |X| + |bias|) + sqrt(60) |shift|, rounded up
        xd, Xd, gm, xb, yb = cu(x), cu(X), cu(gmap), cu(xb), cu(yb)
        key = f'ft/B{B}'
        out[f'{key}/forward/bf16x3'] = _digest(coefs(hip.ft_nonlin(B, C, x_spatial=xd, split=True), B))
        out[f'{key}/forward/f16x2'] = _digest(coefs(hip.ft_nonlin(B, C, x_spatial=xd, split='f16x2', out_bound=xb), B))
        out[f'{key}/inverse/bf16x3'] = _digest(coefs(hip.ft_nonlin(B, C, coef_in=Xd, bias=bias, bn=bn, split=True), B))
        out[f'{key}/inverse/f16x2'] = _digest(coefs(hip.ft_nonlin(B, C, coef_in=Xd, bias=bias, bn=bn, split='f16x2', out_bound=yb), B))
        out[f'{key}/to_group/bf16x3'] = _digest(hip.ft_nonlin(B, C, coef_in=Xd, bias=bias, spatial_out=True, g_map=gm, Lout=LIN, Lvalid=LIVE, split=True)[:, :, :LIVE])
        z, m = hip.ft_nonlin(B, C, coef_in=Xd, bias=bias, spatial_out=True, g_map=gm, Lout=LIN, Lvalid=LIVE, split='f16x2', want_rowmax=True)
        out[f'{key}/to_group/f16x2'], out[f'{key}/to_group/f16x2/rowmax'] = _digest(z[:, :, :LIVE]), _digest(m)


def _match_cases(out):
    import torch

    from roreg_amd import hip
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rng = np.random.default_rng(11)

    def cloud(n):
        a = rng.standard_normal((n, 32)).astype(np.float32)
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    base = cloud(700)
    clouds = [base, (base[rng.permutation(700)[:613]] + 0.05 * rng.standard_normal((613, 32))).astype(np.float32), cloud(1), cloud(255),
              np.concatenate([base[:100], base[:100]]), cloud(20), cloud(17)]
    specs = [(0, 1, 'perm', 'perm'), (1, 0, None, 'perm'), (0, 4, 'perm', None), (2, 3, None, None), (3, 2, 'perm', None), (4, 4, None, None), (5, 6, None, None)]
    tasks = []
    for a, b, ra, rb in specs:
        A, B = clouds[a], clouds[b]
        r0 = rng.permutation(A.shape[0])[:max(1, A.shape[0] - 3)] if ra else None
        r1 = rng.permutation(B.shape[0])[:max(1, B.shape[0] - 2)] if rb else None
        tasks.append((cu(A), cu(B), cu(r0) if r0 is not None else None, cu(r1) if r1 is not None else None))
    mbuf, cnt = hip.mutual_match_batch(tasks)
    out['match/counts'] = _digest(cnt)
    for q, c in enumerate(cnt.cpu().numpy()):
        out[f'match/task{q}'] = _digest(mbuf[q, :c])                       # (rows past the count are not written)


def run_cases():
    """-> {name: sha1 hex digest} from the library roreg_amd.hip loads"""
    from roreg_amd import hip
    hip.ensure_tables()
    out = {}
    for cases in (_conv_cases, _dense_cases, _f32_conv_cases, _ft_cases, _match_cases):
        cases(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=FIXTURE)
    a = ap.parse_args()
    commit = clean_commit('record_conv_bits')
    digests = run_cases()
    save(a.out, commit, digests)
    print(f'{a.out}: {len(digests)} digests, {os.path.getsize(a.out)} bytes; commit {commit}')


if __name__ == '__main__':
    main()
