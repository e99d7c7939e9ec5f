"""HIP kernels (through the C-ABI) against the oracle on identical inputs.  GPU only (-m gpu).
Bar: bit-exact for indices / masks; stated tolerance for floating-point network outputs."""
import numpy as np
import pytest
import torch

from conftest import load_golden, canon_knn, same_knn_up_to_duplicates
from oracle import ref_numpy as O
from roreg_amd import synth

pytestmark = pytest.mark.gpu


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def seeded_net(kind, seed):
    from roreg_amd.network import name2network
    from roreg_amd.parses.parses_test import default_config
    net = name2network[kind](default_config())
    sd = synth.seeded_state_dict(net, seed)
    return net, {k: v.numpy() for k, v in sd.items()}


# ---- group convolution ------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,Cin,Cout,bn,res', [(7, 32, 256, False, False), (9, 256, 512, True, False), (5, 512, 256, True, True),
                                                (11, 256, 32, True, True), (13, 32, 64, True, False), (6, 64, 16, True, True),
                                                (1, 128, 256, True, False), (70, 32, 16, True, False)])
def test_group_conv_full(group, B, Cin, Cout, bn, res):
    from roreg_amd import hip
    rng = np.random.default_rng(B * 1000 + Cin + Cout)
    x = rng.standard_normal((B, Cin, 60)).astype(np.float32)
    W = (rng.standard_normal((Cout, Cin, 1, 13)) / np.sqrt(Cin * 13)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    sd = {'c.2.weight': W, 'c.2.bias': b}
    bnp = None
    if bn:
        sd.update({'c.0.weight': rng.uniform(0.5, 1.5, Cin).astype(np.float32), 'c.0.bias': rng.normal(0, .1, Cin).astype(np.float32),
                   'c.0.running_mean': rng.normal(0, .1, Cin).astype(np.float32), 'c.0.running_var': rng.uniform(.5, 1.5, Cin).astype(np.float32)})
        want = O.comb_conv(x, sd, 'c', group.Nei)
        bnp = tuple(torch.from_numpy(sd[f'c.0.{k}']) for k in ['weight', 'bias', 'running_mean', 'running_var'])
    else:
        want = O.group_conv(x, W, b, group.Nei)
    r = rng.standard_normal((B, Cout, 60)).astype(np.float32) if res else None
    if res:
        want = want + r
    layer = hip.ConvLayer(torch.from_numpy(W), torch.from_numpy(b), bnp)
    got = hip.group_conv(cu(x), layer, residual=cu(r) if res else None).cpu().numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 2e-5 * max(1.0, np.abs(want).max())


def test_group_conv_transpose_detecting(group):
    """A = identity-like weights with an asymmetric activation pattern: catches a swapped C/D mapping."""
    from roreg_amd import hip
    Cin = Cout = 32
    W = np.zeros((Cout, Cin, 1, 13), np.float32)
    for o in range(Cout):
        W[o, (o * 7 + 3) % Cin, 0, o % 13] = 1.0 + o
    x = np.arange(3 * Cin * 60, dtype=np.float32).reshape(3, Cin, 60) / 100.0
    want = O.group_conv(x, W, np.zeros(Cout, np.float32), group.Nei)
    layer = hip.ConvLayer(torch.from_numpy(W), torch.zeros(Cout), None)
    got = hip.group_conv(cu(x), layer).cpu().numpy()
    assert np.array_equal(got, want)


def test_gf_forward_vs_oracle_and_golden(group):
    z = load_golden('gf_forward')
    net, sd = seeded_net('GF_test', int(z['seed']))
    out = net(torch.from_numpy(z['x']))
    eqv = out['eqv'].cpu().numpy(); inv = out['inv'].cpu().numpy()
    want = O.gf_forward(z['x'], sd, group.Nei)
    assert np.abs(eqv - want['eqv']).max() < 1e-5 and np.abs(inv - want['inv']).max() < 1e-5
    assert np.abs(eqv - z['eqv']).max() < 1e-5 and np.abs(inv - z['inv']).max() < 1e-5


def test_gf_equivariance_on_device(group):
    net, _ = seeded_net('GF_test', 5)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((130, 32, 60)).astype(np.float32)
    a = 41
    y0 = net(torch.from_numpy(x))['eqv'].cpu().numpy()
    y1 = net(torch.from_numpy(np.ascontiguousarray(x[:, :, group.P[a]])))['eqv'].cpu().numpy()
    assert np.abs(y1 - y0[:, :, group.P[a]]).max() < 1e-5


def test_rd_forward_vs_golden(group):
    from roreg_amd.network import name2network
    from roreg_amd.parses.parses_test import default_config
    z = load_golden('rd_forward')
    net = name2network['RD_test'](default_config())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in load_golden('weights_RD').items()}, strict=True)
    enc = net.encode(torch.from_numpy(z['x'])).cpu().numpy()                    # irrep-domain evaluation (default)
    assert np.abs(enc - z['enc']).max() < 1e-4 * max(1.0, np.abs(z['enc']).max())
    net.mode = 'direct'
    enc_d = net.encode(torch.from_numpy(z['x'])).cpu().numpy()                  # 13-stencil kernels
    net.mode = 'fourier'
    assert np.abs(enc_d - z['enc']).max() < 1e-4 * max(1.0, np.abs(z['enc']).max())
    assert np.abs(enc - enc_d).max() < 2e-5 * max(1.0, np.abs(z['enc']).max())
    for mode in ('bf16x3', 'f32'):
        net._fourier.gemm = mode
        e2 = net.encode(torch.from_numpy(z['x'])).cpu().numpy()
        assert np.abs(e2 - z['enc']).max() < 1e-4 * max(1.0, np.abs(z['enc']).max())
    net._fourier.gemm = 'f16x2' 
    s = net({'feats': torch.from_numpy(z['x'])})['scores'].cpu().numpy()
    assert np.abs(s - z['scores']).max() < 1e-4
    from roreg_amd import hip
    s2 = hip.det_score(cu(z['enc'])).cpu().numpy()
    assert np.abs(s2 - z['scores']).max() < 5e-5


def test_et_forward_pruned_equals_full_equals_golden(group):
    z = load_golden('et_forward')
    net, sd = seeded_net('ET_test', int(z['seed']))
    batch = {k: torch.from_numpy(z[k].copy()) for k in ['before_eqv0', 'before_eqv1', 'after_eqv0', 'after_eqv1', 'pre_idx']}
    net.pruned = True
    qp = net(batch)['quaternion_pre'].cpu().numpy()
    net.pruned = False
    qf = net(batch)['quaternion_pre'].cpu().numpy()
    assert np.abs(qp - qf).max() < 2e-5
    assert np.abs(qp - z['quaternion']).max() < 1e-4
    want = O.et_forward({k: z[k] for k in ['before_eqv0', 'before_eqv1', 'after_eqv0', 'after_eqv1', 'pre_idx']}, sd, group.Nei, group.P)
    assert np.abs(qp - want).max() < 1e-4


# ---- bit-exact kernels --------------------------------------------------------------------------------------
def test_inv_descriptor_bit_exact():
    from roreg_amd import hip
    z = load_golden('pipeline_mutual_yohoo')
    for pc in ['0', '1']:
        want = O.inv_descriptor(z[f'yoho_{pc}'])
        got = hip.inv_descriptor(cu(z[f'yoho_{pc}'])).cpu().numpy()
        assert np.array_equal(got, want)


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'tie'])
def test_nn_search_bit_exact_golden(tag):
    from roreg_amd import hip
    z = load_golden('knn')
    idx, d = hip.nn_search(cu(z[f'{tag}_source']), cu(z[f'{tag}_target']), want_dist=True)
    od, oi = O.knn(z[f'{tag}_target'], z[f'{tag}_source'], 1)
    assert np.array_equal(idx.cpu().numpy(), oi)
    assert np.array_equal(d.cpu().numpy(), od)
    assert np.array_equal(idx.cpu().numpy(), z[f'{tag}_idx'].reshape(-1))


def test_nn_search_5000_with_row_lists():
    from roreg_amd import hip
    rng = np.random.default_rng(0)
    A = rng.standard_normal((5000, 32)).astype(np.float32); A /= np.linalg.norm(A, axis=1, keepdims=True)
    B = (A[rng.permutation(5000)] + 0.05 * rng.standard_normal((5000, 32))).astype(np.float32)
    ra = rng.permutation(5000)[:4000]; rb = rng.permutation(5000)[:3777]
    idx = hip.nn_search(cu(B), cu(A), src_rows=cu(rb), tgt_rows=cu(ra)).cpu().numpy()
    _, oi = O.knn(A[ra], B[rb], 1)
    assert np.array_equal(idx, oi)


def test_knn5_golden():
    from roreg_amd import hip
    z = load_golden('knn')
    idx = hip.knn_search(cu(z['k5_keys']), cu(z['k5_keys']), 5).cpu().numpy()
    assert np.array_equal(idx, z['k5_idx'][0].T)


def test_knn_matcher_public_methods_vs_reference_golden():
    """modified_knn_matcher's whole public surface (utils/knn_search.py:17-136) against the reference's own outputs: pdist, find_nn_gpu,
    find_knn_gpu, __call__ and find_corr, 'L2' and 'SquareL2', indices and distances bit for bit, shapes and devices as the reference
    returns them; an unknown dist_type raises NotImplementedError like the reference."""
    from roreg_amd.utils.knn_search import knn_module
    z = load_golden('knn_api')
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    M = knn_module.KNN(5)
    for dt in ('L2', 'SquareL2'):
        D = M.pdist(A[:40], B, dist_type=dt)
        assert D.device.type == 'cpu' and np.array_equal(D.numpy(), O.pdist(z['A'][:40], z['B'], dt))
        assert np.abs(D.numpy() - z[f'pdist_{dt}']).max() < 1e-6
        assert M.pdist(A[:40].cuda(), B.cuda(), dist_type=dt).is_cuda
        d, i = M.find_nn_gpu(A, B, nn_max_n=128, dist_type=dt)
        od, oi = O.knn(z['B'], z['A'], 1, dist_type=dt)
        assert d.shape == (301,) and i.dtype == torch.int64 and not i.is_cuda
        assert np.array_equal(i.numpy(), z[f'nn_i_{dt}']) and np.array_equal(d.numpy(), od) and np.abs(d.numpy() - z[f'nn_d_{dt}']).max() < 1e-6
        d, i = M.find_knn_gpu(A, B, nn_max_n=128, dist_type=dt)
        od, oi = O.knn(z['B'], z['A'], 5, dist_type=dt)
        assert d.shape == (301, 1, 5) and i.shape == (301, 5)
        rd, ri = canon_knn(z[f'knn_d_{dt}'][:, 0, :], z[f'knn_i_{dt}'])        # (exactly tied entries: torch.topk's order is unspecified, ours is by index)
        ok, n_dup = same_knn_up_to_duplicates(i.numpy(), ri, z['B'])            # (a tie at the k-th place: which duplicate is listed)
        assert ok and n_dup < 40 and np.array_equal(i.numpy(), oi) and np.array_equal(d.numpy()[:, 0], od)
        d, i2 = M(B.T[None], A.T[None], dist_type=dt)
        assert d.shape == (1, 5, 1, 301) and np.array_equal(i2.numpy()[0].T, i.numpy())
        assert np.abs(d.numpy()[0, :, 0, :].T - rd).max() < 1e-6
        d, i = knn_module.KNN(1)(B.T[None], A.T[None], dist_type=dt)
        assert np.array_equal(i.numpy(), z[f'call1_i_{dt}']) and np.abs(d.numpy() - z[f'call1_d_{dt}']).max() < 1e-6
    assert np.array_equal(M.find_nn_gpu(A, B, return_distance=False).numpy(), z['nn_i_only'])
    d, i = M.find_knn_gpu(torch.from_numpy(z['K']), torch.from_numpy(z['K']))
    assert np.array_equal(i.numpy(), z['knn3_i']) and np.abs(d.numpy() - z['knn3_d']).max() < 1e-6
    np.random.seed(77)
    i0, i1 = M.find_corr(A, B, subsample_size=256, mutual=True)
    assert np.array_equal(i0, z['corr_i0']) and np.array_equal(i1, z['corr_i1'])
    np.random.seed(78)
    i0, i1 = M.find_corr(A, B, subsample_size=-1, mutual=False)
    assert np.array_equal(i0, z['corr_nm_i0']) and np.array_equal(i1, z['corr_nm_i1'])
    with pytest.raises(NotImplementedError):
        M.pdist(A, B, dist_type='cosine')
    with pytest.raises(NotImplementedError):
        M(B.T[None], A.T[None], dist_type='L1')


def test_knn_matcher_other_widths_and_longer_lists_vs_reference_golden():
    """The reference's modified_knn_matcher takes any feature width and any k (utils/knn_search.py:13-162); the tuned kernels serve the pipeline's
    widths 3 / 32 with k <= 8 and everything else goes through the generic kernel (csrc/nn_search.hip, knn_generic_kernel; k <= 32).  F = 16
    with k = 12 and F = 7 with k = 1 against the reference's own outputs (tools/gen_golden.py knn_wide), both distance types: indices bit for
    bit (up to torch.topk's unspecified order among exactly tied duplicates), distances equal to the oracle's and within 1e-6 of the
    reference's; the tuned and the generic kernel agree bit for bit where both apply (F = 32, k = 5 vs the same call padded to k = 9)."""
    from roreg_amd import hip
    from roreg_amd.utils.knn_search import knn_module
    z = load_golden('knn_wide')
    A, B = torch.from_numpy(z['A']), torch.from_numpy(z['B'])
    M = knn_module.KNN(12)
    for dt in ('L2', 'SquareL2'):
        d, i = M.find_knn_gpu(A, B, nn_max_n=100, dist_type=dt)
        od, oi = O.knn(z['B'], z['A'], 12, dist_type=dt)
        assert d.shape == (257, 1, 12) and i.shape == (257, 12) and i.dtype == torch.int64
        rd, ri = canon_knn(z[f'knn_d_{dt}'][:, 0, :], z[f'knn_i_{dt}'])
        ok, n_dup = same_knn_up_to_duplicates(i.numpy(), ri, z['B'])
        assert ok and n_dup <= 80 and np.array_equal(i.numpy(), oi) and np.array_equal(d.numpy()[:, 0], od), (dt, ok, n_dup)
        assert (np.abs(d.numpy()[:, 0] - rd) / np.maximum(1.0, rd)).max() < 1e-6          # (squared distances ~20: one float32 ulp = 1.9e-6)
        d2, i2 = M(B.T[None], A.T[None], dist_type=dt)
        assert d2.shape == (1, 12, 1, 257) and np.array_equal(i2.numpy()[0].T, i.numpy())
        d7, i7 = knn_module.KNN(1).find_nn_gpu(torch.from_numpy(z['A7']), torch.from_numpy(z['B7']), nn_max_n=64, dist_type=dt)
        od7, oi7 = O.knn(z['B7'], z['A7'], 1, dist_type=dt)
        assert np.array_equal(i7.numpy(), z[f'nn7_i_{dt}']) and np.array_equal(i7.numpy(), oi7) and np.array_equal(d7.numpy(), od7)
        assert (np.abs(d7.numpy() - z[f'nn7_d_{dt}']) / np.maximum(1.0, d7.numpy())).max() < 1e-6
    # the generic kernel against the tuned one on the pipeline's own width: the first five of a k = 9 list are the k = 5 list
    g = load_golden('knn_api')
    a, b = torch.from_numpy(g['A']).cuda(), torch.from_numpy(g['B']).cuda()
    for sq in (False, True):
        i5, d5 = hip.knn_search(a, b, 5, want_dist=True, squared=sq)
        i9, d9 = hip.knn_search(a, b, 9, want_dist=True, squared=sq)
        assert torch.equal(i9[:, :5], i5) and torch.equal(d9[:, :5], d5)
    with pytest.raises(NotImplementedError):
        knn_module.KNN(33).find_knn_gpu(A, B)


def test_mutual_matches_bit_exact():
    from roreg_amd import hip
    rng = np.random.default_rng(4)
    for m, n in [(5000, 4800), (37, 50), (1, 1), (2500, 2500)]:
        nn01 = rng.integers(0, n, m); nn10 = rng.integers(0, m, n)
        good = rng.random(m) < 0.5
        for i in np.where(good)[0]:
            nn10[nn01[i]] = i
        s0 = rng.permutation(m + 10)[:m]; s1 = rng.permutation(n + 10)[:n]
        want = O.mutual_check(nn01, nn10)
        want = np.stack([s0[want[:, 0]], s1[want[:, 1]]], 1)
        out, cnt = hip.mutual_matches(cu(nn01), cu(nn10), cu(s0), cu(s1))
        c = int(cnt.item())
        assert c == want.shape[0]
        assert np.array_equal(out[:c].cpu().numpy(), want)


def test_mutual_match_batch_equals_oracle_and_per_pair_calls():
    """The batched matcher (paired-target packed-f32 scan) is bit-identical to the oracle and to the per-pair entry points:
    ragged task sizes, odd target counts, identity row lists, a one-row cloud, duplicate descriptors (first-minimum ties)."""
    from roreg_amd import hip
    rng = np.random.default_rng(11)

    def cloud(n):
        a = rng.standard_normal((n, 32)).astype(np.float32)
        return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    base = cloud(700)
    clouds = [base, (base[rng.permutation(700)[:613]] + 0.05 * rng.standard_normal((613, 32))).astype(np.float32), cloud(1), cloud(255),
              np.concatenate([base[:100], base[:100]])]                       # last: every descriptor twice -> distance ties
    specs = [(0, 1, 'perm', 'perm'), (1, 0, None, 'perm'), (0, 4, 'perm', None), (2, 3, None, None), (3, 2, 'perm', None), (4, 4, None, None)]
    tasks, host = [], []
    for a, b, ra, rb in specs:
        A, B = clouds[a], clouds[b]
        r0 = rng.permutation(A.shape[0])[:max(1, A.shape[0] - 3)] if ra else None
        r1 = rng.permutation(B.shape[0])[:max(1, B.shape[0] - 2)] if rb else None
        tasks.append((cu(A), cu(B), cu(r0) if r0 is not None else None, cu(r1) if r1 is not None else None))
        host.append((A, B, r0, r1))
    mbuf, cnt = hip.mutual_match_batch(tasks)
    cnt = cnt.cpu().numpy(); mbuf = mbuf.cpu().numpy()
    for q, ((A, B, r0, r1), t) in enumerate(zip(host, tasks)):
        sa = A if r0 is None else A[r0]; sb = B if r1 is None else B[r1]
        _, nn01 = O.knn(sb, sa, 1); _, nn10 = O.knn(sa, sb, 1)
        want = O.mutual_check(nn01, nn10)
        i0 = np.arange(sa.shape[0]) if r0 is None else r0; i1 = np.arange(sb.shape[0]) if r1 is None else r1
        want = np.stack([i0[want[:, 0]], i1[want[:, 1]]], 1)
        assert cnt[q] == want.shape[0], q
        assert np.array_equal(mbuf[q, :cnt[q]], want), q
        # and the per-pair C-ABI entry points give the same
        a01 = hip.nn_search(t[0], t[1], src_rows=t[2], tgt_rows=t[3]); a10 = hip.nn_search(t[1], t[0], src_rows=t[3], tgt_rows=t[2])
        out, c = hip.mutual_matches(a01, a10, t[2], t[3])
        assert int(c.item()) == cnt[q] and np.array_equal(out[:cnt[q]].cpu().numpy(), mbuf[q, :cnt[q]])
    e_buf, e_cnt = hip.mutual_match_batch([])
    assert e_cnt.numel() == 0


def test_des2r_bit_exact(group):
    from roreg_amd import hip
    z = load_golden('des2r')
    idx, cor = hip.des2r(cu(z['d1']), cu(z['d2']), want_cor=True)
    want = O.des2r_cor(z['d1'], z['d2'], group.P)
    assert np.array_equal(cor.cpu().numpy(), want)
    assert np.array_equal(idx.cpu().numpy(), want.argmax(1))
    assert np.array_equal(idx.cpu().numpy(), z['idx'])
    # with row lists
    rng = np.random.default_rng(1)
    r1 = rng.integers(0, z['d1'].shape[0], 50); r0 = rng.integers(0, z['d1'].shape[0], 50)
    idx2 = hip.des2r(cu(z['d1']), cu(z['d2']), rows1=cu(r1), rows0=cu(r0)).cpu().numpy()
    assert np.array_equal(idx2, O.des2r(z['d1'][r1], z['d2'][r0], group.P))


def test_feat_coefs_are_the_orthonormal_transform(group):
    from roreg_amd import hip
    from roreg_amd.fourier import group_fourier
    rng = np.random.default_rng(4)
    x = rng.standard_normal((77, 32, 60)).astype(np.float32)
    got = hip.feat_coefs(cu(x)).cpu().numpy()
    want = x.astype(np.float64) @ group_fourier().F.T
    assert got.shape == (77, 32, 60) and np.abs(got - want).max() < 2e-6
    gb = hip.feat_coefs(cu(x).to(torch.bfloat16)).cpu().numpy()                  # bfloat16 storage, float32 arithmetic
    wb = cu(x).to(torch.bfloat16).float().cpu().numpy().astype(np.float64) @ group_fourier().F.T
    assert np.abs(gb - wb).max() < 2e-6


@pytest.mark.parametrize('scale', [1.0, 300.0, 1e-3])
def test_des2r_irrep_bound_with_exact_recheck_is_the_literal_argmax(group, scale):
    """The irrep-domain Des2R (bound from sum_d d^3 = 244 multiply-adds per channel + literal re-evaluation of the candidates) returns the
    literal kernel's index on every row, including exact ties (duplicated rotations), near ties at the 1e-7..1e-3 level and
    correspondences whose correlation is pure noise; and it only re-evaluates a small share of ordinary rows."""
    from roreg_amd import hip
    rng = np.random.default_rng(12)
    n = 3000
    d2 = rng.standard_normal((n, 32, 60)).astype(np.float32)
    d1 = rng.standard_normal((n, 32, 60)).astype(np.float32)                      # rows 0..999: unrelated (noise-level correlations)
    a = rng.integers(0, 60, n)
    for i in range(1000, 2000):                                                  # planted rotation + noise: a clear winner
        d1[i][:, group.P[a[i]]] = d2[i]
        d1[i] += 0.3 * rng.standard_normal((32, 60)).astype(np.float32)
    for i in range(2000, 2400):                                                  # two planted rotations with equal weight: exact / near ties
        b = (a[i] + 1 + i % 58) % 60
        d1[i] = 0
        d1[i][:, group.P[a[i]]] += d2[i]
        tmp = np.zeros((32, 60), np.float32); tmp[:, group.P[b]] = d2[i]
        d1[i] += tmp * np.float32(1.0 + (0.0 if i % 4 == 0 else 10.0 ** -(i % 7 + 1)))
    d1[2400:2700] = d1[2000:2300]; d2[2400:2700] = d2[2000:2300]                  # duplicates of the tie rows
    d1[2700:] = 0                                                                # all-zero side: every correlation is 0 -> index 0
    d1 *= np.float32(scale); d2 *= np.float32(scale)
    D1, D2 = cu(d1), cu(d2)
    want = hip.des2r(D1, D2)                                                     # the literal kernel (itself bit-exact vs the oracle / golden)
    c1, c2 = hip.feat_coefs(D1), hip.feat_coefs(D2)
    hip.des2r_recheck_count()
    got = hip.des2r(D1, D2, coefs1=c1, coefs0=c2)
    assert torch.equal(got, want)
    n_all = hip.des2r_recheck_count()
    assert n_all >= 600                                                          # the tie rows and the all-zero rows took the exact path
    got = hip.des2r(D1, D2, rows1=cu(np.arange(2000)), rows0=cu(np.arange(2000)), coefs1=c1, coefs0=c2)
    assert torch.equal(got, want[:2000]) and hip.des2r_recheck_count() < 0.15 * 2000    # ordinary rows: mostly the bound alone
    # bfloat16 feature storage: coefficients and literal re-evaluation both see the bf16-rounded values
    B1, B2 = D1.to(torch.bfloat16), D2.to(torch.bfloat16)
    wantb = hip.des2r(B1.float(), B2.float())
    gotb = hip.des2r(B1, B2, coefs1=hip.feat_coefs(B1), coefs0=hip.feat_coefs(B2))
    assert torch.equal(gotb, wantb)


def test_des2r_irrep_margin_on_largest_irrep_near_ties(group):
    """Adversarial for the candidate margin of the irrep-domain Des2R (csrc/des2r.hip header): descriptors that live entirely in the
    5-dimensional irrep (where sum |terms| of the irrep evaluation is largest relative to |d1||d2|: the entrywise-absolute representation
    matrices reach spectral norm sqrt(5)) carrying TWO planted rotations whose correlations differ by 1e-6 .. 3e-4 of |d1||d2| -- the range
    around the margin, where a too-small margin would drop the literal winner from the candidate set.  The index must be the literal
    kernel's on every row."""
    from roreg_amd import hip
    from roreg_amd.fourier import group_fourier
    gf = group_fourier()
    F5 = gf.F[int(gf.offsets[4]):int(gf.offsets[5])]                              # [25, 60] rows of the d = 5 irrep
    proj = (F5.T @ F5)                                                            # projector onto its isotypic subspace
    rng = np.random.default_rng(31)
    n = 4096
    d2 = (rng.standard_normal((n, 32, 60)) @ proj).astype(np.float32)
    d1 = np.zeros_like(d2)
    a = rng.integers(0, 60, n); b = (a + 1 + rng.integers(0, 59, n)) % 60
    gaps = 10.0 ** rng.uniform(-6.0, -3.5, n) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
    for i in range(n):
        d1[i][:, group.P[a[i]]] += d2[i]
        tmp = np.zeros((32, 60), np.float32); tmp[:, group.P[b[i]]] = d2[i]
        d1[i] += tmp * np.float32(1.0 + gaps[i])
    for scale in (1.0, 1e-3, 37.0):
        D1, D2 = cu(d1 * np.float32(scale)), cu(d2 * np.float32(scale))
        want = hip.des2r(D1, D2)
        got = hip.des2r(D1, D2, coefs1=hip.feat_coefs(D1), coefs0=hip.feat_coefs(D2))
        assert torch.equal(got, want), int((got != want).sum())
    picked = want.cpu().numpy()
    assert np.mean((picked == a) | (picked == b)) > 0.99                          # the winner is one of the two planted rotations


def test_des2r_recovers_planted_rotation(group):
    from roreg_amd import hip
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2000, 32, 60)).astype(np.float32)
    a = rng.integers(0, 60, 2000)
    xr = np.empty_like(x)
    for i in range(2000):
        xr[i][:, group.P[a[i]]] = x[i]            # d1[:, P[a,g]] = d2[:, g]  ->  cor[a] is the full autocorrelation
    assert np.array_equal(hip.des2r(cu(xr), cu(x)).cpu().numpy(), a)


def test_quat_to_trans_vs_oracle(group):
    from roreg_amd import hip
    z = load_golden('et_forward')
    rng = np.random.default_rng(6)
    M = z['quaternion'].shape[0]
    q = (z['quaternion'] * rng.uniform(0.5, 2.0, (M, 1))).astype(np.float32)      # un-normalised head output
    k0 = rng.uniform(0, 3, (M, 3)); k1 = rng.uniform(0, 3, (M, 3))
    anchor = z['pre_idx']
    T, qn = hip.quat_to_trans(cu(q), cu(anchor), cu(k0), cu(k1), want_quat=True)
    qn_ref = (q / np.sqrt((q * q).sum(1))[:, None]).astype(np.float32)
    want = O.rt_pre(qn.cpu().numpy(), anchor, group.R.astype(np.float32), k0, k1)
    assert np.abs(qn.cpu().numpy() - qn_ref).max() < 1e-6
    assert np.abs(T.cpu().numpy() - want).max() < 1e-12


@pytest.mark.parametrize('tag', ['ones', 'f32'])
def test_ransac_score_masks_bit_exact(tag):
    from roreg_amd import hip
    z = load_golden('ransac')
    k0, k1, sc, Tr = z[f'{tag}_k0'], z[f'{tag}_k1'], z[f'{tag}_scores'], z[f'{tag}_Trans']
    f32 = sc.dtype == np.float32                                  # the rotation-coherence matcher's scores: numpy's float32 reductions
    ov, best, mask = hip.ransac_score(cu(k0), cu(k1), cu(sc.astype(np.float64)), cu(Tr), 0.1, want_mask=True, w_f32=f32)
    assert np.array_equal(mask.cpu().numpy().astype(bool), z[f'{tag}_masks'])
    ovh = ov.cpu().numpy()
    if tag == 'ones':
        assert np.array_equal(ovh, z[f'{tag}_overlap'])          # integer sums: exact
    else:
        assert z[f'{tag}_overlap'].dtype == np.float32
        assert np.array_equal(ovh.astype(np.float32), z[f'{tag}_overlap']) and np.array_equal(ovh.astype(np.float32).astype(np.float64), ovh)
    assert int(best.item()) == int(z[f'{tag}_best'])
    T1 = hip.refine(cu(k0), cu(k1), cu(sc.astype(np.float64)), 0.2, Trans=cu(Tr), best=best, w_f32=f32)
    T2 = hip.refine(cu(k0), cu(k1), cu(sc.astype(np.float64)), 0.1, T_in=T1, w_f32=f32)
    tol = 1e-9
    assert np.abs(T1.cpu().numpy() - z[f'{tag}_refine1']).max() < tol
    assert np.abs(T2.cpu().numpy() - z[f'{tag}_refine2']).max() < tol


def test_refine_rank1_edge_via_host_lapack():
    """Two inliers: H has rank 1 and U V^T is LAPACK's arbitrary completion; the stats path reproduces it."""
    from roreg_amd.test.estimator import refiner
    z = load_golden('ransac')
    T = refiner().Refine_trans(z['rank1_k0'], z['rank1_k1'], z['rank1_T'], np.ones(6), inlinerdist=0.1)
    assert np.abs(T - z['rank1_refined']).max() < 1e-9


def test_refine_single_inlier_edge():
    from roreg_amd import hip
    z = load_golden('ransac')
    T = hip.refine(cu(z['single_k0']), cu(z['single_k1']), cu(np.ones(5)), 0.1, T_in=cu(z['single_T'])).cpu().numpy()
    assert np.allclose(T, z['single_refined'], atol=1e-12)


def test_ransac_hypothesis_subset_and_full_size_properties():
    """BASELINE-size run (M=5000, H=1000) checked through properties: overlap in [0,1], the planted
    transform wins, masks agree with the oracle on a sampled hypothesis."""
    from roreg_amd import hip
    from roreg_amd.group import tables
    rng = np.random.default_rng(9)
    M = 5000
    R = tables().R[33]; t = np.array([0.4, 0.1, -0.3])
    k1 = rng.uniform(0, 3, (M, 3)); k0 = k1 @ R.T + t + 0.01 * rng.standard_normal((M, 3))
    bad = rng.random(M) < 0.4; k0[bad] = rng.uniform(0, 3, (bad.sum(), 3))
    Tr = np.zeros((M, 3, 4))
    for i in range(M):
        Rg = tables().R[int(rng.integers(0, 60))] if i % 7 else R
        Tr[i, :, :3] = Rg; Tr[i, :, 3] = k0[i] - k1[i] @ Rg.T
    rows = rng.permutation(M)[:1000]
    w = np.ones(M)
    ov, best, mask = hip.ransac_score(cu(k0), cu(k1), cu(w), cu(Tr), 0.1, hyp_rows=cu(rows), want_mask=True)
    ovh = ov.cpu().numpy()
    assert ovh.min() >= 0 and ovh.max() <= 1
    b = int(best.item())
    assert ovh[b] == ovh.max() and b == int(np.argmax(ovh))
    assert np.array_equal(mask[b].cpu().numpy().astype(bool), O.inlier_mask(k0, k1, Tr[rows[b]], 0.1))
    assert abs(ovh[b] - (~bad).mean()) < 0.05


def test_ransac_batch_equals_per_pair_calls():
    """The batched estimator tail (five launches for all pairs) is bitwise the per-pair entry points: ragged M and H, weights
    given / implied ones, hypothesis row lists given / identity, a failed pair (no consistent transform), a 3-match pair."""
    from roreg_amd import hip
    from roreg_amd.group import tables
    rng = np.random.default_rng(21)
    R60 = tables().R
    keys = [rng.uniform(0, 3, (900, 3)) for _ in range(3)]
    specs = [(0, 1, 700, 300, True, True, 0.3), (1, 2, 333, None, False, False, 0.5), (2, 0, 3, None, True, False, 0.0),
             (0, 2, 512, 100, False, True, 1.0), (1, 0, 64, 64, True, True, 0.2)]
    tasks, per_pair = [], []
    for a, b, M, H, use_w, use_rows, bad_frac in specs:
        g = int(rng.integers(0, 60)); t = rng.uniform(-0.5, 0.5, 3)
        r1 = rng.permutation(900)[:M]; r0 = rng.permutation(900)[:M]
        K0 = keys[a].copy(); K1 = keys[b].copy()
        K0[r0] = K1[r1] @ R60[g].T + t + 0.01 * rng.standard_normal((M, 3))
        bad = rng.random(M) < bad_frac
        K0[r0[bad]] = rng.uniform(0, 3, (int(bad.sum()), 3))
        matches = np.stack([r0, r1], 1).astype(np.int64)
        nT = M if use_rows else (H or M)
        Tr = np.zeros((nT, 3, 4))
        for i in range(nT):
            Rg = R60[g] if i % 3 == 0 else R60[int(rng.integers(0, 60))]
            j = i % M
            Tr[i, :, :3] = Rg; Tr[i, :, 3] = K0[r0[j]] - K1[r1[j]] @ Rg.T
        rows = rng.permutation(nT)[:H] if (use_rows and H) else None
        w = rng.uniform(0.1, 1.0, M) if use_w else None
        d = dict(k0=cu(K0), k1=cu(K1), m=cu(matches), w=cu(w) if w is not None else None, Tr=cu(Tr), rows=cu(rows) if rows is not None else None)
        tasks.append((d['k0'], d['k1'], d['m'], d['w'], d['Tr'], d['rows'])); per_pair.append((d, M))
    ird = 0.1
    best, T1, st1, T2, st2 = [x.cpu().numpy() for x in hip.ransac_batch(tasks, ird)]
    for q, (d, M) in enumerate(per_pair):
        k0 = hip.gather_rows_f64(d['k0'], d['m'][:, 0].contiguous()); k1 = hip.gather_rows_f64(d['k1'], d['m'][:, 1].contiguous())
        w = d['w'] if d['w'] is not None else torch.ones(M, dtype=torch.float64, device='cuda')
        _, b, _ = hip.ransac_score(k0, k1, w, d['Tr'], ird, hyp_rows=d['rows'])
        a1, s1 = hip.refine(k0, k1, w, ird * 2.0, Trans=d['Tr'], hyp_rows=d['rows'], best=b, want_stats=True)
        a2, s2 = hip.refine(k0, k1, w, ird, T_in=a1, want_stats=True)
        assert int(b.item()) == best[q], q
        for got, want in ((T1[q], a1), (st1[q], s1), (T2[q], a2), (st2[q], s2)):
            assert np.array_equal(got.reshape(-1), want.cpu().numpy().reshape(-1), equal_nan=True), q
    # the same with float32-score arithmetic (tasks without weights keep the float64 form, in the batch as per pair)
    best32, T1f, st1f, T2f, st2f = [x.cpu().numpy() for x in hip.ransac_batch(tasks, ird, w_f32=True)]
    for q, (d, M) in enumerate(per_pair):
        k0 = hip.gather_rows_f64(d['k0'], d['m'][:, 0].contiguous()); k1 = hip.gather_rows_f64(d['k1'], d['m'][:, 1].contiguous())
        w = d['w'] if d['w'] is not None else torch.ones(M, dtype=torch.float64, device='cuda')
        f32 = d['w'] is not None
        _, b, _ = hip.ransac_score(k0, k1, w, d['Tr'], ird, hyp_rows=d['rows'], w_f32=f32)
        a1, s1 = hip.refine(k0, k1, w, ird * 2.0, Trans=d['Tr'], hyp_rows=d['rows'], best=b, want_stats=True, w_f32=f32)
        a2, s2 = hip.refine(k0, k1, w, ird, T_in=a1, want_stats=True, w_f32=f32)
        assert int(b.item()) == best32[q], q
        for got, want in ((T1f[q], a1), (st1f[q], s1), (T2f[q], a2), (st2f[q], s2)):
            assert np.array_equal(got.reshape(-1), want.cpu().numpy().reshape(-1), equal_nan=True), ('w_f32', q)
    assert hip.ransac_batch([], ird)[0].numel() == 0
    # one more refinement of SOME tasks from given transforms in one launch (the engine's pass over rank-deficient pairs) == per-pair calls,
    # float64 and float32-score arithmetic
    for w_f32 in (False, True):
        out = hip.ransac_batch(tasks, ird, w_f32=w_f32, keep=True)
        ctx = out[5]
        sel = [3, 0, 4, 2]
        Tin = rng.standard_normal((len(sel), 4, 4)) * 0.01 + np.asarray(T1)[sel]
        Tb, sb = hip.refine_batch(ctx, sel, Tin, ird)
        for pos, q in enumerate(sel):
            d, M = per_pair[q]
            k0 = hip.gather_rows_f64(d['k0'], d['m'][:, 0].contiguous()); k1 = hip.gather_rows_f64(d['k1'], d['m'][:, 1].contiguous())
            w = d['w'] if d['w'] is not None else torch.ones(M, dtype=torch.float64, device='cuda')
            a, st = hip.refine(k0, k1, w, ird, T_in=cu(Tin[pos]), want_stats=True, w_f32=w_f32 and d['w'] is not None)
            assert np.array_equal(Tb[pos].cpu().numpy().reshape(-1), a.cpu().numpy().reshape(-1), equal_nan=True), (w_f32, q)
            assert np.array_equal(sb[pos].cpu().numpy(), st.cpu().numpy().reshape(-1), equal_nan=True), (w_f32, q)
    assert hip.refine_batch(ctx, [], np.zeros((0, 4, 4)), ird)[0].shape == (0, 4, 4)


def test_gather_rows_batch_equals_index_select():
    """Several (tensor, row list) gathers in one launch: float32 / bfloat16 [*,32,60] feature rows and float64 [*,3] keypoint rows, ragged
    counts incl. an empty task, repeated and unordered indices -- bitwise torch.index_select."""
    from roreg_amd import hip
    g = torch.Generator(device='cuda').manual_seed(4)
    for dtype, shape in ((torch.float32, (32, 60)), (torch.bfloat16, (32, 60)), (torch.float64, (3,))):
        srcs = [torch.randn((n,) + shape, device='cuda', generator=g, dtype=torch.float32).to(dtype) for n in (700, 64, 1300)]
        rows = [torch.randint(0, s.shape[0], (k,), device='cuda', generator=g) for s, k in zip(srcs, (513, 0, 2500))]
        out = torch.zeros((sum(r.shape[0] for r in rows),) + shape, device='cuda', dtype=dtype)
        tasks, o = [], 0
        for s, r in zip(srcs, rows):
            tasks.append((s, r, out[o:o + r.shape[0]])); o += r.shape[0]
        hip.gather_rows_batch(tasks)
        want = torch.cat([torch.index_select(s, 0, r) for s, r in zip(srcs, rows)])
        assert torch.equal(out, want), dtype
    hip.gather_rows_batch([])


def test_lt_batch_equals_per_pair_calls(group):
    """Batched Des2R + ET-input assembly + quaternion->transform against the per-pair entry points: ragged n, hypothesis
    selections given / all matches, an empty task."""
    from roreg_amd import hip
    rng = np.random.default_rng(31)
    clouds = []
    for n in (120, 77, 200):
        clouds.append(dict(before=cu(rng.standard_normal((n, 32, 60)).astype(np.float32)), eqv=cu(rng.standard_normal((n, 32, 60)).astype(np.float32)),
                           keys=cu(rng.uniform(0, 3, (n, 3)))))
    specs = [(0, 1, 60, 25), (1, 2, 40, None), (2, 0, 90, 90), (0, 2, 5, 0)]
    tasks, host = [], []
    for a, b, M, nsel in specs:
        c0, c1 = clouds[a], clouds[b]
        m = np.stack([rng.integers(0, c0['keys'].shape[0], M), rng.integers(0, c1['keys'].shape[0], M)], 1).astype(np.int64)
        sel = rng.permutation(M)[:nsel] if nsel is not None else None
        md = cu(m); sd = cu(sel) if sel is not None else None
        tasks.append((c0['before'], c1['before'], c0['eqv'], c1['eqv'], c0['keys'], c1['keys'], md, sd))
        host.append((c0, c1, m if sel is None else m[sel]))
    # the same tasks with coefficient tensors: Des2R through the irrep-domain bound + exact re-check -> identical indices
    for c in clouds:
        c['ft'] = hip.feat_coefs(c['eqv'])
    tasks_ft = [t + (clouds[a]['ft'], clouds[b]['ft']) for t, (a, b, _, _) in zip(tasks, specs)]
    assert torch.equal(hip.LtBatch(tasks_ft).des2r(), hip.LtBatch(tasks).des2r())
    batch = hip.LtBatch(tasks)
    dr, x = batch.prepare(batch.total + 3)
    assert float(x[batch.total:].abs().max()) == 0.0
    q = cu(rng.standard_normal((batch.total, 4)).astype(np.float32))
    T = batch.finish(q, dr)
    for (o, n), (c0, c1, m) in zip(batch.offsets, host):
        assert n == m.shape[0]
        if n == 0:
            continue
        r0 = cu(m[:, 0].copy()); r1 = cu(m[:, 1].copy())
        dr1 = hip.des2r(c1['eqv'], c0['eqv'], rows1=r1, rows0=r0)
        x1 = hip.et_gather(c0['before'], c1['before'], c0['eqv'], c1['eqv'], dr1, rows0=r0, rows1=r1)
        T1 = hip.quat_to_trans(q[o:o + n].contiguous(), dr1, c0['keys'], c1['keys'], rows0=r0, rows1=r1)
        assert torch.equal(dr[o:o + n], dr1) and torch.equal(x[o:o + n], x1) and torch.equal(T[o:o + n], T1)


@pytest.mark.parametrize('scale', [1.0, 37.5, 0.02])
def test_mfma_matcher_is_exact_on_adversarial_descriptors(scale):
    """The matrix-core matcher (approximate minima + exact check of the candidates) must reproduce the literal formula's first-minimum
    indices where a plain dot-product expansion fails: clustered descriptors (thousands of near ties at the 1e-4..1e-7 level), exact
    duplicates, descriptors of very different norms, any overall scale."""
    from roreg_amd import hip
    rng = np.random.default_rng(5)
    centers = rng.standard_normal((40, 32)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    A = (centers[rng.integers(0, 40, 1500)] + 1e-3 * rng.standard_normal((1500, 32))).astype(np.float32)
    A[100:200] = A[0:100]                                                  # exact duplicates: ties resolved by the first index
    A[300:400] += (1e-6 * rng.standard_normal((100, 32))).astype(np.float32)
    B = (centers[rng.integers(0, 40, 1300)] + 1e-3 * rng.standard_normal((1300, 32))).astype(np.float32)
    B[50:90] = A[500:540]                                                  # zero distances
    B[200:260] *= np.float32(3.0)                                          # a few descriptors with 9x the squared norm
    A = (A * np.float32(scale)).astype(np.float32); B = (B * np.float32(scale)).astype(np.float32)
    mbuf, cnt = hip.mutual_match_batch([(cu(A), cu(B), None, None), (cu(B), cu(A), None, None)])
    cnt = cnt.cpu().numpy(); mbuf = mbuf.cpu().numpy()
    for q, (S, T) in enumerate(((A, B), (B, A))):
        _, nn01 = O.knn(T, S, 1); _, nn10 = O.knn(S, T, 1)
        want = O.mutual_check(nn01, nn10)
        assert cnt[q] == want.shape[0] and np.array_equal(mbuf[q, :cnt[q]], want), (scale, q)


def test_knn_search_segmented_equals_per_cloud():
    """Several clouds stacked (ragged sizes around the 256-row blocks): local indices equal the per-cloud search, ties included."""
    from roreg_amd import hip
    rng = np.random.default_rng(2)
    sizes = [5, 255, 256, 257, 1000, 77]
    clouds = [rng.uniform(0, 1, (n, 3)).astype(np.float32) for n in sizes]
    clouds[3][10:20] = clouds[3][0]                                       # exact duplicates: first index wins
    pts = cu(np.concatenate(clouds))
    got = hip.knn_search_seg(pts, hip.Segments(sizes), 5).cpu().numpy()
    o = 0
    for c in clouds:
        want = hip.knn_search(cu(c), cu(c), 5).cpu().numpy()
        assert np.array_equal(got[o:o + len(c)], want)
        o += len(c)


@pytest.mark.gpu
@pytest.mark.parametrize('env', [{'ROREG_MATCH_TILES': '1'}, {'ROREG_MATCH_BF16X3': '1'}, {'ROREG_GEMM_PIPE': '0'},
                                 {'ROREG_DES2R_SPLIT': '0'}, {'ROREG_DES2R_SPLIT': '1'}, {'ROREG_DES2R_NCH': '8'},
                                 {'ROREG_TOPK_LDS': '0'}, {'ROREG_TOPK_LDS': '0', 'ROREG_TOPK_PACKED': '1'}],
                         ids=['matcher per-tile form', 'matcher 3 x bf16 split', 'GEMM loop without fragment pipelining',
                              'gathered correlation: round-2 kernel', 'gathered correlation: bank-split + packed math', 'gathered correlation: 8 channels per pass',
                              'top-k: a tile per wavefront', 'top-k: packed list maintenance'])
def test_alternative_kernel_forms_stay_correct(env):
    """The kernel variants kept behind environment switches (the per-tile matcher passes, the matcher's 3 x bf16 operand split, the
    irrep GEMM's plain loop; round 6: the earlier forms of the gathered correlation and of the top-k search) are chosen once per process,
    so each runs the relevant exactness tests in a process of its own."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if 'ROREG_GEMM_PIPE' in env:
        args = ['tests/test_hip_fourier.py', '-k', 'gemm or extractor or batch_invariant']
    elif 'ROREG_DES2R_SPLIT' in env or 'ROREG_DES2R_NCH' in env:
        args = ['tests/test_hip_kernels.py', 'tests/test_hip_rm.py', '-k', 'des2r or group_corr or symmetry']
    elif 'ROREG_TOPK_LDS' in env:
        args = ['tests/test_hip_rm.py', '-k', 'topk or match_ot or stacked']
    else:
        args = ['tests/test_hip_kernels.py', 'tests/test_hip_knn.py', '-k', 'mutual or matcher']     # (test_hip_knn.py: mutual_match_batch on the tie families)
    r = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider'] + args + ['--deselect',
                        'tests/test_hip_kernels.py::test_alternative_kernel_forms_stay_correct'], cwd=root, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode()
    assert r.returncode == 0 and ' passed' in out, out[-2000:]


@pytest.mark.gpu
def test_gemm_pipelined_loop_is_bitwise_the_plain_loop():
    """irrep GEMM (fp16 x 2, 256 x 256 tile): the fragment-pipelined loop issues the same MFMAs per accumulator in the same order as
    the plain loop -- identical bits on 61440-keypoint launches of four layer shapes with heavy-tailed operands and bound propagation (tools/gemm_checksum.py)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sums = []
    for pipe in ('1', '0'):
        r = subprocess.run([sys.executable, 'tools/gemm_checksum.py'], cwd=root, env=dict(os.environ, ROREG_GEMM_PIPE=pipe), stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        lines = [l for l in r.stdout.decode().splitlines() if l.startswith('checksum')]
        assert r.returncode == 0 and lines, r.stdout.decode()[-2000:]
        assert len(lines) == 4, lines                       # GF's big layer, its two thin ones (4-wave and 8-wave tiles), ET's Conv_init
        sums.append(lines)
    assert sums[0] == sums[1], sums


def test_gathered_correlation_does_not_depend_on_the_tables_symmetry(group):
    """The R_indicator / Des2R kernel lays its permuted row out by a symmetry it finds in the permutation table (runtime.hip bank_split_table:
    an involution of the rotation group pairs lanes and LDS slots so that no two lanes of a half-wave share a bank).  Any table whose rows are
    permutations is a valid input: one WITHOUT that symmetry gets the plain assignment and must give the same bit-exact correlations (only
    the conflict rate depends on the assignment) -- here a table of random row permutations, checked against the oracle's literal order, both
    table orientations; then the real tables are restored and give the golden's answer again."""
    from roreg_amd import hip
    hip.ensure_tables()
    T = hip.tables()
    rng = np.random.default_rng(12)
    P_odd = np.stack([rng.permutation(60) for _ in range(60)]).astype(np.int32)
    d1 = rng.standard_normal((137, 32, 60)).astype(np.float32); d2 = rng.standard_normal((137, 32, 60)).astype(np.float32)
    nei, R = np.ascontiguousarray(T.Nei, np.int32), np.ascontiguousarray(T.R, np.float64)
    try:
        hip._check(hip.lib().roreg_set_group_tables(P_odd.ctypes.data, nei.ctypes.data, R.ctypes.data), 'roreg_set_group_tables')
        idx, cor = hip.des2r(cu(d1), cu(d2), want_cor=True)
        want = O.des2r_cor(d1, d2, P_odd)
        assert np.array_equal(cor.cpu().numpy(), want) and np.array_equal(idx.cpu().numpy(), want.argmax(1))
        got_t = hip.group_corr(cu(d1), cu(d2), perm_rows=None, bcast_rows=None, transpose=True).cpu().numpy()
        assert np.array_equal(got_t, O.des2r_cor(d1, d2, np.ascontiguousarray(P_odd.T)))
    finally:
        P = np.ascontiguousarray(T.P, np.int32)
        hip._check(hip.lib().roreg_set_group_tables(P.ctypes.data, nei.ctypes.data, R.ctypes.data), 'roreg_set_group_tables')
    z = load_golden('des2r')
    assert np.array_equal(hip.des2r(cu(z['d1']), cu(z['d2'])).cpu().numpy(), z['idx'])
