"""ET's first forward transform on rows read by reference (LtBatch.prepare_rows + hip.ft_nonlin_gathered) against the two-step route it replaces:
hip.et_gather assembles x, hip.row_bound bounds it, hip.ft_nonlin transforms it.  Everything is compared bit for bit.  GPU only."""
import dataclasses

import numpy as np
import pytest
import torch

from roreg_amd import synth
from roreg_amd.parses.parses_test import default_config

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _clouds(rng, sizes, dtype):
    out = []
    for n in sizes:
        before = cu(rng.standard_normal((n, 32, 60)).astype(np.float32)).to(dtype).contiguous()
        after = cu((rng.standard_normal((n, 32, 60)) * rng.uniform(0.2, 3.0, (n, 1, 1))).astype(np.float32)).to(dtype).contiguous()
        out.append((before, after))
    return out


def _bn(rng):
    # both signs of the scale and shifts large enough that the ReLU cuts whole channels: the maxima then differ between the four roles
    return cu((rng.standard_normal(128) * 1.5).astype(np.float32)), cu(rng.standard_normal(128).astype(np.float32))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_role_tables_equal_torch_amax(dtype):
    """role_max[b][k] = amax over (c, g) of relu(x * scale + shift) on channels k*32..k*32+31, x = before (k = 0, 1) or after (k = 2, 3).  The kernel
    uses one fused multiply-add per element; torch forms the same value in float64 (the product of two float32 is exact there, the sum is rounded
    once to 53 bits) and rounds it to float32."""
    from roreg_amd import hip
    rng = np.random.default_rng(7)
    (before, after), = _clouds(rng, [77], dtype)
    scale, shift = _bn(rng)
    got = hip.role_max(before, after, (scale, shift))
    assert got.shape == (77, 4) and got.dtype == torch.float32
    for k, x in enumerate((before, before, after, after)):
        sc = scale[k * 32:(k + 1) * 32].double()[None, :, None]; sh = shift[k * 32:(k + 1) * 32].double()[None, :, None]
        want = torch.relu((x.double() * sc + sh).float()).amax((1, 2))
        assert torch.equal(got[:, k].view(torch.int32), want.view(torch.int32)), k


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_role_columns_from_the_fused_kernels_equal_role_max(dtype):
    """The extractor's first bound kernel (before) and the matcher-descriptor kernel (after) fill the same table role_max computes, and their own
    results stay what they are without the table."""
    from roreg_amd import hip
    rng = np.random.default_rng(9)
    (before, after), = _clouds(rng, [131], dtype)
    bn = _bn(rng)
    want = hip.role_max(before, after, bn)
    role = torch.full((131, 4), float('nan'), dtype=torch.float32, device='cuda')
    bound = hip.row_bound(before, roles=(bn[0], bn[1], role))
    inv = hip.inv_descriptor(after, roles=(bn[0], bn[1], role))
    assert torch.equal(role.view(torch.int32), want.view(torch.int32))
    assert torch.equal(bound.view(torch.int32), hip.row_bound(before).view(torch.int32))
    assert torch.equal(inv.view(torch.int32), hip.inv_descriptor(after).view(torch.int32))


def _tasks(rng, clouds, with_sel):
    """Three pairs over three clouds: cloud 1 is side 1 of the first pair and side 0 of the second; the third pair has no correspondence.  The row
    count (61 + 38) is not a multiple of 32."""
    from roreg_amd import hip
    (bA, aA), (bB, aB), (bC, aC) = clouds
    nA, nB, nC = bA.shape[0], bB.shape[0], bC.shape[0]
    keys = [cu(rng.standard_normal((n, 3))) for n in (nA, nB, nC)]
    coefs = [hip.feat_coefs(a) for a in (aA, aB, aC)]
    m1 = cu(np.stack([rng.integers(0, nA, 90), rng.integers(0, nB, 90)], 1).astype(np.int64))
    m2 = cu(np.stack([rng.integers(0, nB, 38), rng.integers(0, nC, 38)], 1).astype(np.int64))
    m3 = torch.empty((0, 2), dtype=torch.int64, device='cuda')
    sel1 = cu(rng.permutation(90)[:61].astype(np.int64)) if with_sel else None
    if not with_sel:
        m1 = m1[:61].contiguous()
    return [(bA, bB, aA, aB, keys[0], keys[1], m1, sel1, coefs[0], coefs[1]),
            (bB, bC, aB, aC, keys[1], keys[2], m2, None, coefs[1], coefs[2]),
            (bA, bC, aA, aC, keys[0], keys[2], m3, None, coefs[0], coefs[2])]


@pytest.mark.parametrize('with_sel', [True, False])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_gathered_transform_equals_gather_then_transform(dtype, with_sel):
    from roreg_amd import hip
    rng = np.random.default_rng(11)
    clouds = _clouds(rng, [70, 50, 64], dtype)
    bn = _bn(rng)
    tasks = _tasks(rng, clouds, with_sel)
    roles = {id(b): hip.role_max(b, a, bn) for b, a in clouds}
    batch = hip.LtBatch([t + (roles[id(t[0])], roles[id(t[1])]) for t in tasks])
    assert batch.has_roles and batch.total == 99 and batch.offsets == [(0, 61), (61, 38), (99, 0)]
    dr, g = batch.prepare_rows()
    B = batch.total
    # the independent route, pair by pair through the per-pair API
    dr_ref, x_ref = [], []
    for (b0, b1, a0, a1, _, _, m, sel, c0, c1) in tasks:
        mm = m if sel is None else m[sel]
        if mm.shape[0] == 0:
            continue
        r0, r1 = mm[:, 0].contiguous(), mm[:, 1].contiguous()
        d = hip.des2r(a1, a0, rows1=r1, rows0=r0, coefs1=c1, coefs0=c0)
        dr_ref.append(d); x_ref.append(hip.et_gather(b0, b1, a0, a1, d, rows0=r0, rows1=r1))
    dr_ref, x_ref = torch.cat(dr_ref), torch.cat(x_ref)
    assert x_ref.shape == (B, 128, 60) and torch.equal(dr, dr_ref)
    bound_ref = hip.row_bound(x_ref, bn=bn)
    assert torch.equal(g.bound.view(torch.int32), bound_ref.view(torch.int32))
    assert float(g.bound[B:].abs().max()) == 0.0 and float(g.bound[:B].min()) > 0.0
    for planes in (False, True):
        want = hip.ft_nonlin(B, 128, x_spatial=x_ref, bn=bn, split='f16x2', out_bound=bound_ref, planes=planes)
        got = hip.ft_nonlin_gathered(g, bn=bn, planes=planes)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), planes
    # and the batched assembly, which the by-reference form replaces in the engine
    dr2, x2, xb2 = hip.LtBatch(tasks).prepare(bound_bn=bn)
    assert torch.equal(dr2, dr) and torch.equal(x2, x_ref) and torch.equal(xb2.view(torch.int32), g.bound.view(torch.int32))


def test_tasks_without_role_tables_keep_the_assembled_route():
    from roreg_amd import hip
    rng = np.random.default_rng(3)
    clouds = _clouds(rng, [70, 50, 64], torch.float32)
    tasks = _tasks(rng, clouds, False)
    batch = hip.LtBatch(tasks)
    assert not batch.has_roles
    with pytest.raises(hip.HipError):
        batch.prepare_rows()
    roles = hip.role_max(*clouds[0], _bn(rng))
    assert not hip.LtBatch([tasks[0] + (roles, hip.role_max(*clouds[1], _bn(rng))), tasks[1]]).has_roles       # all tasks or none


@pytest.mark.parametrize('name', ['fp32', 'bf16'])
def test_engine_local_transforms_by_reference_equal_the_assembled_route(name):
    """RegistrationEngine.local_transforms_many on clouds that carry role tables (rows by reference) and on the same clouds without them
    (x assembled by et_gather_batch_kernel): the same anchors and the same transforms, bit for bit."""
    from roreg_amd import hip
    from roreg_amd.engine import RegistrationEngine
    from roreg_amd.network import name2network
    cfg = default_config(keynum=300, max_iter=1000, ET='yohoo')
    gf = name2network['GF_test'](cfg); synth.seeded_state_dict(gf, 101)
    et = name2network['ET_test'](cfg); synth.seeded_state_dict(et, 202)
    ds = synth.make_scene(21, n_clouds=3, n_kpts=300, overlap=0.6)
    eng = RegistrationEngine(cfg, gf, et)
    eng.set_descriptor_dtype(name)
    clouds = eng.extract_many(ds.feats, [ds.get_kps(i) for i in ds.pc_ids])
    assert all(c.role is not None and c.role.shape == (300, 4) for c in clouds)
    bn = et.conv_init_bn()
    for c in clouds:
        assert torch.equal(c.role.view(torch.int32), hip.role_max(c.before, c.eqv, bn).view(torch.int32))
    one = eng.extract(ds.feats[1], ds.get_kps(ds.pc_ids[1]))
    assert torch.equal(one.role, clouds[1].role) and torch.equal(one.eqv, clouds[1].eqv)
    bare = [dataclasses.replace(c, role=None, role_bn=None) for c in clouds]
    rng = np.random.default_rng(5)
    m01 = cu(rng.integers(0, 300, (211, 2)).astype(np.int64)); m12 = cu(rng.integers(0, 300, (77, 2)).astype(np.int64))
    sel = cu(rng.permutation(211)[:150].astype(np.int64))
    items = lambda cs: [(cs[0], cs[1], m01, sel), (cs[1], cs[2], m12, None)]
    got = eng.local_transforms_many(items(clouds))
    want = eng.local_transforms_many(items(bare))
    for (dg, Tg), (dw, Tw) in zip(got, want):
        assert torch.equal(dg, dw) and torch.equal(Tg.view(torch.int64), Tw.view(torch.int64))
    # several passes of the ET network (max_rows below the total) see the same rows
    again = eng.local_transforms_many(items(clouds), max_rows=160)
    for (dg, Tg), (da, Ta) in zip(got, again):
        assert torch.equal(dg, da) and torch.equal(Tg.view(torch.int64), Ta.view(torch.int64))
