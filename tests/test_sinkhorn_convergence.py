"""Sinkhorn on HIP against a float64 evaluation of the reference's formula after all 100 iterations, on inputs that converge SLOWLY
(tests/_sinkhorn_cases.py: clustered descriptors; what makes them slow is pinned on the CPU by tests/test_sinkhorn_oracle.py) beside fast
and never-settling controls: every form of the iteration, with the per-pair early exit (csrc/ot_flash.hip, conv_stop) on and off.  GPU only.

The bar is bar_Z = 1e-4 * max(1, max|Z_ref| / 20) throughout -- the one test_hip_rm.py holds the kernels to against the float32 oracle; the
float32 oracle itself sits at 0.03 .. 0.13 of it on these cases (test_sinkhorn_oracle.py).  Every test prints what it measured in lines
starting with '[convergence]' (pytest -s)."""
import numpy as np
import pytest
import torch

import _sinkhorn_cases as C
from oracle import match_ot_numpy as MO

pytestmark = pytest.mark.gpu

FORM_NAMES = {True: 'recomputed', 'coop': 'recomputed, coop', False: 'materialised', 'literal': 'literal one-pair kernel'}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_stacked(names, recompute, on):
    """-> ([matches0, matches1, mscores0, mscores1] numpy, source offsets, target offsets, (iterations run, pairs))"""
    from roreg_amd import hip
    D = [C.descriptors(k) for k in names]
    alphas = {C.CASES[k][6] for k in names}
    assert len(alphas) == 1                                            # (one dustbin score per call)
    seg_s = hip.Segments([s.shape[0] for s, _ in D]); seg_t = hip.Segments([t.shape[0] for _, t in D])
    hip.sinkhorn_iteration_stats()
    with hip.sinkhorn_early_exit(on):
        out = hip.sinkhorn_batch(cu(np.concatenate([s for s, _ in D])), cu(np.concatenate([t for _, t in D])), seg_s, seg_t, alphas.pop(), C.ITERS,
                                 recompute=recompute)
    return [x.cpu().numpy() for x in out], seg_s.host, seg_t.host, hip.sinkhorn_iteration_stats()


# (form, early exit): the exit lives in the recomputed iterations only -- the materialised form and the literal kernel always run all of them
FORMS = [pytest.param(True, True, id='recomputed-exit_on'), pytest.param(True, False, id='recomputed-exit_off'),
         pytest.param('coop', True, id='coop-exit_on'), pytest.param('coop', False, id='coop-exit_off'),
         pytest.param(False, True, id='materialised'), pytest.param('literal', True, id='literal')]


@pytest.mark.parametrize('form,on', FORMS)
@pytest.mark.parametrize('name', list(C.CASES))
def test_log_couplings_of_one_pair_against_float64(name, form, on):
    """max |Z_dev - Z_ref| <= bar_Z for one pair per call.  With the exit OFF the figure is the kernels' arithmetic alone (fp16 hi/lo
    recomputation, float32 potentials); ON adds whatever tail of the iteration the rule left undone.  Executed iterations of the recomputed
    forms: fast pairs < 60, never pairs == 100, all 100 with the exit off; for slow pairs the count is recorded, not asserted.

    Measured on an MI355X, slow cases (bar 1.35e-4 .. 1.49e-4; float32 oracle 4.8e-6 .. 6.7e-6): exit off 5.5e-6 .. 8.6e-6 in every form
    (0.9 .. 1.3 x the float32 oracle); exit on 3.6e-5 .. 6.4e-5 after 71 .. 87 iterations (7 .. 12 x; 0.26 .. 0.47 of the bar).  Fast and never
    cases 0.7 .. 1.3 x either way.  Table: DESIGN.md section 4.6, profiles/r08_sinkhorn_slow_convergence.txt."""
    from roreg_amd import hip
    cls, alpha = C.CASES[name][0], C.CASES[name][6]
    s, t = C.descriptors(name)
    Z_ref, _ = C.reference(name)
    noise32 = float(np.abs(C.replay32(name)[0] - Z_ref).max())
    bar = C.bar_Z(Z_ref)
    hip.sinkhorn_iteration_stats()
    if form == 'literal':
        Z = hip.sinkhorn(cu(s), cu(t), alpha, C.ITERS)[0]
        ran = None
    else:
        with hip.sinkhorn_early_exit(on):
            Z = hip.sinkhorn_batch(cu(s), cu(t), hip.Segments([s.shape[0]]), hip.Segments([t.shape[0]]), alpha, C.ITERS, recompute=form, want_Z=True)[0]
        st = hip.sinkhorn_iteration_stats()
        ran = st[0] if form is not False else None
        assert st == ((0, 0) if form is False else (st[0], 1)), st               # (the statistics count the recomputed forms only)
    err = float(np.abs(Z.cpu().numpy().astype(np.float64) - Z_ref).max())
    print(f'[convergence] {name:24s} {FORM_NAMES[form]:24s} exit {"on " if on and ran is not None else ("off" if ran is not None else "n/a")} '
          f'iterations {ran if ran is not None else C.ITERS:3d}  max|dZ| {err:.2e}  bar {bar:.2e}  x float32 oracle {err / noise32:6.1f}')
    if ran is not None:
        if not on:
            assert ran == C.ITERS, ran
        elif cls == 'fast':
            assert 2 <= ran < 60, ran
        elif cls == 'never':
            assert ran == C.ITERS, ran
    assert err <= bar, (name, form, on, err, bar)


@pytest.mark.parametrize('recompute,on', FORMS[:5])
def test_stacked_read_out_against_float64(recompute, on):
    """All classes ragged in one call (per dustbin score): matches0 / matches1 equal the read-out of Z_ref wherever its arg-max is decided by
    more than 1e-3 on both sides of the mutual check; the matching scores are exp(Z) and small here (0.007 .. 0.12), so on agreeing rows
    |s_dev / s_ref - 1| <= bar_Z (a relative error of exp(Z) IS an absolute error of Z)."""
    for alpha in sorted({c[6] for c in C.CASES.values()}):
        names = [k for k, c in C.CASES.items() if c[6] == alpha]
        (g0, g1, gs0, gs1), hs, ht, st = run_stacked(names, recompute, on)
        worst = 0.0
        for q, name in enumerate(names):
            m, n = C.CASES[name][3:5]
            Z_ref, _ = C.reference(name)
            w0, w1, ws0, ws1 = MO.readout(Z_ref)
            keep0, keep1 = C.decided(Z_ref, m, n)
            h0, h1 = g0[hs[q]:hs[q] + m], g1[ht[q]:ht[q] + n]
            assert np.array_equal(h0[keep0], w0[keep0]) and np.array_equal(h1[keep1], w1[keep1]), (name, int((h0[keep0] != w0[keep0]).sum()), int((h1[keep1] != w1[keep1]).sum()))
            assert (w0[keep0] >= 0).sum() >= 5, name                            # (the comparison below is not empty)
            for keep, h, w, hsc, wsc in ((keep0, h0, w0, gs0[hs[q]:hs[q] + m], ws0), (keep1, h1, w1, gs1[ht[q]:ht[q] + n], ws1)):
                sure = keep & (h == w) & (w >= 0)
                rel = float(np.abs(hsc[sure].astype(np.float64) / wsc[sure].astype(np.float64) - 1).max(initial=0.0))
                worst = max(worst, rel / C.bar_Z(Z_ref))
                assert rel <= C.bar_Z(Z_ref), (name, rel, C.bar_Z(Z_ref))
                assert np.all(hsc[keep & (w < 0)] == 0)
        print(f'[convergence] stacked {names} {FORM_NAMES[recompute]}, exit {"on" if on else "off"}: iterations {st[0]} over {st[1]} pairs, worst score error {worst:.2f} of the bar')


@pytest.mark.parametrize('mode', [True, 'coop'])
def test_slow_pair_is_bitwise_the_same_stacked_and_alone(mode):
    """A pair's convergence record depends on its own data only: with the exit on, every slow pair's matches AND scores are bitwise the same
    alone and stacked beside fast pairs (which stop some sixty iterations before it)."""
    names = [k for k, c in C.CASES.items() if c[6] == C.ALPHA_RM]
    stacked, hs, ht, st = run_stacked(names, mode, True)
    total = 0
    for q, name in enumerate(names):
        if name not in C.SLOW:
            continue
        m, n = C.CASES[name][3:5]
        one, _, _, st1 = run_stacked([name], mode, True)
        total += st1[0]
        assert np.array_equal(stacked[0][hs[q]:hs[q] + m], one[0]) and np.array_equal(stacked[1][ht[q]:ht[q] + n], one[1]), name
        assert np.array_equal(stacked[2][hs[q]:hs[q] + m], one[2]) and np.array_equal(stacked[3][ht[q]:ht[q] + n], one[3]), name
    rest = sum(run_stacked([k], mode, True)[3][0] for k in names if k not in C.SLOW)
    assert st == (total + rest, len(names)), (st, total, rest)                  # and the stacked call ran exactly the pairs' own iterations
