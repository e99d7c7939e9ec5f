"""The float64 Sinkhorn oracle, the restated early-exit rule and the input families of tests/test_sinkhorn_convergence.py: the inputs are
what they claim to be, from the oracles alone.  CPU only (torch on the host)."""
import numpy as np
import pytest

import _sinkhorn_cases as C
from oracle import match_ot_numpy as MO


def test_early_exit_iteration_restates_the_rule():
    """conv_stop (csrc/ot_flash.hip): skip iteration t >= 1 if steps[t-1] <= 1; or t >= 2, steps[t-1] <= 8 and steps[t-1] >= steps[t-2]."""
    E = MO.early_exit_iteration
    assert E([500, 30, 0.9, 0.1]) == 3                         # (a)
    assert E([0.5, 100, 100]) == 1                             # (a) may fire right after iteration 0 ...
    assert E([5, 5, 5]) == 2                                   # ... (b) needs two recorded steps: 5 <= 8 and 5 >= 5
    assert E([500, 9, 7, 6, 6, 3]) == 5                        # (b): equal steps count as "not smaller"
    assert E([500, 9, 7, 6, 6.5, 3]) == 5
    assert E([500, 20, 9, 8.5, 8.5, 8.25]) == 6                # above the band a plateau does not stop; strictly shrinking steps do not either
    assert E([500, 20, 9, 8.5, 8.5, 8.0, 8.0]) == 7
    assert E([500, 7, 6, 5, 4, 3, 2]) == 7                     # a monotone sequence runs until (a)
    assert E([500, 7, 6, 5, 4, 3, 2, 1.0, 77]) == 8
    assert E([]) == 0 and E([3.0]) == 1 and E([0.0]) == 1


def test_float64_oracle_is_the_formula_of_the_float32_oracle():
    """log_sinkhorn_steps against log_sinkhorn (pinned to the reference's golden) on a small pair: float64 within float32's rounding of it,
    the float32 replay likewise; the step record in units of max(2^-22 |u|, 2^-20 ln 2) shrinks to (a) and stays there."""
    rng = np.random.default_rng(3)
    s, t = C.planted(rng, 50, 37, 0.25)
    score = (s @ t.T).astype(np.float32)
    want = MO.log_sinkhorn(score, np.float32(1.5), 100)
    Z64, st64 = MO.log_sinkhorn_steps(score, 1.5, 100, 'float64')
    Z32, st32 = MO.log_sinkhorn_steps(score, 1.5, 100, 'float32')
    assert Z64.dtype == np.float64 and Z32.dtype == np.float32 and Z64.shape == want.shape == (51, 38)
    assert np.abs(Z64 - want).max() < 1e-5 and np.abs(Z32 - want).max() < 1e-5
    assert st64.shape == (100,) and st64[0] > 1e4 and st64[-1] < 1e-3          # float64 goes on shrinking far below one float32 unit
    assert (np.diff(st64[:20]) < 0).all()
    assert st32[-1] <= 2.0 and MO.early_exit_iteration(st32) < 40
    # the couplings are a transport plan: rows and columns of exp(Z + norm) sum to mu, nu
    P = np.exp(Z64 - np.log(50 + 37))
    assert np.abs(P.sum(1)[:-1] - 1 / 87).max() < 1e-9 and abs(P.sum(1)[-1] - 37 / 87) < 1e-9
    assert np.abs(P.sum(0)[:-1] - 1 / 87).max() < 1e-12 and abs(P.sum(0)[-1] - 50 / 87) < 1e-12
    # 0 iterations: the raw scores with the dustbins, shifted by -norm
    Z0, st0 = MO.log_sinkhorn_steps(score, 1.5, 0)
    assert st0.shape == (0,) and np.allclose(Z0[:50, :37], score.astype(np.float64) + np.log(87.0)) and np.allclose(Z0[50], 1.5 + np.log(87.0))


@pytest.mark.parametrize('name', list(C.CASES))
def test_case_belongs_to_its_class(name):
    """Class membership by the rule replayed on the float32 iteration's own step record (slow: the stop lies in [40, 95] and the float64
    iteration still moves by more than a unit there; fast: below 40; never: no stop before 100); the reference's own noise (float32, all 100
    iterations, against float64) within a quarter of the bar the kernels are held to; the arg-max filter of the GPU test leaves out at most
    5 % of the rows and of the columns.  Measured: slow cases stop at 72 .. 90 with float64 steps of 3.3 .. 5.9 units, float32 noise
    4.8e-6 .. 6.7e-6 (bar 1.35e-4 .. 1.49e-4), 1.2 .. 4.3 % left out."""
    cls = C.CASES[name][0]
    s, t = C.descriptors(name)
    m, n = s.shape[0], t.shape[0]
    assert (m, n) == C.CASES[name][3:5] and s.dtype == t.dtype == np.float32
    Z64, st64 = C.reference(name)
    Z32, st32 = C.replay32(name)
    stop = MO.early_exit_iteration(st32)
    noise = float(np.abs(Z32 - Z64).max())
    keep0, keep1 = C.decided(Z64, m, n)
    print(f'[{name}] float32 replay stops at {stop}, float64 step there {st64[min(stop, C.ITERS - 1)]:.2f} units, float32 vs float64 max|dZ| {noise:.2e} '
          f'(bar {C.bar_Z(Z64):.2e}), max|Z| {np.abs(Z64).max():.1f}, undecided rows {1 - keep0.mean():.3f} columns {1 - keep1.mean():.3f}')
    if cls == 'slow':
        assert 40 <= stop <= 95, stop
        assert st64[stop] > 1.0, st64[stop]
        stop64 = MO.early_exit_iteration(st64)                      # float64 itself shrinks its steps monotonically: (b) never fires on it,
        assert stop64 > stop and (stop64 == C.ITERS or st64[stop64 - 1] <= 1.0), stop64       # and (a) only later, if at all
        assert (np.diff(st64[stop - 10:]) < 0).all()
    elif cls == 'fast':
        assert stop < 40, stop
    else:
        assert stop == C.ITERS and st32.min() > 8.0, (stop, st32.min())
    assert noise <= 0.25 * C.bar_Z(Z64), (noise, C.bar_Z(Z64))
    assert keep0.mean() >= 0.95 and keep1.mean() >= 0.95, (keep0.mean(), keep1.mean())


def test_duplicated_rows_are_exact_ties():
    s, t = C.descriptors('slow_1000x1000_dup')
    assert np.array_equal(t[40:50], t[3:13]) and np.array_equal(s[100:107], s[20:27])
    Z64, _ = C.reference('slow_1000x1000_dup')
    assert np.array_equal(Z64[:, 40:50], Z64[:, 3:13]) and np.array_equal(Z64[100:107], Z64[20:27])
