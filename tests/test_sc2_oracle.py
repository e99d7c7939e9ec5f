"""The spatial-compatibility estimator without a GPU: the conditions the device tests rely on hold for every case under the oracle alone
(threshold margin, conditioning filter), the definition recovers the ground truth of the 60 %, 90 % and 95 % outlier cases, and the feature's
plumbing exists (stage registry, configuration, C-ABI table)."""
import os
import re

import numpy as np
import pytest

import _sc2_cases as C
import _sc2_oracle as O
from oracle import ref_numpy as R
from roreg_amd.utils.r_eval import compute_R_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_threshold_margin_of_every_case():
    """no off-diagonal |a_ij - b_ij| lies within 1e-10 of tau: a last-bit difference of a square root cannot flip a bit of C"""
    for case in C.stage_cases() + C.recovery_cases():
        print(f'{case.name}: margin {case.margin:.1e}')
        assert case.margin >= 1e-10, case.name
        assert np.array_equal(case.ref.C, case.ref.C.T) and not case.ref.C.diagonal().any()


def test_cases_cover_what_they_are_for():
    tied = C.tied_case()
    assert (tied.ref.deg == tied.P.shape[0] - 1).all() and np.array_equal(tied.ref.seeds, np.arange(tied.P.shape[0]))
    assert np.array_equal(tied.ref.cons[5], [5] + [j for j in range(20) if j != 5])
    out = C.all_outlier_case()
    members = (out.ref.cons >= 0).sum(1)
    assert (members < 3).sum() >= 20 and (members >= 3).sum() >= 20 and out.ref.deg.max() < out.K - 1
    dup = C.duplicates_case()
    assert dup.ref.C[5, 3] and dup.ref.C[3, 40] and dup.ref.diff[5, 3] == 0.0
    for case in (C.synth_case(11, 129, 0.6, K=64), C.synth_case(11, 65, 0.9, K=64)):
        assert (case.ref.deg < case.K - 1).any()                  # K - 1 greater than some seeds' degree
    short = C.synth_case(11, 257, 0.6, max_seeds=10)
    assert short.ref.seeds.shape == (10,) and short.ref.N2.shape == (10, 257)


def test_conditioning_filter_leaves_out_at_most_a_tenth():
    """the device tests compare a fitted row only where sigma2 / sigma1 >= 1e-3: at most 10 % of a case's fitted rows may fall outside"""
    for case in C.stage_cases():
        fitted, ok = C.fitted_rows(case)
        print(f'{case.name}: {int(fitted.sum())} fitted rows, {int((fitted & ~ok).sum())} left out')
        assert (fitted & ~ok).sum() <= C.MAX_CONDITION_DROP * fitted.sum(), case.name
        Rm = case.ref.Trans[fitted][:, :, :3]
        assert np.abs(np.linalg.det(Rm) - 1.0).max(initial=0.0) < 1e-12


def test_determinant_fix_is_exercised():
    """the all-outlier case fits random sets: about half of their U V^T are reflections, which the fix turns into the oracle's rotations"""
    case = C.all_outlier_case()
    fitted, ok = C.fitted_rows(case)
    assert (np.linalg.det(C.unfixed_rotations(case, ok)) < 0).sum() >= 10


def test_oracle_bit_rows():
    case = C.synth_case(11, 129, 0.6)
    bits = case.ref.bits
    assert bits.shape == (129, 3) and bits.dtype == np.uint64
    for i, j in ((0, 1), (5, 64), (128, 127), (77, 128), (3, 3)):
        assert bool(int(bits[i, j // 64]) >> (j % 64) & 1) == bool(case.ref.C[i, j])
    assert (bits[:, 2] >> np.uint64(1) == 0).all()               # columns 129..191 are padding
    assert np.array_equal(np.array([bin(int(w)).count('1') for w in bits.reshape(-1)]).reshape(129, 3).sum(1), case.ref.deg)


@pytest.mark.parametrize('idx', [0, 1, 2])
def test_recovery(idx):
    """scored with the oracle's overlap and refined twice, the winner lies within 1 degree / 2 cm of the ground truth"""
    case = C.recovery_cases()[idx]
    Tg = C.ground_truth()
    ov = np.array([R.overlap_cal(case.P, case.Q, T, case.scores, case.tau) for T in case.ref.Trans])
    best = int(np.argmax(ov))                                     # np.argmax: the first of the greatest, like the running '>' scan
    T0 = case.ref.Trans[best]
    T2 = R.refine_trans(case.P, case.Q, R.refine_trans(case.P, case.Q, T0, case.scores, 2 * case.tau), case.scores, case.tau)
    for name, T, rot, tr in (('before refinement', T0, 1.0, 0.02), ('refined', T2, 1.0, 0.02)):
        rre = compute_R_diff(Tg[:3, :3], T[:3, :3]); rte = float(np.linalg.norm(Tg[:3, 3] - T[:3, 3]))
        print(f'{case.name}: winner row {best}, {name}: {rre:.3f} deg / {rte * 1e3:.1f} mm')
        assert rre < rot and rte < tr, (case.name, name, rre, rte)


def test_plumbing():
    from roreg_amd import _abi
    from roreg_amd.parses.parses_test import default_config
    from roreg_amd.test import name2estimator
    cfg = default_config(ET='sc2')
    assert cfg.ET == 'sc2' and default_config().ET == 'yohoc'
    est = name2estimator['sc2'](cfg)
    assert callable(est.run)
    assert 'roreg_sc2_workspace' in _abi.PROTOTYPES and 'roreg_sc2_hypotheses_batch' in _abi.PROTOTYPES
    assert _abi._SC2_TASK.itemsize == 64
    from roreg_amd import hip
    header = open(os.path.join(ROOT, 'include', 'roreg_hip.h')).read()
    for name, value in (('MAX_M', hip.SC2_MAX_M), ('SEED_TILE', hip.SC2_SEED_TILE), ('COL_TILE', hip.SC2_COL_TILE)):
        assert int(re.search(rf'#define\s+ROREG_SC2_{name}\s+(\d+)', header).group(1)) == value
    L = hip.lib()                                                 # a host function: works without a GPU
    import ctypes
    offs = (ctypes.c_size_t * 5)()
    total = L.roreg_sc2_workspace(100, 200, 1000, ctypes.cast(offs, ctypes.c_void_p))
    ends = [offs[0] + 2400, offs[1] + 2400, offs[2] + 1600, offs[3] + 400, offs[4] + 2000]
    assert all(e + 64 <= nx for e, nx in zip(ends, list(offs[1:]) + [total])) and all(o % 256 == 0 for o in offs)
    assert L.roreg_sc2_workspace(-1, 0, 0, None) == 0
