"""The input families of tests/test_hip_ransac_f32_sums.py are what they claim to be, from the oracle and numpy alone: the planted inlier
sets are the oracle's masks, the oracle's overlap is the written-out pairwise model of np.sum, the inputs tell a wrong reduction order
from numpy's, and the tree of every chunk fits the kernel's tables.  CPU only."""
import re
import pathlib

import numpy as np
import pytest

import _ransac_sum_cases as C
from oracle import ref_numpy as O

ALL = [(name, seed) for name in C.CASES for seed in C.SEEDS[name]]


def sequential_f32(a):
    return np.cumsum(a, dtype=np.float32)[-1] if a.size else np.float32(0)


def float64_then_rounded(a):
    return np.float32(np.sum(a.astype(np.float64)))


@pytest.mark.parametrize('name', list(C.CASES))
def test_planted_groups_are_the_oracle_masks_and_overlap_is_the_model(name):
    M, counts = C.CASES[name]
    assert len(C.SEEDS[name]) >= 4
    for seed in C.SEEDS[name]:
        k0, k1, sc, Tr, group = C.case(name, seed)
        assert sc.dtype == np.float32 and k0.shape == k1.shape == (M, 3) and Tr.shape == (len(counts), 3, 4)
        assert np.array_equal(k1 * 8, np.round(k1 * 8))
        ov, best = C.oracle(name, seed)
        for h, n in enumerate(counts):
            inl = O.inlier_mask(k0, k1, Tr[h], C.IRD)
            assert np.array_equal(inl, group == h) and int(inl.sum()) == n, (seed, h)
            assert np.array_equal(O.inlier_mask(k0, k1, Tr[h], 2 * C.IRD), inl), (seed, h)     # the first refinement's radius: the same set
            want = np.float32(O.np_sum_f32_model(sc[inl])) / np.float32(M)
            assert type(ov[h]) is np.float32 and ov[h] == want, (seed, h)
            if n == 0:
                assert ov[h] == np.float32(0.0)
        assert best == int(np.argmax(ov)) and ov[best] > 0 and (ov[:best] < ov[best]).all()


def test_spill_and_boundary_cases():
    """The mixed chunk cases carry part of a ballot group over the chunk boundary (case() asserts it for every case of SPILL and denies it
    for the all-inlier case); at least two of them do."""
    assert len(C.SPILL) >= 2
    for name in C.SPILL + ('C_all',):
        for seed in C.SEEDS[name]:
            group = C.case(name, seed)[4]
            idx = np.where(group == 0)[0]
            lane = int(idx[C.NP_CHUNK - 1] % 64)
            assert (lane == 63) == (name == 'C_all'), (name, seed, lane)


def test_cases_tell_orders_apart():
    """For every count >= 16 some seed gives scores whose sequential float32 sum is not np.sum's value, for every count >= 129 some seed
    gives scores whose float64 accumulation, rounded once, is not: a kernel that summed in either order fails the device test."""
    for name, (M, counts) in C.CASES.items():
        for h, n in enumerate(counts):
            sums = []
            for seed in C.SEEDS[name]:
                sc, group = C.case(name, seed)[2], C.case(name, seed)[4]
                a = sc[group == h]
                sums.append((np.sum(a), sequential_f32(a), float64_then_rounded(a)))
            if n >= 16:
                assert any(s[1] != s[0] for s in sums), (name, n)
            if n >= 129:
                assert any(s[2] != s[0] for s in sums), (name, n)
    for name, (M, counts) in C.REFINE_CASES.items():           # the refinement's sum (stats[15]): one seed, the larger groups
        sc, group = C.case(name, C.REFINE_SEED)[2], C.case(name, C.REFINE_SEED)[4]
        for h, n in enumerate(counts):
            if n >= 1000:
                a = sc[group == h]
                assert sequential_f32(a) != np.sum(a), (name, n)


def test_refine_cases_are_as_planted():
    for name, (M, counts) in C.REFINE_CASES.items():
        k0, k1, sc, Tr, group = C.case(name, C.REFINE_SEED)
        for h, n in enumerate(counts):
            inl = O.inlier_mask(k0, k1, Tr[h], C.IRD)
            assert np.array_equal(inl, group == h) and int(inl.sum()) == n
            if n >= 8:                                             # non-degenerate: a well-conditioned cross-covariance
                T = O.refine_trans(k0, k1, Tr[h], sc, C.IRD)
                a = k0[inl] - k0[inl].mean(0); b = k1[inl] - k1[inl].mean(0)
                sv = np.linalg.svd(a.T @ b, compute_uv=False)
                assert sv[2] > 1e-2 * sv[0] and np.abs(T[:3] - Tr[h]).max() < 0.05


def test_every_chunk_tree_fits_the_kernel_tables():
    """np_pairwise_sum_wave (csrc/ransac.hip) keeps the leaves of one chunk's recursion in tables of NP_MAX_LEAVES entries and its pending
    nodes on stacks of fixed depth: the bound holds for every length a chunk can have."""
    src = (pathlib.Path(__file__).resolve().parents[1] / 'roreg_amd' / 'csrc' / 'ransac.hip').read_text()
    cap = int(re.search(r'constexpr int NP_MAX_LEAVES = (\d+);', src).group(1))
    stack = int(re.search(r'int32_t stack\[(\d+)\];', src).group(1)); vstack = int(re.search(r'float vstack\[(\d+)\];', src).group(1))
    assert int(re.search(r'constexpr int NP_CHUNK = (\d+);', src).group(1)) == C.NP_CHUNK
    most_leaves = most_pending = most_values = 0
    for n in range(1, C.NP_CHUNK + 1):
        leaves, vals, st = 0, 0, [n]
        while st:                                                  # the kernel's second walk: -1 marks "add the two values on top"
            most_pending = max(most_pending, len(st))
            m = st.pop()
            if m < 0:
                vals -= 1
            elif m <= 128:
                leaves += 1; vals += 1; most_values = max(most_values, vals)
            else:
                n2 = 8 * (m // 16)
                st += [-1, m - n2, n2]
        assert vals == 1
        most_leaves = max(most_leaves, leaves)
    assert most_leaves <= cap and most_pending <= stack and most_values <= vstack, (most_leaves, most_pending, most_values)
