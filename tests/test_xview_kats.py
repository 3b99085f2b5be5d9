"""Known answers for the cross-view prediction contract of include/mvhdp.h, on the host: the restatement (tests/native/xview_ref.c) against
exact rational arithmetic and hand-derived cases, its order and rank definitions, and how far a reordered or unfused chain moves the
scores of the GPU test's own inputs -- so that the bit-for-bit GPU test cannot pass on another summation."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import xview_cases as xc
from tests import xview_ref as xr


def fma_exact(a, b, c):
    """a correctly rounded fused multiply-add: the exact rational a * b + c, rounded once by float()"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def test_the_rank_count_and_the_marker_are_the_shared_ones():
    """(the select / order pair of this unit stays its own: as one kernel on wave_first_n it was slower, profiles/select_refactor.md)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvtopicmodel_amd", "csrc")
    unit, header = open(os.path.join(csrc, "mvhdp_xview.hip")).read(), open(os.path.join(csrc, "mvhdp_select.h")).read()
    assert header.count("int wave_first_n(") == 1 and "int wave_first_n(" not in unit                # one copy, in the shared header
    assert header.count("int wave_rank_count(") == 1 and "= wave_rank_count(" in unit and "wave_count(" not in unit
    assert "constexpr u64 XV_EXCLUDED" in open(os.path.join(csrc, "mvhdp_xview.h")).read() and "constexpr u64 XV_EXCLUDED" not in unit


@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
def test_the_chain_is_a_sequence_of_correctly_rounded_fmas(K):
    rng = np.random.default_rng(K)
    for trial in range(50):
        theta = rng.random(K) ** 3
        nwk = rng.integers(0, 5, (1, K)).astype(np.int32)
        nk = nwk[0] + rng.integers(0, 50, K).astype(np.int32)
        phi = xr.phi_table(nwk, nk, 0.01, 0.37)[0]
        for k in range(K):                                                   # phi: one correctly rounded division of two rounded sums
            assert phi[k] == float(Fraction(float(nwk[0, k]) + 0.01) / Fraction(float(nk[k]) + 0.37))
        s = 0.0
        for k in range(K):
            s = fma_exact(theta[k], phi[k], s)
        assert xr.chain(theta, phi) == s
        assert xr.scores(theta[None, :], phi[None, :])[0, 0] == s


def test_a_hand_derived_case_with_binary_exact_numbers():
    # K = 2, V = 3, beta = 0.5, betaSum = 2: n_k = (6, 2) -> denominators 8 and 4; rows (1, 1), (3, 0), (0, 1) -> numerators 1.5 1.5 | 3.5 0.5 | 0.5 1.5
    nwk = np.array([[1, 1], [3, 0], [0, 1]], dtype=np.int32)
    nk = np.array([6, 2], dtype=np.int32)
    phi = xr.phi_table(nwk, nk, 0.5, 2.0)
    assert phi.tolist() == [[0.1875, 0.375], [0.4375, 0.125], [0.0625, 0.375]]
    theta = np.array([[0.25, 0.75], [1.0, 0.0]])
    S = xr.scores(theta, phi)
    assert S.tolist() == [[0.328125, 0.203125, 0.296875], [0.1875, 0.4375, 0.0625]]
    items, sc, counts = xr.predict(S, 4)
    assert items.tolist() == [[0, 2, 1, -1], [1, 0, 2, -1]] and counts.tolist() == [3, 3]
    assert sc.tolist() == [[0.328125, 0.296875, 0.203125, 0.0], [0.4375, 0.1875, 0.0625, 0.0]]
    # an inactive topic is exactly 0.0 in every row
    phi0 = xr.phi_table(nwk, nk, 0.5, 2.0, inactive=[0, 1])
    assert phi0.tolist() == [[0.1875, 0.0], [0.4375, 0.0], [0.0625, 0.0]]
    assert xr.scores(theta, phi0)[0].tolist() == [0.046875, 0.109375, 0.015625]


def test_equal_rows_give_equal_scores_and_the_id_decides():
    rng = np.random.default_rng(4)
    K, V = 7, 9
    nwk = rng.integers(0, 4, (V, K)).astype(np.int32)
    nwk[6] = nwk[2]; nwk[8] = nwk[2]                                         # three equal rows
    nk = nwk.sum(0).astype(np.int32)
    S = xr.scores(rng.random((5, K)), xr.phi_table(nwk, nk, 0.01, 0.09))
    assert (S[:, 2] == S[:, 6]).all() and (S[:, 2] == S[:, 8]).all()
    items, sc, counts = xr.predict(S, V)
    for d in range(5):
        row = items[d].tolist()
        assert sorted(row) == list(range(V)) and counts[d] == V
        assert row.index(2) + 1 == row.index(6) and row.index(6) + 1 == row.index(8)
        assert all(sc[d, i] > sc[d, i + 1] or (sc[d, i] == sc[d, i + 1] and row[i] < row[i + 1]) for i in range(V - 1))
        assert sc[d].tolist() == [S[d, w] for w in row]


def test_the_rank_counts_what_precedes_and_is_not_excluded():
    S = np.array([[0.5, 0.25, 0.5, 0.125, 0.25]])                            # order: 0 2 1 4 3
    ent = np.zeros(5, dtype=np.int64)
    score, rank = xr.score_pairs(S, ent, np.arange(5))
    assert rank.tolist() == [0, 2, 1, 4, 3] and score.tolist() == S[0].tolist()
    off, tok = np.array([0, 3]), np.array([2, 1, 2])                         # the entity holds types 1 and 2 (2 twice); a token >= V is none of them
    score, rank = xr.score_pairs(S, ent, np.arange(5), True, off, tok)
    assert rank.tolist() == [0, 1, 1, 2, 1] and score.tolist() == S[0].tolist()   # 1 and 2 are ranked although excluded; nobody counts them
    items, sc, counts = xr.predict(S, 5, True, off, tok)
    assert items.tolist() == [[0, 4, 3, -1, -1]] and counts.tolist() == [3] and sc.tolist() == [[0.5, 0.25, 0.125, 0.0, 0.0]]
    items, _, counts = xr.predict(S, 2, True, np.array([0, 5]), np.arange(5))                 # every type excluded
    assert items.tolist() == [[-1, -1]] and counts.tolist() == [0]
    # repeated and unsorted pairs are answered one by one
    S2 = np.vstack([S, S[:, ::-1]])                                          # the second row's order: 2 4 0 3 1
    score, rank = xr.score_pairs(S2, np.array([1, 0, 1, 1]), np.array([4, 3, 0, 4]))
    assert rank.tolist() == [1, 4, 2, 1] and score.tolist() == [0.5, 0.125, 0.25, 0.5]


@pytest.mark.parametrize("shape", [s for s in xc.SHAPES if s[0] >= 64], ids=str)
def test_a_reordered_or_unfused_chain_moves_the_scores_of_the_gpu_inputs(shape):
    """On the GPU test's own inputs with K >= 64: the chain in descending k changes the bits of at least half of the scores, the unfused
    chain s + a * b at least a tenth of them."""
    c = xc.make(*shape)
    nwk, nk = c.counts(c.m)
    phi = xr.phi_table(nwk, nk, c.hy.beta[c.m], c.hy.beta_sum[c.m])
    theta = c.theta()[:40]
    S = xr.scores(theta, phi)
    desc = float((xr.scores(theta, phi, xr.DESCENDING) != S).mean())
    unfused = float((xr.scores(theta, phi, xr.UNFUSED) != S).mean())
    print(shape, "descending changes", desc, "unfused changes", unfused)
    assert desc >= 0.5 and unfused >= 0.1
