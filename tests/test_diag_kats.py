"""Known answers of the diagnostics checker (tests/diag_numpy.py) on a hand-built model: every expected number is written out here.
No device: these pin the checker that tests/test_gpu_diagnostics.py holds the device against.

The model (K = 3, view 0 of four types; topic 2 inactive, alpha0 = [0.5, 0.25, 0, 0.25], gamma0 = 1, alphaSum0 = 1, beta0 = 0.01):
  entity 0: types [0, 1, 1, 2], topics [0, 0, 0, 1]
  entity 1: types [1, 3],       topics [1, 1]
  entity 2: types [0, 2],       topics [0, 1]        (a rank-1 tie: topics 0 and 1 hold one token each)
  entity 3: view 0 present and empty; entity 4: view 0 absent (both: no tokens)
n_wk of view 0: type 0 -> topic 0: 2; type 1 -> topic 0: 2, topic 1: 1; type 2 -> topic 1: 2; type 3 -> topic 1: 1.
"""
import math

import numpy as np
import pytest

from tests import diag_numpy as dn

K, N = 3, 3
DOC_OFF = np.array([0, 4, 6, 8, 8, 8], np.int64)
TOKENS = np.array([0, 1, 1, 2, 1, 3, 0, 2], np.int32)
Z = np.array([0, 0, 0, 1, 1, 1, 0, 1], np.int32)
ALPHA0 = np.array([0.5, 0.25, 0.0, 0.25])
NWK0 = np.array([[2, 0, 0], [2, 1, 0], [0, 2, 0], [0, 1, 0]], np.int32)
NWK1 = np.array([[1, 1, 0], [0, 3, 0]], np.int32)
NWK2 = np.array([[0, 0, 0], [2, 2, 0]], np.int32)
NK0 = np.array([4, 4, 0], np.int32)
WORD_LENGTH = np.array([1, 2, 3, 4], np.int32)


def _run(word_length=WORD_LENGTH):
    return dn.diagnostics([NWK0, NWK1, NWK2], NK0, ALPHA0, 1.0, 1.0, 0.01, DOC_OFF, TOKENS, Z, N, word_length)


def test_top_words_ties_go_to_the_higher_type():
    t, c, nz = dn.top_words(NWK0, N)
    assert t.tolist() == [[1, 0, -1], [2, 3, 1], [-1, -1, -1]]
    assert c.tolist() == [[2, 2, 0], [2, 1, 1], [0, 0, 0]]
    assert nz.tolist() == [2, 3, 0]


def test_document_pass_integers():
    d = _run()
    assert d["num_tokens"] == 8
    assert d["word_type_counts"].tolist() == [2, 3, 2, 1]
    assert d["num_nonzero_docs"].tolist() == [2, 3, 0]
    assert d["num_rank1_docs"].tolist() == [2, 1, 0]                 # entity 2's tie goes to topic 0
    assert d["num_docs_at_proportions"].tolist() == [[2] * 7, [3, 3, 3, 3, 3, 2, 1], [0] * 7]


def test_codocument_matrices_with_the_padding_quirk():
    """Topic 0 has two words (types 1, 0): its third position holds type 0, so it is 'present' wherever type 0 is."""
    d = _run()
    assert d["codoc"][0].tolist() == [[1, 1, 1], [1, 2, 2], [1, 2, 2]]
    assert d["codoc"][1].tolist() == [[2, 0, 0], [0, 1, 1], [0, 1, 1]]
    assert d["codoc"][2].tolist() == [[0] * 3] * 3


def test_sum_count_log_count():
    d = _run()
    assert d["sum_count_log_count"].tolist() == [3 * math.log(3), 2 * math.log(2), 0.0]


def test_discr_weight_per_view_is_cumulative_over_three_views():
    assert dn.type_discr_weight(NWK0).tolist() == [1.0, 5 / 9, 1.0, 1.0]
    assert dn.type_discr_weight(NWK1).tolist() == [0.5, 1.0]
    assert dn.type_discr_weight(NWK2).tolist() == [0.0, 0.5]
    pv = dn.discr_weight_per_view([NWK0, NWK1, NWK2])
    np.testing.assert_allclose(pv, [32 / 45, 13 / 18, 25 / 36], rtol=1e-15)


def test_scores_with_an_inactive_topic():
    d = _run()
    s, w = d["scores"], d["word_scores"]
    l2, l3 = math.log(2), math.log(3)
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-13, atol=0)
    assert s["tokens"].tolist() == [4, 4, 0]
    close(s["document_entropy"][:2], [-3 * l3 / 4 + math.log(4), 1.5 * l2])
    assert math.isnan(s["document_entropy"][2])                       # -0/0 + log 0
    assert s["word-length"].tolist() == [1.0, 3.0, 0.0]
    assert w["word-length"].tolist() == [[2, 1, 0], [3, 4, 2], [0, 0, 0]]
    assert s["coherence"][0] == 0.0 and s["coherence"][2] == 0.0
    close(s["coherence"][1], 2 * math.log(0.01 / 2.01))
    close(w["coherence"][1], [0.0, math.log(0.01 / 2.01), math.log(0.01 / 2.01)])
    close(s["discrWeight"][:2], [424 / 784, 430 / 1024])
    assert s["discrWeight"][2] == 0.0 and s["normDiscrWeight"][2] == 0.0          # alpha0[2] == 0: left at 0
    close(s["normDiscrWeight"][:2], [(424 / 784) / math.log10(1.5), (430 / 1024) / math.log10(4 / 3)])
    close(s["uniform_dist"][:2], [l2, 0.5 * l2])
    close(w["uniform_dist"][0, :2], [0.5 * l2, 0.5 * l2])
    assert s["uniform_dist"][2] == 0.0 and s["corpus_dist"][2] == 0.0             # an empty TreeSet: 0, not NaN
    close(s["corpus_dist"][:2], [0.5 * math.log(4 / 3) + 0.5 * l2, 0.5 * l2 + 0.25 * l2 + 0.25 * math.log(2 / 3)])
    close(w["corpus_dist"][1], [0.5 * l2, 0.25 * l2, 0.25 * math.log(2 / 3)])
    close(s["eff_num_words"][:2], [2.0, 1 / 0.375])
    assert s["eff_num_words"][2] == math.inf                         # 1 / 0
    mean0, mean1 = (0.5 + 1 / 3) / 2, (0.5 + 2 / 3) / 2
    t0 = [0.25 * math.log(0.5 / mean0) + (1 / 6) * math.log((1 / 3) / mean0),
          0.25 * math.log(0.5 / mean1) + (1 / 3) * math.log((2 / 3) / mean1), 0.0]
    close(w["token-doc-diff"][0], t0)
    close(s["token-doc-diff"][0], sum(t0))
    assert s["token-doc-diff"][1] == 0.0 and s["token-doc-diff"][2] == 0.0
    close(s["rank_1_docs"][:2], [1.0, 1 / 3])
    close(s["allocation_ratio"][:2], [1.0, 1 / 3])
    close(s["allocation_count"][:2], [1.0, 2 / 3])
    for row in ("rank_1_docs", "allocation_ratio", "allocation_count"):
        assert math.isnan(s[row][2])                                   # 0 / 0
    assert all(math.isnan(x) for x in _run(None)["scores"]["word-length"])


def test_unassigned_or_out_of_vocabulary_token_is_refused():
    z = Z.copy()
    z[3] = -1
    with pytest.raises(dn.JavaArithmeticError):
        dn.diagnostics([NWK0], NK0, ALPHA0, 1.0, 1.0, 0.01, DOC_OFF, TOKENS, z, N)
    t = TOKENS.copy()
    t[0] = 4
    with pytest.raises(dn.JavaArithmeticError):
        dn.diagnostics([NWK0], NK0, ALPHA0, 1.0, 1.0, 0.01, DOC_OFF, t, Z, N)
