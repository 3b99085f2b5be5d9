"""Known answers for the restatement tests/nearest_numpy.py (hand-derived, so that the GPU tests compare against something that is itself
pinned), the pure host function mvhdp_nearest_probe against the same arithmetic in Python, and native.merge_nearest.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, _lib
from mvtopicmodel_amd.native import NearestResult, merge_nearest, merge_topic_top_entities, nearest_probe
from tests import nearest_numpy as nn
from tests import sim_numpy as sn

INF = np.inf


def test_the_selection_is_the_shared_one():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mvtopicmodel_amd", "csrc")
    unit, header = open(os.path.join(csrc, "mvhdp_nearest.hip")).read(), open(os.path.join(csrc, "mvhdp_select.h")).read()
    assert header.count("int wave_first_n(") == 1 and "int wave_first_n(" not in unit      # one copy, in the shared header
    assert unit.count("= wave_first_n(") == 2                                # near_pick_kernel and topk_merge_kernel


def test_orthogonal_and_identical_rows():
    c = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 0.0], [1.0, 1.0]])
    ids, sims, counts = nn.nearest(np.array([[5.0, 0.0]]), c, 4)
    # cos = 1 (rows 0 and 2: identical direction, the id decides), 1/sqrt(2) as the chain gives it, then 0
    assert list(ids[0]) == [0, 2, 3, 1] and counts[0] == 4
    assert sims[0, 0] == 1.0 and sims[0, 1] == 1.0 and sims[0, 3] == 0.0
    assert sims[0, 2] == 5.0 / (5.0 * math.sqrt(2.0))


def test_a_tie_is_resolved_by_id_and_n_may_exceed_the_candidates():
    c = np.array([[0.0, 1.0], [2.0, 0.0], [4.0, 0.0], [1.0, 0.0]])
    ids, sims, counts = nn.nearest(np.array([[1.0, 0.0]]), c, 2)
    assert list(ids[0]) == [1, 2] and list(sims[0]) == [1.0, 1.0] and counts[0] == 2      # three ties at 1.0: the two smallest ids
    ids, sims, counts = nn.nearest(np.array([[1.0, 0.0]]), c, 7, id_base=100)
    assert list(ids[0]) == [101, 102, 103, 100, -1, -1, -1] and counts[0] == 4 and list(sims[0, 3:]) == [0.0] * 4
    # the query itself left out
    ids, _, counts = nn.nearest(c, c, 2, self_index=np.arange(4))
    assert [list(r) for r in ids] == [[1, 2], [2, 3], [1, 3], [1, 2]] and list(counts) == [2, 2, 2, 2]


def test_zero_rows_nan_rows_and_min_weight():
    c = np.array([[0.0, 0.0], [1.0, 0.0], [0.02, 1.0]])
    q = np.array([[0.0, 0.0], [1.0, 0.0], [np.nan, 1.0], [2.0 ** 600, 0.0]])
    ids, sims, counts = nn.nearest(q, c, 3)
    assert list(counts) == [0, 2, 0, 0]                                      # zero query, NaN query, a norm that overflows: nothing
    assert list(ids[1]) == [1, 2, -1]                                        # the zero candidate is never listed
    assert sims[1, 1] == 0.02 / (1.0 * math.sqrt(0.02 * 0.02 + 1.0))
    ids, sims, counts = nn.nearest(q[1:2], c, 3, min_weight=0.03)            # 0.02 counts as 0: the pair is orthogonal
    assert list(ids[0]) == [1, 2, -1] and list(sims[0]) == [1.0, 0.0, 0.0]
    ids, sims, counts = nn.nearest(q[1:2], c, 3, min_weight=1.0)             # every entry emptied: no norm anywhere
    assert counts[0] == 0 and (ids == -1).all()


def test_topic_top_entities_by_hand():
    prop = np.array([[0.5, 0.1], [0.2, 0.1], [0.5, 0.8], [0.3, 0.0]])
    ids, w, counts = nn.topic_top_entities(prop, 3)
    assert [list(r) for r in ids] == [[0, 2, 3], [2, 0, 1]] and [list(r) for r in w] == [[0.5, 0.5, 0.3], [0.8, 0.1, 0.1]]
    ids, w, counts = nn.topic_top_entities(prop, 3, threshold=0.1, id_base=10)       # strictly above
    assert [list(r) for r in ids] == [[10, 12, 13], [12, -1, -1]] and list(counts) == [3, 1] and list(w[1]) == [0.8, 0.0, 0.0]
    assert list(nn.topic_top_entities(prop, 5)[2]) == [4, 4]


@pytest.mark.parametrize("nq,nc,K,bq,sc", [(0, 10, 4, 0, 0), (10, 0, 4, 0, 0), (1, 1, 1, 0, 0), (130, 300, 33, 0, 0), (130, 300, 400, 7, 96),
                                           (129, 257, 100, 128, 128), (65536, 1000000, 400, 0, 0), (70000, 20000, 400, 100000, 9000),
                                           (5, 9000, 2, 1, 1 << 20), (300, 300, 65536, 64, 1)])
def test_probe_geometry_equals_the_python_arithmetic(nq, nc, K, bq, sc):
    st = nearest_probe(nq, nc, K, bq, sc)
    assert st.margin == nn.margin(K) == (K + 4) * 2.0 ** -23
    assert st.blocks == nn.blocks(nq, nc, bq, sc) and st.cells_screened == nn.cells(nq, nc, bq, sc)
    assert (st.candidates, st.exact_only_rows, st.regrown) == (0, 0, 0)


def test_probe_geometry_by_hand_and_error_codes():
    assert nearest_probe(130, 300, 33).cells_screened == 2 * 3 * 128 * 128 and nearest_probe(130, 300, 33).blocks == 1
    st = nearest_probe(130, 300, 33, 7, 96)                                  # 19 blocks of at most 7 queries x 4 stripes: one tile each
    assert st.blocks == 19 and st.cells_screened == 19 * 4 * 128 * 128
    assert nearest_probe(65536, 1000000, 400).blocks == 8
    L = _lib.load_library()
    st = _lib.NearestStatsC()
    assert L.mvhdp_nearest_probe(10, 10, 65537, 0, 0, C.byref(st)) == -6     # MVHDP_ERR_UNSUPPORTED
    for bad in ((-1, 10, 4, 0, 0), (10, -1, 4, 0, 0), (10, 10, 0, 0, 0), (10, 10, 4, -1, 0), (10, 10, 4, 0, -1)):
        assert L.mvhdp_nearest_probe(*bad, C.byref(st)) == -1                # MVHDP_ERR_INVALID_ARG
    assert L.mvhdp_nearest_probe(10, 10, 4, 0, 0, None) == -1
    with pytest.raises(MvhdpError) as e:
        nearest_probe(1, 1, 65537)
    assert e.value.code == -6
    # NULL handles: MVHDP_ERR_INVALID_ARG, no device touched
    assert L.mvhdp_nearest_entities(None, None, None, None, None, None) == -1
    assert L.mvhdp_topic_top_entities(None, None, 0, 0, 1, 0.0, 0, 0, None, None, None) == -1


def test_merge_nearest_over_splits_of_one_result():
    rng = np.random.default_rng(3)
    q = rng.dirichlet(np.full(12, 0.3), 9)
    c = rng.dirichlet(np.full(12, 0.3), 50)
    c[20] = c[4]; c[33] = c[4]; c[41] = 0.0                                  # ties across the splits, a row that is never listed
    for n in (1, 5, 60):
        whole = nn.nearest(q, c, n)
        for cuts in ([0, 50], [0, 25, 50], [0, 5, 21, 34, 50], [0, 0, 50, 50]):
            parts = [NearestResult(*nn.nearest(q, c[a:b], n, id_base=a)) for a, b in zip(cuts[:-1], cuts[1:])]
            got = merge_nearest(parts, n)
            assert np.array_equal(got.ids, whole[0]) and got.sims.tobytes() == whole[1].tobytes() and np.array_equal(got.counts, whole[2])
            assert got.stats is None
            mine = nn.merge([(p.ids, p.sims, p.counts) for p in parts], n)
            assert np.array_equal(mine[0], whole[0]) and mine[1].tobytes() == whole[1].tobytes()
    with pytest.raises(ValueError):
        merge_nearest([NearestResult(*nn.nearest(q, c, 3)), NearestResult(*nn.nearest(q[:4], c, 3))], 3)
    prop = rng.dirichlet(np.full(6, 0.2), 40)
    prop[30] = prop[2]
    for n in (1, 4, 45):
        whole = nn.topic_top_entities(prop, n, 0.01)
        parts = [nn.topic_top_entities(prop[a:b], n, 0.01, id_base=a) for a, b in ((0, 13), (13, 14), (14, 40))]
        got = merge_topic_top_entities(parts, n)
        assert np.array_equal(got[0], whole[0]) and got[1].tobytes() == whole[1].tobytes() and np.array_equal(got[2], whole[2])


def test_the_margin_covers_the_screen_on_the_seeded_rows():
    """The condition of tests/test_gpu_nearest.py's "the screen must screen", on the host: with the fp32 product and sim_margin the
    seeded Dirichlet rows give at most n + 1 candidates per query, and the exact first n lie inside the candidate set."""
    K, C_, nq, n = 100, 300, 16, 5
    x = np.random.default_rng(20261019).dirichlet(np.full(K, 0.1), C_)
    sim, okq, okc = nn.cosine_rect(x[:nq], x)
    scr = nn.screen_f32_rect(x[:nq], x)
    assert np.abs(scr - sim).max() <= nn.margin(K) / 2
    for q in range(nq):
        row = np.delete(scr[q], q)
        tau = np.sort(row)[-n]
        cand = np.flatnonzero(row >= tau - nn.margin(K))
        assert len(cand) <= n + 1
        top = nn.first_n(np.delete(sim[q], q), np.arange(C_ - 1), n)
        assert set(top) <= set(cand)
    assert sn.margin(K) == nn.margin(K)
