"""mvhdp_predict_entities / mvhdp_rank_entities without a device: the entries through every layer (header, loader, library export, wrappers,
build list, documents), and the sequential restatement of their contract (tests/native/xview_entities_ref.c) against exact rationals on a
hand-sized model, against xview_ref's scores transposed, against worked cases, and the host merge against the unsplit result."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np

from tests import xview_cases as xc
from tests import xview_entities_cases as ec
from tests import xview_entities_ref as er
from tests import xview_ref as xr
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mvhdp_predict_entities", "mvhdp_rank_entities")
ARGS_FIELDS = ["m", "exclude_present", "view_weights", "c0", "c1", "nq", "q_off", "q_items", "q_weights", "psi", "block_entities", "block_queries"]
STATS_FIELDS = ["cells", "excluded", "blocks", "kernel_ms"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_entries_exist_in_every_layer():
    hdr = read("include", "mvhdp.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*mvhdp_handle\s+h\s*,\s*const\s+mvhdp_entities_args\s*\*" % n, code), n
    for name, fields in (("mvhdp_entities_args", ARGS_FIELDS), ("mvhdp_entities_stats", STATS_FIELDS)):
        st = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code)
        assert st and [f.split()[-1].lstrip("*") for f in re.split(r"[;,]", st.group(1)) if f.strip()] == fields, name
    for phrase in ("xview_entities_ref.c", "fma(c_i, phi[w_i][k], p)", "fma(theta_d[k], psi_j[k], s)", "equal scores by ascending entity id",
                   "(88 bytes)", "(32 bytes", "n_pairs x (c1 - c0) comparisons"):
        assert phrase in hdr, phrase
    from mvtopicmodel_amd import _lib, native
    for n in NAMES:
        assert n in _lib.ABI_SYMBOLS
    assert [f[0] for f in _lib.EntitiesArgsC._fields_] == ARGS_FIELDS and C.sizeof(_lib.EntitiesArgsC) == 88
    assert [f[0] for f in _lib.EntitiesStatsC._fields_] == STATS_FIELDS and C.sizeof(_lib.EntitiesStatsC) == 32
    L = _lib.load_library()
    assert len(L.mvhdp_predict_entities.argtypes) == 7 and len(L.mvhdp_rank_entities.argtypes) == 7
    assert L.mvhdp_predict_entities.restype is C.c_int and L.mvhdp_rank_entities.restype is C.c_int
    assert L.mvhdp_predict_entities(None, None, 1, None, None, None, None) == -1         # a NULL handle: no device touched
    assert L.mvhdp_rank_entities(None, None, 0, None, None, None, None) == -1
    sig = inspect.signature(native.NativeSampler.predict_entities).parameters
    assert list(sig) == ["self", "m", "view_weights", "n", "items", "weights", "psi", "c0", "c1", "exclude_present", "block_entities", "block_queries"]
    assert sig["exclude_present"].default is True and sig["c1"].default is None
    assert list(inspect.signature(native.NativeSampler.rank_entities).parameters)[:5] == ["self", "m", "view_weights", "queries", "entities"]
    assert list(inspect.signature(native.NativeGroup.predict_entities).parameters)[:7] == ["self", "m", "view_weights", "n", "items", "weights", "psi"]
    assert not hasattr(native.NativeGroup, "rank_entities")
    assert [f for f in native.EntityRanking.__dataclass_fields__] == ["ids", "scores", "counts", "stats"]
    srcs = re.search(r"^SRCS\s*=(.*)$", read("mvtopicmodel_amd", "csrc", "Makefile"), flags=re.M).group(1)
    assert "mvhdp_xview_entities.hip" in srcs and "mvhdp_xview.h" in read("mvtopicmodel_amd", "csrc", "Makefile")
    unit = read("mvtopicmodel_amd", "csrc", "mvhdp_xview_entities.hip")
    assert "key_descent(" not in unit and "wave_first_n(" in unit and "XE_EXCLUDED" not in unit      # the selection: one copy, in the shared header
    assert read("mvtopicmodel_amd", "csrc", "mvhdp_select.h").count("int wave_first_n(") == 1 and "int wave_first_n(" not in unit
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "CHANGELOG.md"):
        for n in NAMES:
            assert n in read(doc), (doc, n)
    assert "predict_entities(" in read("INTEGRATION.md") and "7h" in read("DESIGN.md")
    log = read("CHANGELOG.md")
    for not_done in ("a JNI class", "mvhdp_group_", "rank_entities on a group", "vectors mix", "theta rows supplied by the host", "approximate retrieval"):
        assert not_done in log, not_done


# ---- the hand-sized model: K = 3, V = 4, D = 5 ----
NWK = np.array([[3, 0, 1], [0, 2, 2], [1, 1, 0], [0, 0, 5]], dtype=np.int32)
NK = NWK.sum(0).astype(np.int32)
BETA, BETA_SUM = 0.01, 0.04
THETA = np.array([[0.7, 0.2, 0.1], [0.1, 0.1, 0.8], [1 / 3, 1 / 3, 1 / 3], [0.1, 0.1, 0.8], [0.05, 0.9, 0.05]])
DOC_OFF = np.array([0, 2, 3, 3, 5, 6], dtype=np.int64)
TOK = np.array([0, 2, 3, 3, 1, 1], dtype=np.int32)                          # entity 0: {0, 2}; 1: {3}; 2: none; 3: {3, 1}; 4: {1}


def rfma(a, b, c):
    """the correctly rounded a * b + c, by exact rationals"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def exact_psi(items, weights, inactive=None):
    out = np.zeros((len(items), 3))
    for j, (q, ws) in enumerate(zip(items, weights)):
        for k in range(3):
            p = 0.0
            for w, cw in zip(q, ws):
                phi = 0.0 if inactive is not None and inactive[k] else float(Fraction(float(NWK[w, k]) + BETA) / Fraction(float(NK[k]) + BETA_SUM))
                p = rfma(cw, phi, p)
            out[j, k] = p
    return out


def exact_scores(psi):
    out = np.zeros((len(psi), len(THETA)))
    for j in range(len(psi)):
        for d in range(len(THETA)):
            s = 0.0
            for k in range(3):
                s = rfma(THETA[d, k], psi[j, k], s)
            out[j, d] = s
    return out


ITEMS = [[0], [3, 1], [2, 2, 0], [], [1, 3]]
WEIGHTS = [[1.0], [0.5, 3.0], [1.0, 0.3, 2.0], [], [0.0, 1.0]]


def test_the_restatement_equals_exact_rationals_on_the_hand_sized_model():
    for inactive in (None, np.array([0, 1, 0], dtype=np.uint8)):
        psi = er.psi_rows(NWK, NK, BETA, BETA_SUM, inactive, ITEMS, WEIGHTS)
        want = exact_psi(ITEMS, WEIGHTS, inactive)
        assert np.array_equal(bits(psi), bits(want))
        S = er.scores(THETA, psi)
        assert np.array_equal(bits(S), bits(exact_scores(want)))
        if inactive is not None:
            assert (psi[:, 1] == 0.0).all()
    psi = er.psi_rows(NWK, NK, BETA, BETA_SUM, None, ITEMS, WEIGHTS)
    phi = xr.phi_table(NWK, NK, BETA, BETA_SUM)
    assert np.array_equal(bits(psi[0]), bits(phi[0]))                        # one item of weight 1.0: the bits of phi[w]
    assert np.array_equal(bits(psi[4]), bits(phi[3]))                        # a weight of 0 adds nothing
    assert (psi[3] == 0.0).all() and not np.signbit(psi[3]).any()            # the empty query: +0.0
    unweighted = er.psi_rows(NWK, NK, BETA, BETA_SUM, None, [[2, 2, 0]])     # without weights every weight is 1.0
    assert np.array_equal(bits(unweighted), bits(exact_psi([[2, 2, 0]], [[1.0, 1.0, 1.0]])))
    assert (unweighted[0] > phi[2] + phi[0]).all()                           # the repeated item added twice


def test_worked_cases_order_ties_exclusion_and_ranks():
    psi = er.psi_rows(NWK, NK, BETA, BETA_SUM, None, ITEMS, WEIGHTS)
    S = er.scores(THETA, psi)
    assert np.array_equal(bits(S[:, 1]), bits(S[:, 3]))                      # entities 1 and 3: equal theta rows, a tie for every query
    ex = er.excluded(DOC_OFF, TOK, ITEMS)
    assert ex.tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 1, 1], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 1, 0, 1, 1]]
    ids, sc, counts = er.predict(S, 7, None, id0=100)
    assert counts.tolist() == [5] * 5 and (ids[:, 5:] == -1).all() and (sc[:, 5:] == 0.0).all()
    for j in range(5):
        order = sorted(range(5), key=lambda d: (-S[j, d], d))
        assert ids[j, :5].tolist() == [100 + d for d in order] and np.array_equal(bits(sc[j, :5]), bits(S[j, order]))
        if j != 3:
            assert ids[j, :5].tolist().index(101) + 1 == ids[j, :5].tolist().index(103)  # the tie: by id, side by side
    assert ids[3, :5].tolist() == [100, 101, 102, 103, 104]                  # the empty query scores 0.0 everywhere: by id alone
    ids, sc, counts = er.predict(S, 2, ex)
    assert counts.tolist() == [2, 2, 2, 2, 2]
    assert 0 not in ids[0] and not set(ids[1]) & {1, 3, 4}
    # exclusion that removes every candidate: the candidates {1, 3, 4} all hold an item of query 1
    ids, sc, counts = er.predict(S[:, [1, 3, 4]], 3, ex[:, [1, 3, 4]], id0=0)
    assert counts[1] == 0 and (ids[1] == -1).all() and (sc[1] == 0.0).all() and counts[0] == 3
    # ranks: 0-based, the queried entity apart; an excluded queried entity is still scored and ranked among the others
    q = np.array([0, 1, 1, 3, 3], dtype=np.int64)
    e = np.array([0, 3, 1, 3, 1], dtype=np.int64)
    score, rk = er.rank(S, q, e, ex)
    assert np.array_equal(bits(score), bits(S[q, e]))
    for i in range(5):
        want = sum(1 for d in range(5) if d != e[i] and not ex[q[i], d] and (S[q[i], d] > S[q[i], e[i]] or (S[q[i], d] == S[q[i], e[i]] and d < e[i])))
        assert rk[i] == want
    assert ex[0, 0] == 1 and ex[1, 3] == 1                                   # pairs 0 and 1 query an excluded entity
    assert rk[3] == 3 and rk[4] == 1                                         # the empty query scores 0.0 everywhere: the smaller ids precede
    _, plain = er.rank(S, q, e, None)
    for i in range(5):                                                       # without exclusion: the excluded ones that precede come back
        assert plain[i] - rk[i] == sum(1 for d in range(5) if d != e[i] and ex[q[i], d] and (S[q[i], d] > S[q[i], e[i]] or (S[q[i], d] == S[q[i], e[i]] and d < e[i])))
    assert plain[1] == rk[1] + 1 + int(S[1, 4] > S[1, 3])                    # pair (1, 3): its twin 1 precedes it by id once nothing is excluded


def test_one_item_queries_are_xview_ref_scores_transposed():
    for shape in ((5, 3, 65, 3), (64, 127, 300, 3), (17, 129, 65, 1)):
        c = xc.make(*shape)
        nwk, nk = c.counts(c.m)
        theta = c.theta()
        V = c.V[c.m]
        phi = xr.phi_table(nwk, nk, c.hy.beta[c.m], c.hy.beta_sum[c.m], c.hy.inactive)
        psi = er.psi_rows(nwk, nk, c.hy.beta[c.m], c.hy.beta_sum[c.m], c.hy.inactive, np.arange(V, dtype=np.int32))
        assert np.array_equal(bits(psi), bits(phi))
        assert np.array_equal(bits(er.scores(theta, psi)), bits(xr.scores(theta, phi).T.copy()))
        # ... and the two rankings hold the same score for every (d, w)
        S = er.scores(theta, psi)
        ids, sc, counts = er.predict(S, c.D)
        items, sc2, _ = xr.predict(S.T.copy(), V)
        back = np.zeros_like(S); back[np.arange(V)[:, None], ids] = sc
        back2 = np.zeros_like(S); back2[items.T, np.arange(c.D)[None, :]] = sc2.T
        assert np.array_equal(bits(back), bits(S)) and np.array_equal(bits(back2), bits(S))


def test_merge_of_split_inputs_equals_the_unsplit_result():
    from mvtopicmodel_amd.native import EntityRanking, merge_predicted_entities
    c = ec.make(16)
    nwk, nk = c.counts(c.m)
    theta = c.theta()
    theta[40:80] = theta[40]                                                 # equal rows across both cuts: ties the merge must order by id
    items, weights = ec.queries(c, 33)
    psi = er.psi_rows(nwk, nk, c.hy.beta[c.m], c.hy.beta_sum[c.m], c.hy.inactive, items, weights)
    S = er.scores(theta, psi)
    ex = er.excluded(c.doc_off[c.m], c.tokens[c.m], items)
    for n in (1, 20, 45, c.D + 3):
        whole = er.predict(S, n, ex)
        cuts = [0, 50, 61, c.D]
        parts = [EntityRanking(*er.predict(S[:, a:b], n, ex[:, a:b], id0=a)) for a, b in zip(cuts, cuts[1:])]
        got = merge_predicted_entities(parts, n)
        assert np.array_equal(got.ids, whole[0]) and np.array_equal(bits(got.scores), bits(whole[1])) and np.array_equal(got.counts, whole[2])
        assert got.ids.dtype == np.int64 and got.counts.dtype == np.int32
