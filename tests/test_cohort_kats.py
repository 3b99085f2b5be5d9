"""mvhdp_cohort_top_words without a device: the entry through every layer (header, loader, library export, wrappers, build list,
documents), and the literal restatement of its contract (tests/cohort_numpy.py) against answers worked by hand on a corpus of six
entities, with the properties that tie it to a plain recount."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import cohort_cases as cc
from tests import cohort_numpy as cn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvhdp_cohort_top_words"
ARGS_FIELDS = ["m", "n", "order", "min_count", "scratch_bytes"]
STATS_FIELDS = ["listings", "tokens", "skipped", "passes", "cohorts_per_pass", "kernel_ms"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_entry_exists_in_every_layer():
    hdr = read("include", "mvhdp.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*mvhdp_handle\s+h\s*,\s*const\s+mvhdp_cohort_args\s*\*\s*a\s*,\s*int64_t\s+n_cohorts\s*,\s*const\s+int64_t\s*\*\s*member_off\s*,"
                     r"\s*const\s+int64_t\s*\*\s*members\s*,\s*int32_t\s*\*\s*types\s*,\s*int32_t\s*\*\s*counts\s*,\s*int32_t\s*\*\s*nonzero\s*,"
                     r"\s*int64_t\s*\*\s*tokens\s*,\s*int64_t\s*\*\s*docs\s*,\s*mvhdp_cohort_stats\s*\*\s*stats\s*\)" % NAME, code)
    assert re.search(r"MVHDP_COHORT_BY_COUNT\s*=\s*0\s*,\s*MVHDP_COHORT_BY_SHARE\s*=\s*1\s*\}\s*mvhdp_cohort_order", code)
    for name, fields in (("mvhdp_cohort_args", ARGS_FIELDS), ("mvhdp_cohort_stats", STATS_FIELDS)):
        st = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code)
        assert st and [f.split()[-1].lstrip("*") for f in re.split(r"[;,]", st.group(1)) if f.strip()] == fields, name
    for phrase in ("every listing counts", "0 <= type < V_m and 0 <= z < K", "once per listing", "64-bit cross products", "never by a floating-point quotient",
                   "equal shares by count descending", "IDSorter.compareTo", "2^31 - 1 tokens", "before any device work", "It changes no result",
                   "never an error", "the same bytes", "does not\n *   depend on which other cohorts share the call", "Pending work on the handle's stream lands first",
                   "no count table is needed", "one clear and one scan of a K x V_m int32 table", "(24 bytes)", "(40 bytes)", "untouched on any error"):
        assert phrase in hdr, phrase
    from mvtopicmodel_amd import _lib, native
    assert NAME in _lib.ABI_SYMBOLS
    assert [f[0] for f in _lib.CohortArgsC._fields_] == ARGS_FIELDS and C.sizeof(_lib.CohortArgsC) == 24
    assert [f[0] for f in _lib.CohortStatsC._fields_] == STATS_FIELDS and C.sizeof(_lib.CohortStatsC) == 40
    assert (_lib.COHORT_BY_COUNT, _lib.COHORT_BY_SHARE) == (0, 1)
    L = _lib.load_library()
    assert len(L.mvhdp_cohort_top_words.argtypes) == 11 and L.mvhdp_cohort_top_words.restype is C.c_int
    assert L.mvhdp_cohort_top_words(None, None, 0, None, None, None, None, None, None, None, None) == -1        # a NULL handle: no device touched
    sig = inspect.signature(native.NativeSampler.cohort_top_words).parameters
    assert list(sig) == ["self", "m", "cohorts", "n", "order", "min_count", "trends_only", "scratch_bytes"]
    assert [sig[p].default for p in list(sig)[3:]] == [20, "count", 1, False, 0]
    assert [f for f in native.CohortWords.__dataclass_fields__] == ["types", "counts", "nonzero", "tokens", "docs", "stats"]
    assert [f for f in native.CohortStats.__dataclass_fields__] == STATS_FIELDS
    for method in ("trend", "words"):
        assert "host derivation" in getattr(native.CohortWords, method).__doc__.lower(), method
    make = read("mvtopicmodel_amd", "csrc", "Makefile")
    assert "mvhdp_cohort.hip" in re.search(r"^SRCS\s*=(.*)$", make, flags=re.M).group(1)
    assert os.path.exists(os.path.join(ROOT, "mvtopicmodel_amd", "csrc", "mvhdp_cohort.hip"))
    diag = read("mvtopicmodel_amd", "csrc", "mvhdp_diag.hip")
    assert "void topn_offer" not in diag and "void topn_offer" in read("mvtopicmodel_amd", "csrc", "mvhdp_select.h")     # one copy, in the shared header
    assert "void topn_offer" not in read("mvtopicmodel_amd", "csrc", "mvhdp_cohort.hip")
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "CHANGELOG.md"):
        assert NAME in read(doc), doc
    assert "7j" in read("DESIGN.md") and "FLOW:807-1083" in read("INTEGRATION.md") and "cohort_top_words(" in read("INTEGRATION.md")
    log = read("CHANGELOG.md")
    for not_done in ("a JNI class", "mvhdp_group_", "NativeGroup", "sparse (hashed) form", "phrases per cohort", "weighted listings"):
        assert not_done in log, not_done


# ---- the hand-sized corpus: tests/cohort_cases.py HAND_*; every answer below is worked out by hand from the lists there ----
K = cc.HAND_K
A, B, NONE, ABSENT, E, ALL = [0], [2, 2], [], [3], [1, 4], [0, 1, 2, 3, 4, 5]
COHORTS = [A, B, NONE, ABSENT, E, ALL]


@pytest.fixture(scope="module")
def hand():
    off, tok, z = cc.hand_view(cc.HAND_DOCS0)
    nwk, nk = cn.recount(K, cc.HAND_V[0], tok, z)
    return off, tok, z, nwk, nk, cn.count(K, cc.HAND_V[0], off, tok, z, COHORTS)


def lists(types, counts, g, k):
    return [(int(t), int(c)) for t, c in zip(types[g, k], counts[g, k])]


def test_the_restatement_equals_the_answers_worked_by_hand(hand):
    off, tok, z, nwk, nk, cd = hand
    # the whole corpus, counted tokens only: topic 0 {0: 4, 1: 2, 3: 1, 4: 3}, topic 1 {1: 2, 2: 3, 3: 1, 4: 1}, topic 2 {0: 1, 5: 3}
    assert nwk.tolist() == [[4, 0, 1], [2, 2, 0], [0, 3, 0], [1, 1, 0], [3, 1, 0], [0, 0, 3]] and nk.tolist() == [10, 7, 4]
    assert cd.tokens.tolist() == [[3, 1, 1], [2, 4, 4], [0, 0, 0], [0, 0, 0], [5, 2, 0], [10, 7, 4]]
    assert cd.docs.tolist() == [[1, 1, 1], [2, 2, 2], [0, 0, 0], [0, 0, 0], [2, 1, 0], [5, 4, 3]]
    assert cd.nonzero.tolist() == [[2, 1, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0], [4, 2, 0], [4, 4, 2]]
    assert cd.skipped == 4 + 4 and cd.counted == 5 + 10 + 7 + 21          # entities 1 and 4 hold two skipped tokens each, listed in E and in ALL
    t, c = cn.select(cd, 2, cn.BY_COUNT)
    assert lists(t, c, 0, 0) == [(0, 2), (1, 1)] and lists(t, c, 0, 1) == [(2, 1), (-1, 0)]
    assert lists(t, c, 1, 0) == [(4, 2), (-1, 0)] and lists(t, c, 1, 1) == [(2, 4), (-1, 0)] and lists(t, c, 1, 2) == [(5, 4), (-1, 0)]     # the repeated listing counts twice
    for g in (2, 3):                                                         # the empty cohort, the entity without the view
        assert (t[g] == -1).all() and not c[g].any()
    assert lists(t, c, 4, 0) == [(0, 2), (4, 1)]                             # types 1, 3 and 4 tie at count 1 across the cut: the largest type id
    assert lists(t, c, 4, 1) == [(3, 1), (1, 1)] and lists(t, c, 4, 2) == [(-1, 0), (-1, 0)]               # (9, 2) is out of the vocabulary
    # min_count at the boundary: 2 keeps the count of 2, 3 keeps nothing; nonzero does not move
    t2, c2 = cn.select(cd, 2, cn.BY_COUNT, min_count=2)
    assert lists(t2, c2, 4, 0) == [(0, 2), (-1, 0)] and lists(t2, c2, 0, 0) == [(0, 2), (-1, 0)] and lists(t2, c2, 4, 1) == [(-1, 0), (-1, 0)]
    t3, c3 = cn.select(cd, 2, cn.BY_COUNT, min_count=3)
    assert (t3[4] == -1).all() and lists(t3, c3, 1, 1) == [(2, 4), (-1, 0)]
    # by share, cohort E, topic 0: 1/1 (type 3), then 2/4 against 1/2 -- equal, the larger count first --, then 1/3 (type 4)
    ts, cs = cn.select(cd, 4, cn.BY_SHARE, nwk=nwk)
    assert lists(ts, cs, 4, 0) == [(3, 1), (0, 2), (1, 1), (4, 1)]
    assert lists(ts, cs, 0, 0) == [(0, 2), (1, 1), (-1, 0), (-1, 0)]         # cohort A: 2/4 against 1/2 again, where the type id alone would say (1, 0)
    assert lists(ts, cs, 4, 1) == [(3, 1), (1, 1), (-1, 0), (-1, 0)]         # 1/1, 1/2
    assert lists(ts, cs, 1, 1) == [(2, 4), (-1, 0), (-1, 0), (-1, 0)]        # a share above 1: the repeated listing
    assert lists(ts, cs, 5, 0) == [(0, 4), (4, 3), (1, 2), (3, 1)]           # every entity once: all shares are 1, so by count
    ts2, cs2 = cn.select(cd, 4, cn.BY_SHARE, min_count=2, nwk=nwk)
    assert lists(ts2, cs2, 4, 0) == [(0, 2), (-1, 0), (-1, 0), (-1, 0)]
    # view 1, cohort {2, 5}
    off1, tok1, z1 = cc.hand_view(cc.HAND_DOCS1)
    t1, c1, nz1, tk1, dc1, cd1 = cn.cohort_top_words(K, cc.HAND_V[1], off1, tok1, z1, [[2, 5]], n=2)
    assert lists(t1, c1, 0, 0) == [(2, 1), (0, 1)] and lists(t1, c1, 0, 1) == [(1, 2), (-1, 0)]
    assert tk1.tolist() == [[2, 2, 0]] and dc1.tolist() == [[1, 1, 0]] and nz1.tolist() == [[2, 1, 0]] and cd1.skipped == 0


def test_a_bad_token_is_an_error_only_where_it_is_listed():
    off, tok, z = cc.hand_view(cc.HAND_DOCS0)
    for bad_tok, bad_z in ((-1, 0), (0, K), (0, -2)):
        t, zz = tok.copy(), z.copy()
        t[0], zz[0] = bad_tok, bad_z                                         # entity 0
        with pytest.raises(cn.StateError):
            cn.count(K, cc.HAND_V[0], off, t, zz, [[1], [0]])
        cn.count(K, cc.HAND_V[0], off, t, zz, [[1], [2, 5]])


def test_the_cohort_of_every_entity_is_a_plain_recount(hand):
    off, tok, z, nwk, nk, cd = hand
    assert np.array_equal(cd.c[5], nwk) and np.array_equal(cd.tokens[5], nk)
    for n in (1, 2, 6):
        t, c = cn.select(cd, n, cn.BY_COUNT)
        wt, wc, wnz = cn.top_words(nwk, n)
        assert np.array_equal(t[5], wt) and np.array_equal(c[5], wc) and np.array_equal(cd.nonzero[5], wnz)
    c3 = cc.make(5, [65, 64, 5], seed=3)
    for m in (0, 1):
        whole = cn.count(c3.K, c3.V[m], c3.doc_off[m], c3.tokens[m], c3.z[m], [list(range(c3.D))])
        nwk3, nk3 = cn.recount(c3.K, c3.V[m], c3.tokens[m], c3.z[m])
        assert np.array_equal(whole.c[0], nwk3) and np.array_equal(whole.tokens[0], nk3)
        t, c = cn.select(whole, 20)
        wt, wc, wnz = cn.top_words(nwk3, 20)
        assert np.array_equal(t[0], wt) and np.array_equal(c[0], wc) and np.array_equal(whole.nonzero[0], wnz)
        assert whole.skipped == 8                                            # the holes of tests/cohort_cases.py


def test_cohort_order_and_disjoint_unions():
    c = cc.make(5, [65, 64, 5], seed=4)
    m = 0
    co = cc.cohorts(c)
    nwk, _ = cn.recount(c.K, c.V[m], c.tokens[m], c.z[m])
    view = (c.K, c.V[m], c.doc_off[m], c.tokens[m], c.z[m])
    fwd = cn.count(*view, co)
    back = cn.count(*view, co[::-1])
    assert np.array_equal(fwd.c, back.c[::-1]) and np.array_equal(fwd.docs, back.docs[::-1]) and fwd.skipped == back.skipped
    for order in (cn.BY_COUNT, cn.BY_SHARE):
        a, b = cn.select(fwd, 20, order, 2, nwk), cn.select(back, 20, order, 2, nwk)
        assert np.array_equal(a[0], b[0][::-1]) and np.array_equal(a[1], b[1][::-1])
        alone = cn.select(cn.count(*view, [co[4]]), 20, order, 2, nwk)
        assert np.array_equal(alone[0][0], a[0][4]) and np.array_equal(alone[1][0], a[1][4])
    # a union of disjoint cohorts adds tokens, docs and the cells
    x, y = list(range(0, 11)), list(range(11, c.D))
    parts = cn.count(*view, [x, y, x + y])
    assert np.array_equal(parts.c[0] + parts.c[1], parts.c[2]) and np.array_equal(parts.tokens[0] + parts.tokens[1], parts.tokens[2])
    assert np.array_equal(parts.docs[0] + parts.docs[1], parts.docs[2])


def test_the_host_derivations():
    from mvtopicmodel_amd.native import CohortWords
    off, tok, z = cc.hand_view(cc.HAND_DOCS0)
    types, counts, nz, tokens, docs, _ = cn.cohort_top_words(K, cc.HAND_V[0], off, tok, z, COHORTS, n=2)
    w = CohortWords(types, counts, nz, tokens, docs)
    tr = w.trend()
    assert tr.shape == (6, 3) and np.allclose(tr[0], [0.6, 0.2, 0.2]) and not tr[2].any() and np.allclose(tr[[0, 1, 4, 5]].sum(1), 1.0)
    assert w.words(4, 0) == [(0, 2), (4, 1)] and w.words(2, 0) == [] and w.words(0, 1, vocabulary="abcdef") == [("c", 1)]
    with pytest.raises(ValueError):
        CohortWords(None, None, None, tokens, docs).words(0, 0)
