"""mvhdp_word_cooccurrence without a device: the entry through every layer (header, loader, library export, wrappers, build list), the
literal restatement of its contract (tests/cooc_numpy.py) against counts worked by hand on a corpus of five entities, the host measures
against the formulas evaluated with math.log, and the identities that tie the windows to each other."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from tests import cohort_cases as cc
from tests import cooc_cases as kc
from tests import cooc_numpy as kn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvhdp_word_cooccurrence"
ARGS_FIELDS = ["m", "n", "window", "d0", "d1"]
STATS_FIELDS = ["entities", "tokens", "hits", "oov", "distinct_words", "memberships", "kernel_ms"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_entry_exists_in_every_layer():
    hdr = read("include", "mvhdp.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*mvhdp_handle\s+h\s*,\s*const\s+mvhdp_cooc_args\s*\*\s*a\s*,\s*int64_t\s+n_sets\s*,\s*const\s+int32_t\s*\*\s*sets\s*,"
                     r"\s*int64_t\s+num_docs\s*,\s*const\s+int64_t\s*\*\s*doc_off\s*,\s*const\s+int32_t\s*\*\s*tokens\s*,\s*int64_t\s*\*\s*co\s*,"
                     r"\s*int64_t\s*\*\s*windows\s*,\s*mvhdp_cooc_stats\s*\*\s*stats\s*\)" % NAME, code)
    for name, fields in (("mvhdp_cooc_args", ARGS_FIELDS), ("mvhdp_cooc_stats", STATS_FIELDS)):
        st = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code)
        assert st and [f.split()[-1].lstrip("*") for f in re.split(r"[;,]", st.group(1)) if f.strip()] == fields, name
    for phrase in ("every such slot counts", "z is never read", "matches no slot", "L - W + 1", "[i, min(i + W, L))", "never exceeds *windows",
                   "the same bytes", "additive over disjoint entity ranges", "a window never crosses an\n *   entity", "Pending work on the handle's stream lands first",
                   "staged and copied out\n *   once", "(32 bytes)", "(48 bytes)", "untouched on any error", "2^26 cells", "The formulas stay on the host"):
        assert phrase in hdr, phrase
    from mvtopicmodel_amd import _lib, native
    assert NAME in _lib.ABI_SYMBOLS
    assert [f[0] for f in _lib.CoocArgsC._fields_] == ARGS_FIELDS and C.sizeof(_lib.CoocArgsC) == 32
    assert (_lib.CoocArgsC.window.offset, _lib.CoocArgsC.d0.offset, _lib.CoocArgsC.d1.offset) == (8, 16, 24)
    assert [f[0] for f in _lib.CoocStatsC._fields_] == STATS_FIELDS and C.sizeof(_lib.CoocStatsC) == 48
    assert (_lib.CoocStatsC.distinct_words.offset, _lib.CoocStatsC.memberships.offset, _lib.CoocStatsC.kernel_ms.offset) == (32, 36, 40)
    L = _lib.load_library()
    assert len(L.mvhdp_word_cooccurrence.argtypes) == 10 and L.mvhdp_word_cooccurrence.restype is C.c_int
    assert L.mvhdp_word_cooccurrence(None, None, 0, None, 0, None, None, None, None, None) == -1             # a NULL handle: no device touched
    sig = inspect.signature(native.NativeSampler.word_cooccurrence).parameters
    assert list(sig) == ["self", "sets", "m", "window", "d0", "d1", "corpus"]
    assert [sig[p].default for p in list(sig)[2:]] == [0, 0, 0, None, None]
    assert list(inspect.signature(native.NativeGroup.word_cooccurrence).parameters) == list(sig)
    sig = inspect.signature(native.NativeSampler.topic_coherence).parameters
    assert list(sig) == ["self", "n", "m", "window", "measure", "corpus"] and [sig[p].default for p in list(sig)[1:]] == [20, 0, 0, "npmi", None]
    assert [f for f in native.WordCooccurrence.__dataclass_fields__] == ["co", "windows", "sets", "stats"]
    assert [f for f in native.CoocStats.__dataclass_fields__] == STATS_FIELDS
    for method in ("occurrences", "pair_scores", "coherence"):
        assert "host derivation" in getattr(native.WordCooccurrence, method).__doc__.lower(), method
    assert "no equality with any toolkit" in native.WordCooccurrence.__doc__
    make = read("mvtopicmodel_amd", "csrc", "Makefile")
    assert "mvhdp_cooc.hip" in re.search(r"^SRCS\s*=(.*)$", make, flags=re.M).group(1)
    src = read("mvtopicmodel_amd", "csrc", "mvhdp_cooc.hip")
    assert '#include "mvhdp_side.h"' in src and '#include "mvhdp_select.h"' in src and "DevArray<" in src
    kernel = src[src.index("__global__"):src.index("// the corpus of a call")]
    assert not re.search(r"\b(double|float)\b", kernel)                                      # no floating point on the device


# ---- the hand-sized corpus: every count below was worked out on paper from kc.HAND_DOCS ----
HAND = {   # window: (windows, co of the sets [0, 1, -], [2, 3, 5], [0, -, 0])
    0: (4, [[[3, 3, 0], [3, 3, 0], [0, 0, 0]], [[2, 1, 0], [1, 2, 0], [0, 0, 0]], [[3, 0, 3], [0, 0, 0], [3, 0, 3]]]),
    1: (15, [[[4, 0, 0], [0, 4, 0], [0, 0, 0]], [[3, 0, 0], [0, 2, 0], [0, 0, 0]], [[4, 0, 4], [0, 0, 0], [4, 0, 4]]]),
    2: (12, [[[4, 1, 0], [1, 5, 0], [0, 0, 0]], [[5, 1, 0], [1, 4, 0], [0, 0, 0]], [[4, 0, 4], [0, 0, 0], [4, 0, 4]]]),
    3: (9, [[[4, 3, 0], [3, 5, 0], [0, 0, 0]], [[5, 2, 0], [2, 5, 0], [0, 0, 0]], [[4, 0, 4], [0, 0, 0], [4, 0, 4]]]),
    4: (7, [[[4, 3, 0], [3, 4, 0], [0, 0, 0]], [[5, 3, 0], [3, 4, 0], [0, 0, 0]], [[4, 0, 4], [0, 0, 0], [4, 0, 4]]]),
}


def test_the_hand_corpus_has_what_it_is_for():
    lens = [len(d) for d in kc.HAND_DOCS]
    assert lens == [0, 1, 3, 4, 7] and sum(t >= kc.HAND_V for d in kc.HAND_DOCS for t in d) == 1
    assert kc.HAND_DOCS[3][:2] == [1, 1] and kc.HAND_DOCS[4][0] == kc.HAND_DOCS[4][-1]       # a repeat inside a window of two; both ends


@pytest.mark.parametrize("window", sorted(HAND))
def test_the_restatement_gives_the_hand_counts(window):
    off, tok = kc.hand_corpus()
    r = kn.cooc(kc.HAND_V, off, tok, kc.HAND_SETS, window)
    windows, co = HAND[window]
    assert r.windows == windows and r.co.tolist() == co
    assert (r.entities, r.tokens, r.hits, r.oov, r.distinct_words, r.memberships) == (4, 15, 13, 1, 5, 7)


def test_a_negative_type_is_refused_by_the_restatement():
    off, tok = kc.hand_corpus()
    tok = tok.copy()
    tok[2] = -1
    with pytest.raises(kn.NegativeType):
        kn.cooc(kc.HAND_V, off, tok, kc.HAND_SETS, 0)
    assert kn.cooc(kc.HAND_V, off, tok, kc.HAND_SETS, 0, 3, 5).windows == 2                  # ... only where it is read


def close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * abs(b)


@pytest.mark.parametrize("window", sorted(HAND))
def test_the_measures_are_the_formulas(window):
    """pair_scores and coherence on the hand counts against the formulas of the contract evaluated here with math.log, to a relative 1e-12:
    a handful of roundings of 2^-53 over at most 3 pairs, with three orders of magnitude to spare.  NaN sits exactly where the contract
    puts it: an empty slot, a slot that never occurs, and for umass everything but j < i."""
    from mvtopicmodel_amd.native import WordCooccurrence
    windows, co = HAND[window]
    sets = np.array(kc.HAND_SETS)
    wc = WordCooccurrence(np.array(co, dtype=np.int64), windows, sets)
    assert wc.occurrences().tolist() == [[row[i][i] for i in range(3)] for row in co]
    eps = 1e-12
    for measure in ("uci", "npmi", "umass"):
        got = wc.pair_scores(measure)
        want_sets = []
        for s in range(3):
            vals = []
            for i in range(3):
                for j in range(3):
                    ok = sets[s][i] >= 0 and sets[s][j] >= 0 and co[s][i][i] > 0 and co[s][j][j] > 0
                    if measure == "umass":
                        ok = ok and j < i
                    want = float("nan")
                    if ok:
                        pi, pj, pij = co[s][i][i] / windows, co[s][j][j] / windows, co[s][i][j] / windows
                        if measure == "umass":
                            want = math.log((pij + eps) / pj)
                        else:
                            want = math.log((pij + eps) / (pi * pj))
                            if measure == "npmi":
                                want = want / -math.log(pij + eps)
                    assert close(float(got[s, i, j]), want), (measure, s, i, j, got[s, i, j], want)
                    if j < i and ok:
                        vals.append(want)
            want_sets.append(vals)
        for agg in ("mean", "sum"):
            coh = wc.coherence(measure, agg)
            for s in range(3):
                want = float("nan") if not want_sets[s] else (sum(want_sets[s]) / len(want_sets[s]) if agg == "mean" else sum(want_sets[s]))
                assert close(float(coh[s]), want), (measure, agg, s, coh[s], want)
    assert np.isnan(got[0, 2]).all() and np.isnan(got[1, 2]).all() and np.isnan(got[2, 1]).all() and np.isnan(got[:, 0, :]).all()
    lonely = WordCooccurrence(np.array([[[3, 0], [0, 0]], [[0, 0], [0, 0]]], dtype=np.int64), 5, np.array([[1, 2], [-1, -1]]))
    assert np.isnan(lonely.coherence("npmi")).all() and np.isnan(lonely.coherence("umass", "sum")).all()
    with pytest.raises(ValueError):
        wc.pair_scores("c_v")
    with pytest.raises(ValueError):
        wc.coherence("uci", "median")


def test_merge_sums_and_refuses_other_sets():
    from mvtopicmodel_amd.native import CoocStats, WordCooccurrence, merge_word_cooccurrence
    off, tok = kc.hand_corpus()
    sets = np.array(kc.HAND_SETS, dtype=np.int32)

    def part(d0, d1, s=sets):
        r = kn.cooc(kc.HAND_V, off, tok, s, 2, d0, d1)
        return WordCooccurrence(r.co, r.windows, s, CoocStats(r.entities, r.tokens, r.hits, r.oov, r.distinct_words, r.memberships, 1.0))
    whole, merged = part(0, 5), merge_word_cooccurrence([part(0, 3), part(3, 4), part(4, 5)])
    assert np.array_equal(merged.co, whole.co) and merged.windows == whole.windows == 12 and merged.co.dtype == np.int64
    assert (merged.stats.entities, merged.stats.tokens, merged.stats.hits, merged.stats.oov, merged.stats.distinct_words, merged.stats.memberships) == (4, 15, 13, 1, 5, 7)
    other = sets.copy()
    other[0, 0] = 4
    with pytest.raises(ValueError):
        merge_word_cooccurrence([part(0, 3), part(3, 5, other)])
    from mvtopicmodel_amd.native import _word_sets
    assert _word_sets([[1, 2, 3], [4], []]).tolist() == [[1, 2, 3], [4, -1, -1], [-1, -1, -1]]


@pytest.mark.parametrize("K,V", [(5, [64, 64, 5]), (400, [5, 64, 5])])
def test_identities_of_the_restatement(K, V):
    c = cc.make(K, V)
    off, tok, Vm = c.doc_off[0], c.tokens[0], V[0]
    n = min(6, Vm)
    sets, hot, _ = kc.special_sets(c, 0, n)
    longest = int(np.diff(off).max())
    doc = kn.cooc(Vm, off, tok, sets, 0)
    for w in (longest, longest + 1, 2 ** 31 - 1):
        r = kn.cooc(Vm, off, tok, sets, w)
        assert r.windows == doc.windows == int((np.diff(off) > 0).sum()) and np.array_equal(r.co, doc.co), w
    one = kn.cooc(Vm, off, tok, sets, 1)
    freq = kc.frequencies(c, 0)
    assert one.windows == len(tok) == one.tokens
    for s in range(len(sets)):
        for i in range(n):
            for j in range(n):
                same = sets[s, i] >= 0 and sets[s, i] == sets[s, j]
                assert one.co[s, i, j] == (freq[sets[s, i]] if same else 0), (s, i, j)
    assert one.co[3, 0, n - 1] == freq[hot] > 0                                              # the same word in two slots of a row
    ten = kn.cooc(Vm, off, tok, sets, 10)
    assert not np.array_equal(ten.co, doc.co) and ten.windows > doc.windows                  # window 0 and window 10 differ
    for r in (doc, one, ten):
        assert np.array_equal(r.co, r.co.transpose(0, 2, 1)) and (r.co <= r.windows).all() and (r.co >= 0).all()
        assert (r.co.diagonal(axis1=1, axis2=2)[:, :, None] >= r.co).all()
    x = c.D // 3
    a, b = kn.cooc(Vm, off, tok, sets, 10, 0, x), kn.cooc(Vm, off, tok, sets, 10, x, c.D)
    assert np.array_equal(a.co + b.co, ten.co) and a.windows + b.windows == ten.windows
    assert (a.tokens + b.tokens, a.hits + b.hits, a.oov + b.oov, a.entities + b.entities) == (ten.tokens, ten.hits, ten.oov, ten.entities)
    assert ten.oov > 0 and ten.hits > 0
    alone = kn.cooc(Vm, off, tok, sets[3:4], 10)                                             # a set's result does not depend on the others
    assert np.array_equal(alone.co[0], ten.co[3])
