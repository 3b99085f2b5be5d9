"""mvhdp_word_cooccurrence on a device against the literal restatement of its contract (tests/cooc_numpy.py): every output is an integer and
every integer is compared -- co, windows and the statistics.  Corpora of a few thousand tokens (tests/cooc_cases.py) at the shapes where the
device code takes another path: spans of 0, 1, 64, 65, 700 and 4 100 tokens against windows at and around 64 (a chunk of window starts) and
700 (one window or two), n at 1, 63 and 64 (the slot mask's last bit), word sets that keep the per-wave state in LDS and sets that push it
into global memory, a caller's corpus that goes up in several chunks."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import NativeGroup, SWEEP_NO_APPLY, merge_word_cooccurrence
from tests import cooc_cases as kc
from tests import cooc_numpy as kn
from tests.helpers import INV, STATE, UNSUPPORTED, load, state_of, untouched

pytestmark = pytest.mark.gpu
BIG = 2 ** 31 - 1
STAT_INTS = ("entities", "tokens", "hits", "oov", "distinct_words", "memberships")


def as_bytes(r):
    return r.co.tobytes() + np.int64(r.windows).tobytes() + b"".join(np.int64(getattr(r.stats, f)).tobytes() for f in STAT_INTS)


def check(s, c, m, sets, window, d0=0, d1=None, corpus=None, what=None):
    """one call against the restatement; returns (the device's answer, the restatement's)"""
    sets = np.asarray(sets, dtype=np.int32)
    ref = kn.cooc(c.V[m], c.doc_off[m], c.tokens[m], sets, window, d0, d1)
    got = s.word_cooccurrence(sets, m, window, d0, d1, corpus)
    where = (what, c.K, c.V[m], m, sets.shape, window, d0, d1)
    assert got.co.dtype == np.int64 and got.co.shape == ref.co.shape, where
    assert np.array_equal(got.co, ref.co), (where, np.argwhere(got.co != ref.co)[:6])
    assert got.windows == ref.windows, (where, got.windows, ref.windows)
    assert [getattr(got.stats, f) for f in STAT_INTS] == [getattr(ref, f) for f in STAT_INTS], (where, got.stats)
    assert np.array_equal(got.sets, sets)
    return got, ref


# (V_0, K, n, windows): every V, K, n and window at least once; the windows around 64 and 700 meet the 64-, 65- and 700-token entities in
# every case, for every case holds them
SHAPES = [(1, 1, 1, [0, 1, BIG]), (63, 5, 20, [2, 63, 64, 65]), (64, 65, 63, [10, 699, 700, 701]), (65, 5, 64, [64, 0, 110]),
          (257, 400, 20, [10, 0]), (1000, 65, 64, [1, 65])]


def test_the_shapes_cover_the_axes():
    assert {s[0] for s in SHAPES} == set(kc.V_VALUES) and {s[1] for s in SHAPES} == {1, 5, 65, 400} and {s[2] for s in SHAPES} == {1, 20, 63, 64}
    assert {w for s in SHAPES for w in s[3]} == {0, 1, 2, 10, 63, 64, 65, 110, 699, 700, 701, BIG}


@pytest.mark.parametrize("V0,K,n,windows", SHAPES)
def test_every_shape_equals_the_restatement(V0, K, n, windows):
    other = kc.V_VALUES[(kc.V_VALUES.index(V0) + 1) % len(kc.V_VALUES)]
    c = kc.make(K, [V0, other, 5])
    assert {0, 1, 64, 65, 700, kc.LONG} <= set(np.diff(c.doc_off[0]).tolist())
    with load(c) as s:
        top = s.top_words(0, n)[0]
        special, hot, never = kc.special_sets(c, 0, n)
        assert top.shape == (K, n) and (special[0] == -1).all() and (special[2] >= 0).sum() == 1
        if n >= 3:
            assert special[1, n // 2] == -1 and special[1, 0] >= 0 and (special[1, n // 2 + 1] >= 0 or V0 < n)
        if n >= 2:
            assert special[3, 0] == special[3, n - 1] == hot
        if V0 >= 257:
            assert never is not None and special[4, 0] == never, "every word occurs: reseed"
        if n == 64 and V0 >= 64:
            assert len(set(special[5].tolist())) == 64 and (special[5] >= 0).all()
        sets = np.concatenate([top, special[:1]]) if K == 400 else np.concatenate([top, special])
        assert len(sets) == (401 if K == 400 else K + 7)
        seen = dict(differs=False)
        doc = None
        for w in windows:
            got, ref = check(s, c, 0, sets, w)
            assert ref.oov > 0 and ref.hits > 0
            if never is not None and K != 400:
                assert got.co[K + 4, 0, 0] == 0 and (got.co[K + 4, 0] == 0).all()   # the word that never occurs: its row stays 0
            if n >= 2 and K != 400:
                assert got.co[K + 3, 0, n - 1] == got.co[K + 3, 0, 0] > 0           # the same word in two slots: both count
            doc = got if doc is None else doc
            seen["differs"] |= not np.array_equal(got.co, doc.co)
        if len({min(w, kc.LONG) for w in windows}) > 1 and V0 > 1:
            assert seen["differs"], "every window gives the same counts: reseed"
        w = windows[0]
        if K == 1:                                                           # n_sets 0 and 1
            check(s, c, 0, np.zeros((0, n), np.int32), w)
            check(s, c, 0, top, w)
        check(s, c, 0, special, w, what="seven sets")                        # n_sets 7
        hotsets = kc.with_hot_word(sets[:70], hot)
        assert (hotsets == hot).any(axis=1).all()
        got, _ = check(s, c, 0, hotsets, w, what="the hot word in every row")
        assert (got.co[:, n - 1, n - 1] == got.co[0, n - 1, n - 1]).all() and got.co[0, n - 1, n - 1] > 0
        check(s, c, 1, s.top_words(1, n)[0], w, what="view 1")


def test_sets_that_do_not_fit_lds_without_a_sliding_span():
    """6 001 sets of one slot: the per-wave masks and lists of a document-mode call live in global memory"""
    c = kc.make(5, [257, 64, 5], seed=1)
    sets = (np.arange(6001, dtype=np.int32) % 257).reshape(-1, 1)
    with load(c) as s:
        for w in (0, BIG):
            got, _ = check(s, c, 0, sets, w)
        assert np.array_equal(got.co[:257], got.co[257:514])


def test_the_callers_corpus():
    c = kc.make(5, [65, 64, 5], seed=2)
    with load(c) as s, NativeSampler(c.K, c.V) as bare:
        sets = np.concatenate([s.top_words(1, 20)[0], kc.special_sets(c, 1, 20)[0]])
        own = (c.doc_off[1], c.tokens[1])
        for w in (0, 10, 700):
            mine, _ = check(s, c, 1, sets, w)
            assert as_bytes(s.word_cooccurrence(sets, 1, w, corpus=own)) == as_bytes(mine), w
            # a handle that holds no corpus, no counts and no hyper-parameters
            assert as_bytes(bare.word_cooccurrence(sets, 1, w, corpus=own)) == as_bytes(mine), w
        x = c.D // 2
        got, _ = check(bare, c, 1, sets, 10, 3, x, corpus=own, what="a range of the caller's corpus")
        other = kc.make(5, [65, 64, 5], seed=3)                              # a corpus that is not the handle's
        check(s, other, 1, sets, 10, corpus=(other.doc_off[1], other.tokens[1]), what="another corpus")


def test_the_callers_corpus_in_several_chunks(monkeypatch):
    c = kc.make(5, [65, 64, 5], seed=2)
    own = (c.doc_off[0], c.tokens[0])
    with NativeSampler(c.K, c.V) as bare:
        sets = kc.special_sets(c, 0, 20)[0]
        one = bare.word_cooccurrence(sets, 0, 10, corpus=own)
        monkeypatch.setenv("MVHDP_COOC_CHUNK_TOKENS", "1000")                # the 4 100-token entity is a chunk of its own, above the size
        assert len(c.tokens[0]) > 5000
        got, _ = check(bare, c, 0, sets, 10, corpus=own, what="chunks of 1000 tokens")
        assert as_bytes(got) == as_bytes(one)
        check(bare, c, 0, sets, 0, 2, c.D - 1, corpus=own, what="chunks of 1000 tokens, a range")


def test_ranges_add_up_and_a_group_is_the_single_handle():
    c = kc.make(65, [257, 64, 5], seed=4)
    D = c.D
    with load(c) as s:
        sets = np.concatenate([s.top_words(0, 20)[0], kc.special_sets(c, 0, 20)[0]])
        for w in (0, 10):
            whole, _ = check(s, c, 0, sets, w)
            assert as_bytes(whole) == as_bytes(s.word_cooccurrence(sets, 0, w))                         # two calls, the same bytes
            for x in (0, 1, D // 3, D - 1, D):
                a, _ = check(s, c, 0, sets, w, 0, x)
                b, _ = check(s, c, 0, sets, w, x, D)
                assert as_bytes(merge_word_cooccurrence([a, b])) == as_bytes(whole), (w, x)
            assert as_bytes(s.word_cooccurrence(sets, 0, w, 0, D)) == as_bytes(whole)
            alone = s.word_cooccurrence(sets[3:4], 0, w)                     # a set's result does not depend on the others
            assert np.array_equal(alone.co[0], whole.co[3])
        h = D // 2
        with load(c, 0, h, counts=False) as a, load(c, h, None, counts=False) as b:
            g = NativeGroup.__new__(NativeGroup)
            g.members, g.g = [a, b], None
            for w in (0, 10):
                one = s.word_cooccurrence(sets, 0, w)
                assert as_bytes(g.word_cooccurrence(sets, 0, w)) == as_bytes(one)
                part = g.word_cooccurrence(sets, 0, w, 3, D - 2)
                assert as_bytes(part) == as_bytes(s.word_cooccurrence(sets, 0, w, 3, D - 2))
            assert g.word_cooccurrence(sets, 0, 0, 5, 5).windows == 0


def test_against_the_diagnostics_and_the_word_counts():
    """K = 1 and every token is topic 0, so the assignment-bound counts of mvhdp_diagnostics are the assignment-free ones"""
    c = kc.make(1, [257, 64, 5], holes=False)
    with load(c) as s:
        nz = int(s.top_words(0, 1)[2][0])
        for N in (1, 20, min(64, nz)):
            assert N <= nz
            d = s.diagnostics(N)
            assert (d.top_words >= 0).all()
            got = s.word_cooccurrence(d.top_words, 0, 0)
            assert np.array_equal(got.co[0], d.codoc[0].astype(np.int64)), N
        V = c.V[0]
        sets = np.full((-(-V // 64), 64), -1, dtype=np.int32)
        sets.reshape(-1)[:V] = np.arange(V)
        one = s.word_cooccurrence(sets, 0, 1)
        assert np.array_equal(one.occurrences().reshape(-1)[:V], d.word_type_counts.astype(np.int64)) and one.windows == len(c.tokens[0])
        coh = s.topic_coherence(20, 0, 10, "npmi")
        assert coh.shape == (1,) and np.isfinite(coh[0]) and -1.0 <= coh[0] <= 1.0
        same = s.word_cooccurrence(s.top_words(0, 20)[0], 0, 10).coherence("npmi")
        assert coh.tobytes() == same.tobytes()


# ---- the error paths: every output pre-filled and found untouched ----
def raw_call(s, args, S, sets, num_docs=0, doc_off=None, tokens=None, n=3, skip=(), sentinel=-7):
    arr = dict(co=np.full((max(S, 1), n, n), sentinel, np.int64), windows=np.full(1, sentinel, np.int64))
    st = _lib.CoocStatsC(sentinel, sentinel, sentinel, sentinel, sentinel, sentinel, float(sentinel))
    ptr = [None if k in skip else arr[k].ctypes.data for k in ("co", "windows")]
    rc = s.L.mvhdp_word_cooccurrence(s.h, None if args is None else C.byref(args), S, None if sets is None else sets.ctypes.data, num_docs,
                                     None if doc_off is None else doc_off.ctypes.data, None if tokens is None else tokens.ctypes.data, *ptr, C.byref(st))
    clean = untouched(arr, sentinel) and (st.entities, st.memberships, st.kernel_ms) == (sentinel, sentinel, float(sentinel))
    return rc, clean


def i32(*x):
    return np.array(x, dtype=np.int32)


def i64(*x):
    return np.array(x, dtype=np.int64)


def test_error_paths_leave_the_outputs_alone():
    c = kc.make(5, [65, 64, 5], seed=5, holes=False)
    A = _lib.CoocArgsC
    good = A(0, 3, 2, 0, -1)
    row = i32(1, -1, 2)
    off, tok = i64(0, 2, 5), i32(1, 70, 2, 0, 3)
    with load(c) as s:
        D = c.D
        bad = [
            dict(args=None, S=1, sets=row),                                  # NULL a
            dict(args=good, S=1, sets=row, skip=("co",)), dict(args=good, S=1, sets=row, skip=("windows",)),
            dict(args=good, S=-1, sets=row), dict(args=good, S=1, sets=None),
            dict(args=A(-1, 3, 2, 0, -1), S=1, sets=row), dict(args=A(3, 3, 2, 0, -1), S=1, sets=row),                # m
            dict(args=A(0, 0, 2, 0, -1), S=0, sets=None), dict(args=A(0, 65, 2, 0, -1), S=0, sets=None),              # n
            dict(args=A(0, 3, -1, 0, -1), S=1, sets=row),                                                             # window
            dict(args=good, S=1, sets=i32(1, -2, 2)), dict(args=good, S=1, sets=i32(1, 65, 2)),                       # a slot
            dict(args=good, S=1, sets=row, num_docs=-1, doc_off=off, tokens=tok),
            dict(args=good, S=1, sets=row, num_docs=2, doc_off=off, tokens=None),
            dict(args=good, S=1, sets=row, num_docs=2, doc_off=i64(1, 2, 5), tokens=tok),
            dict(args=good, S=1, sets=row, num_docs=2, doc_off=i64(0, 3, 2), tokens=tok),
            dict(args=good, S=1, sets=row, num_docs=2, doc_off=off, tokens=i32(1, 70, -1, 0, 3)),
            dict(args=A(0, 3, 2, -1, -1), S=1, sets=row), dict(args=A(0, 3, 2, 0, -2), S=1, sets=row),                # the range
            dict(args=A(0, 3, 2, 3, 2), S=1, sets=row), dict(args=A(0, 3, 2, 0, D + 1), S=1, sets=row),
            dict(args=A(0, 3, 2, 0, 3), S=1, sets=row, num_docs=2, doc_off=off, tokens=tok),
        ]
        for k, kw in enumerate(bad):
            rc, clean = raw_call(s, **kw)
            assert rc == INV and clean, (k, rc, clean)
            assert len(s.L.mvhdp_last_error(s.h)) > 10
        # the order: a bad slot is reported before a bad corpus, a bad corpus before a bad range
        raw_call(s, A(0, 3, 2, 0, 9), 1, i32(1, 99, 2), 2, i64(1, 2, 5), tok)
        assert b"slot" in s.L.mvhdp_last_error(s.h)
        raw_call(s, A(0, 3, 2, 0, 9), 1, row, 2, i64(1, 2, 5), tok)
        assert b"doc_off" in s.L.mvhdp_last_error(s.h)
        # more than 2^26 cells: refused before the sets are looked at beyond their slots
        S = 2 ** 26 // 64 ** 2 + 1
        many = np.zeros((S, 64), np.int32)
        rc, clean = raw_call(s, A(0, 64, 0, 0, -1), S, many, n=64)           # (co is never written: its one block is enough)
        assert rc == UNSUPPORTED and clean and b"2^26" in s.L.mvhdp_last_error(s.h)
        many[S - 1, 63] = 65
        assert raw_call(s, A(0, 64, 0, 0, -1), S, many, n=64) == (INV, True)  # a bad slot comes first
        # no sets, an empty range: OK, the windows still counted
        assert raw_call(s, A(0, 3, 2, 0, -1), 0, None, skip=())[0] == 0
        none = s.word_cooccurrence(np.zeros((0, 3), np.int32), 0, 2)
        assert none.windows == kn.cooc(c.V[0], c.doc_off[0], c.tokens[0], np.zeros((0, 3), np.int64), 2).windows > 0 and none.co.shape == (0, 3, 3)
        empty = s.word_cooccurrence([[1, 2, 3]], 0, 2, 4, 4)
        assert empty.windows == 0 and not empty.co.any() and empty.stats.memberships == 3
        # the caller's corpus with an out-of-vocabulary token is fine
        assert raw_call(s, good, 1, row, 2, off, tok)[0] == 0
        # nothing of the handle moves, and the call goes between a NO_APPLY sweep and its apply
        s.build_trees()
        before = (state_of(s), s.counts_written(), bytes(s.get_tuning()))
        trees = s.trees_current()
        sets = s.top_words(0, 20)[0]
        for w in (0, 10):
            check(s, c, 0, sets, w)
        assert (state_of(s), s.counts_written(), bytes(s.get_tuning())) == before and s.trees_current() == trees
        s.sweep(0, 5, flags=SWEEP_NO_APPLY)
        z = s.get_assignments(0)
        pending, _ = check(s, c, 0, sets, 10, what="pending")
        assert np.array_equal(s.get_assignments(0), z)
        s.apply_delta()
        assert as_bytes(s.word_cooccurrence(sets, 0, 10)) == as_bytes(pending)
        # a negative type in the handle's corpus is refused where it is read, and nowhere else
        t = c.tokens[0].copy()
        d0 = int(np.flatnonzero(np.diff(c.doc_off[0]) > 2)[0])
        t[c.doc_off[0][d0] + 1] = -1
        s.set_corpus(0, c.doc_off[0], t)
        rc, clean = raw_call(s, A(0, 3, 2, d0, d0 + 1), 1, row)
        assert rc == STATE and clean and b"negative type" in s.L.mvhdp_last_error(s.h)
        assert raw_call(s, A(0, 3, 2, d0 + 1, -1), 1, row)[0] == 0 and raw_call(s, A(0, 3, 2, 0, d0), 1, row)[0] == 0
        with pytest.raises(MvhdpError) as e:
            s.word_cooccurrence([[1, 2]], 0, 0)
        assert e.value.code == STATE
    with NativeSampler(3, [4, 5]) as fresh:                                  # no corpus of the view
        rc, clean = raw_call(fresh, A(1, 3, 2, 0, -1), 1, row)
        assert rc == STATE and clean and b"set_corpus" in fresh.L.mvhdp_last_error(fresh.h)
        with pytest.raises(ValueError):
            fresh.word_cooccurrence(np.zeros(3, np.int32))
