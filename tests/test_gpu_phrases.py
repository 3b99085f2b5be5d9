"""mvhdp_topic_phrases on a device against the literal restatement of findTopicPhrases (tests/phrases_numpy.py).  Everything is compared
exactly and in whole: topic_off, word_off, words, counts, distinct, occurrences and the statistics.  No sweep is needed to place a z:
set_assignments does.  Shapes: document lengths at and around the 64-wide step of the walk and its multiples, documents of thousands of
tokens, and constructed documents whose runs, phrases and chains of length-2 runs cross those steps."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import Hyper, NativeGroup, merge_topic_phrases
from tests import jni_harness as H
from tests import phrases_numpy as pn
from tests.helpers import INV, STATE, untouched
from tests.native_build import jvm  # noqa: F401

pytestmark = pytest.mark.gpu
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129]


def sampler(K, V, off, tok, z=None):
    """view 0 as given; every further view of V a small corpus of its own over the same entities"""
    s = NativeSampler(K, V)
    s.set_corpus(0, off, tok)
    if z is not None:
        s.set_assignments(0, z)
    rng = np.random.default_rng(len(V))
    D = len(off) - 1
    for m in range(1, len(V)):
        o = np.concatenate([[0], np.cumsum(rng.integers(0, 6, D))]).astype(np.int64)
        s.set_corpus(m, o, rng.integers(0, V[m], o[-1]).astype(np.int32))
        s.set_assignments(m, rng.integers(0, K, o[-1]).astype(np.int32))
    return s


def random_case(K, V, seed, sets=20, long_docs=(2048, 5000)):
    """Runs and repeats on purpose: a token keeps the topic before it with probability 0.55; topics and words are drawn from geometric
    distributions, so that a few phrases repeat often and the tail ties at count 1.  With K >= 3 topic 1 is never drawn."""
    rng = np.random.default_rng(seed)
    lens = np.array(LENGTHS * sets + list(long_docs))
    rng.shuffle(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    tok = np.minimum(rng.geometric(0.4, N) - 1, V - 1).astype(np.int32)
    draw = np.minimum(rng.geometric(0.3, N) - 1, K - 1)
    if K >= 3:
        draw = np.where(draw >= 1, np.minimum(draw + 1, K - 1), 0)
    stay = rng.random(N) < 0.55
    start = np.zeros(N, bool)
    start[off[:-1][lens > 0]] = True
    z = draw.astype(np.int32)
    for i in range(1, N):
        if stay[i] and not start[i]:
            z[i] = z[i - 1]
    return off, tok, z


def assert_equal(got, want, what):
    names = ["topic_off", "word_off", "words", "counts", "distinct", "occurrences"]
    for name, g, w in zip(names, got[:6], want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, g[:12], w[:12])


def check(s, K, off, tok, z, max_n, hash_bits=0, what=None):
    got = s.topic_phrases_raw(max_n, hash_bits)
    want = pn.topic_phrases(K, off, tok, z, max_n)
    assert_equal(got, want, what)
    st = got[6]
    assert st.occurrences == int(want[5].sum()) and st.distinct == int(want[4].sum()) and st.kept == len(want[3]), (what, st)
    assert st.runs == pn.count_runs(off, z), (what, st)
    return got, want


@pytest.mark.parametrize("V0", [2, 4, 50])
@pytest.mark.parametrize("K", [1, 3, 5, 100])
def test_random_documents_equal_the_restatement(K, V0):
    off, tok, z = random_case(K, V0, 100 * K + V0)
    assert set(LENGTHS) | {2048, 5000} <= set(np.diff(off))
    ph = pn.find_topic_phrases(K, off, tok, z)
    if K == 1:
        # one topic: every entity is a single run, and a run that reaches the end of the entity is dropped -- the reference finds nothing
        assert not any(ph)
    else:
        # the case has something to find: repeated phrases, a count tie across the cut at 20, a topic without a phrase
        assert max(max(p.values()) for p in ph if p) >= 2
        ties = [k for k in range(K) if len(ph[k]) > 20 and pn.order_and_cut(ph[k], 21)[19][1] == pn.order_and_cut(ph[k], 21)[20][1]]
        assert ties, "no topic ties at the cut: reseed"
        assert any(not p for p in ph)
    with sampler(K, [V0], off, tok, z) as s:
        for max_n in (20, -1):
            check(s, K, off, tok, z, max_n, what=(K, V0, max_n))


def alternating(n, a=0, b=1):
    return [a if i % 2 == 0 else b for i in range(n)]


def chain(nruns, first=0):
    """nruns consecutive runs of length 2 over three topics, then one token that ends the last run"""
    out = []
    for r in range(nruns):
        out += [(first + r) % 3] * 2
    return out + [(first + nruns) % 3]


SEAMS = {
    # (list of per-document topic sequences)
    "run_62_to_66": [alternating(62) + [2] * 5 + [0, 1]],
    "phrase_longer_than_64": [[0] * 70 + [1]],
    "phrase_longer_than_256": [[1] + [2] * 300 + [0, 0]],
    "chain_of_40": [chain(40)],
    "chain_of_40_shifted": [[2] + chain(40)],
    "chain_of_40_from_60": [alternating(60, 1, 2) + chain(40)],
    "chain_of_40_from_61": [alternating(61, 1, 2) + chain(40, 2)],
    "one_single_run": [[1] * 200],
    "ends_in_an_open_phrase": [[0, 1, 1, 1], [2] * 64 + [1] * 64, [0] * 65],
    "entity_without_view_0": [[0, 0, 1], [], [0, 0, 1, 1, 1, 2]],
    "break_on_the_first_lane": [alternating(62) + [2, 2] + [0], alternating(126) + [2, 2] + [0], [2] * 64 + [0], [1] + [2] * 127 + [0]],
}


def seam_corpus(docs, V0=400, words="position"):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    z = np.array([t for d in docs for t in d], dtype=np.int32)
    if words == "position":
        tok = np.concatenate([np.arange(len(d)) % V0 for d in docs] + [np.zeros(0, int)]).astype(np.int32)
    else:
        tok = np.random.default_rng(len(z)).integers(0, 2, len(z)).astype(np.int32)
    return off, tok, z


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_constructed_documents_at_the_seams(name):
    K = 3
    for words in ("position", "binary"):
        off, tok, z = seam_corpus(SEAMS[name], words=words)
        ph = pn.find_topic_phrases(K, off, tok, z)
        lens = sorted(len(ids) for p in ph for ids in p)
        n = sum(sum(p.values()) for p in ph)
        if name == "run_62_to_66":
            assert n == 1 and lens == [5] and list(ph[2])[0][0] == tok[62]
        elif name == "phrase_longer_than_64":
            assert lens == [70]
        elif name == "phrase_longer_than_256":
            assert lens == [300]
        elif name.startswith("chain_of_40"):
            assert n == 20 and set(lens) == {2}                              # every second run of the chain
        elif name == "one_single_run":
            assert n == 0
        elif name == "ends_in_an_open_phrase":
            assert n == 1 and lens == [64]                                   # only the run of 2s that a 1 breaks; the open ones are dropped
        elif name == "entity_without_view_0":
            assert n == 3 and off[1] == off[2]
        with sampler(K, [400], off, tok, z) as s:
            check(s, K, off, tok, z, -1, what=(name, words))
            check(s, K, off, tok, z, 1, what=(name, words))
    # the two chains really differ by the parity of the swallowed token
    a = pn.find_topic_phrases(3, *seam_corpus(SEAMS["chain_of_40"]))
    b = pn.find_topic_phrases(3, *seam_corpus(SEAMS["chain_of_40_shifted"]))
    assert sorted(i[0] for p in a for i in p) == list(range(0, 80, 4)) and sorted(i[0] for p in b for i in p) == list(range(1, 81, 4))


@pytest.fixture(scope="module")
def base():
    K, V0 = 3, 4
    off, tok, z = random_case(K, V0, 7)
    ph = pn.find_topic_phrases(K, off, tok, z)
    s = sampler(K, [V0], off, tok, z)
    yield s, K, V0, off, tok, z, ph
    s.close()


def test_only_view_0_is_read():
    K = 5
    off, tok, z = random_case(K, 4, 11, sets=3, long_docs=(300,))
    with sampler(K, [4, 7, 9], off, tok, z) as s:
        assert s.M == 3
        check(s, K, off, tok, z, 20, what="M = 3")


def test_cuts(base):
    s, K, V0, off, tok, z, ph = base
    longest = max(len(p) for p in ph)
    assert longest > 20
    for max_n in (-1, 0, 1, 20, longest + 5, 10 ** 6):
        got, want = check(s, K, off, tok, z, max_n, what=("cut", max_n))
        assert got[6].kept == sum(len(p) if max_n < 0 else min(max_n, len(p)) for p in ph)
    r = s.topic_phrases(2, vocabulary=["a", "b", "c", "d"])
    ids = s.topic_phrases(2)
    assert [[(" ".join("abcd"[i] for i in k), c) for k, c in row] for row in ids.phrases] == r.phrases
    assert ids.phrases == pn.lists(ph, 2) and list(ids.occurrences) == [sum(p.values()) for p in ph]


@pytest.mark.parametrize("bits", [1, 4])
def test_forced_hash_collisions_change_nothing(base, bits):
    s, K, V0, off, tok, z, ph = base
    assert sum(sum(p.values()) for p in ph) > 2000 and sum(len(p) for p in ph) > 100
    plain, want = check(s, K, off, tok, z, -1, what="64 bits")
    assert plain[6].hash_collisions == 0
    forced, _ = check(s, K, off, tok, z, -1, hash_bits=bits, what=("bits", bits))
    assert_equal(forced, plain[:6], ("bits against 64", bits))
    assert forced[6].hash_collisions > 0
    check(s, K, off, tok, z, 20, hash_bits=bits, what=("bits", bits, 20))


def raw_call(s, max_n, cap_p, cap_w, sentinel=-7):
    """the arrays filled with a sentinel, one element longer than their capacity"""
    a = _lib.PhraseArgsC(max_n, 0)
    arr = dict(topic_off=np.full(s.K + 1, sentinel, np.int64), word_off=np.full(cap_p + 2, sentinel, np.int64), words=np.full(cap_w + 1, sentinel, np.int32),
               counts=np.full(cap_p + 1, sentinel, np.int32), distinct=np.full(s.K, sentinel, np.int64), occurrences=np.full(s.K, sentinel, np.int64))
    n, w, st = C.c_int64(sentinel), C.c_int64(sentinel), _lib.PhraseStatsC()
    rc = s.L.mvhdp_topic_phrases(s.h, C.byref(a), cap_p, cap_w, *[arr[k].ctypes.data for k in ("topic_off", "word_off", "words", "counts", "distinct", "occurrences")],
                                 C.byref(n), C.byref(w), C.byref(st))
    return rc, arr, n.value, w.value


def test_capacity_protocol(base):
    s, K, V0, off, tok, z, ph = base
    want = pn.topic_phrases(K, off, tok, z, 20)
    np_, nw = len(want[3]), len(want[2])
    assert np_ == sum(min(20, len(p)) for p in ph) > 20 and nw >= np_ * 2
    # the size query: the sizes, and the per-topic arrays unless NULL
    a = _lib.PhraseArgsC(20, 0)
    n, w = C.c_int64(), C.c_int64()
    toff, di, oc = np.zeros(K + 1, np.int64), np.zeros(K, np.int64), np.zeros(K, np.int64)
    assert s.L.mvhdp_topic_phrases(s.h, C.byref(a), 0, 0, None, None, None, None, None, None, C.byref(n), C.byref(w), None) == 0
    assert (n.value, w.value) == (np_, nw)
    assert s.L.mvhdp_topic_phrases(s.h, C.byref(a), 0, 0, toff.ctypes.data, None, None, None, di.ctypes.data, oc.ctypes.data, C.byref(n), C.byref(w), None) == 0
    assert np.array_equal(toff, want[0]) and np.array_equal(di, want[4]) and np.array_equal(oc, want[5])
    # exact caps: filled, and nothing behind the capacity is written
    rc, arr, n2, w2 = raw_call(s, 20, np_, nw)
    assert rc == 0 and (n2, w2) == (np_, nw)
    assert_equal((arr["topic_off"], arr["word_off"][:np_ + 1], arr["words"][:nw], arr["counts"][:np_], arr["distinct"], arr["occurrences"]), want, "exact caps")
    assert arr["word_off"][np_ + 1] == -7 and arr["words"][nw] == -7 and arr["counts"][np_] == -7
    # one cap too small: INVALID_ARG, the sizes set, the arrays untouched
    for cp, cw in ((np_ - 1, nw), (np_, nw - 1), (0, nw), (np_, 0)):
        rc, arr, n2, w2 = raw_call(s, 20, cp, cw)
        assert rc == INV and (n2, w2) == (np_, nw) and untouched(arr), (cp, cw)
        assert b"cap" in s.L.mvhdp_last_error(s.h)
    # the argument contract
    assert s.L.mvhdp_topic_phrases(s.h, None, 0, 0, None, None, None, None, None, None, C.byref(n), C.byref(w), None) == INV
    assert s.L.mvhdp_topic_phrases(s.h, C.byref(a), -1, 0, None, None, None, None, None, None, C.byref(n), C.byref(w), None) == INV
    assert s.L.mvhdp_topic_phrases(s.h, C.byref(a), 4, 4, None, None, None, None, None, None, C.byref(n), C.byref(w), None) == INV
    assert s.L.mvhdp_topic_phrases(s.h, C.byref(_lib.PhraseArgsC(20, 64)), 0, 0, None, None, None, None, None, None, C.byref(n), C.byref(w), None) == INV
    assert s.L.mvhdp_topic_phrases(s.h, C.byref(a), 0, 0, None, None, None, None, None, None, None, C.byref(w), None) == INV


def test_error_cases_leave_the_outputs_and_the_handle_alone():
    K, V0 = 3, 4
    off, tok, z = random_case(K, V0, 3, sets=2, long_docs=(200,))
    N = len(z)

    def refused(s):
        rc, arr, n, w = raw_call(s, 20, 1000, 10000)
        assert rc == STATE and untouched(arr) and (n, w) == (-7, -7), rc
        assert len(s.L.mvhdp_last_error(s.h)) > 10
        with pytest.raises(MvhdpError) as e:
            s.topic_phrases()
        assert e.value.code == STATE

    with NativeSampler(K, [V0]) as s:                                        # no corpus
        refused(s)
        s.set_corpus(0, off, tok)                                            # no assignments set: every z is -1
        refused(s)
        for pos in (0, 63, 64, N - 1):                                       # one unassigned token, on the first and last lane of a step too
            zz = z.copy()
            zz[pos] = -1
            s.set_assignments(0, zz)
            refused(s)
        # z = K cannot be placed: set_assignments itself refuses it, so the state never reaches the walk (which checks z >= K all the same)
        zz = z.copy()
        zz[5] = K
        with pytest.raises(MvhdpError) as e:
            s.set_assignments(0, zz)
        assert e.value.code == INV
        s.set_assignments(0, z)                                              # the handle is usable afterwards
        check(s, K, off, tok, z, 20, what="after the refusals")
        for bad in (V0, V0 + 9, -1):                                         # a token outside [0, V_0)
            t2 = tok.copy()
            t2[N // 2] = bad
            s.set_corpus(0, off, t2)
            s.set_assignments(0, z)
            refused(s)
        s.set_corpus(0, off, tok)
        s.set_assignments(0, z)
        check(s, K, off, tok, z, -1, what="after a bad token")
    # an empty corpus, and entities that are all empty, are not errors
    with sampler(K, [V0], np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)) as s:
        check(s, K, np.zeros(1, np.int64), [], [], 20, what="D = 0")
    with sampler(K, [V0], np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)) as s:
        check(s, K, np.zeros(5, np.int64), [], [], -1, what="empty spans")


def as_bytes(got):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in got[:6])


def test_two_calls_give_the_same_bytes_also_across_a_sweep():
    K, V0 = 3, 4
    off, tok, z = random_case(K, V0, 7)
    with sampler(K, [V0], off, tok, z) as s:
        first = as_bytes(s.topic_phrases_raw(20))
        assert first == as_bytes(s.topic_phrases_raw(20))
        full = as_bytes(s.topic_phrases_raw(-1))
        assert full == as_bytes(s.topic_phrases_raw(-1)) == as_bytes(s.topic_phrases_raw(-1, 4))
        s.set_hyper(Hyper.defaults(K, [V0]))
        s.build_counts()
        s.sweep(0, 99)                                                       # one deferred sweep moves z
        moved = s.get_assignments(0)
        assert (moved != z).any()
        check(s, K, off, tok, moved, 20, what="after a sweep")
        s.set_assignments(0, z)                                              # the same z restored: the same bytes
        assert as_bytes(s.topic_phrases_raw(20)) == first and as_bytes(s.topic_phrases_raw(-1)) == full


def test_merge_over_two_handles_equals_one_handle():
    K, V0 = 5, 4
    off, tok, z = random_case(K, V0, 21, sets=6, long_docs=(700,))
    D = len(off) - 1
    h = D // 2
    with sampler(K, [V0], off, tok, z) as whole, \
            sampler(K, [V0], off[:h + 1], tok[:off[h]], z[:off[h]]) as a, \
            sampler(K, [V0], off[h:] - off[h], tok[off[h]:], z[off[h]:]) as b:
        for max_n in (20, -1, 1):
            one = whole.topic_phrases(max_n)
            two = merge_topic_phrases([a.topic_phrases(-1), b.topic_phrases(-1)], max_n)
            assert two.phrases == one.phrases and np.array_equal(two.distinct, one.distinct) and np.array_equal(two.occurrences, one.occurrences)
            assert (two.stats.occurrences, two.stats.distinct, two.stats.kept) == (one.stats.occurrences, one.stats.distinct, one.stats.kept)
        # NativeGroup.topic_phrases merges its local members (no sweep, so no counts are needed to form the group's answer)
        g = NativeGroup.__new__(NativeGroup)
        g.members, g.g = [a, b], None
        assert g.topic_phrases(20).phrases == whole.topic_phrases(20).phrases
        assert g.topic_phrases(3, vocabulary="abcd").phrases == whole.topic_phrases(3, vocabulary="abcd").phrases


# ---- the Java path: the four shim sources as one library, under the test-side JNIEnv (tests/jni_harness.py) ---------------------------
IAE = "java/lang/IllegalArgumentException"


def test_the_java_entry_equals_the_binding(jvm, base):
    s, K, V0, off, tok, z, ph = base
    j = H.JniSampler(jvm, K, [V0])
    try:
        j.setCorpus(0, off, tok)
        h = j.handle
        with pytest.raises(H.JavaException) as e:                            # a library error becomes a RuntimeException with its text
            jvm.call("nTopicPhrases", h, 20, 0, None, None, None, None, None, None, jvm.longs(2), None)
        assert e.value.cls == "java/lang/RuntimeException" and "unassigned" in e.value.msg
        j.setAssignments(0, z)
        for max_n in (20, -1):
            want = s.topic_phrases_raw(max_n)
            sizes = jvm.longs(2)
            n = jvm.call("nTopicPhrases", h, max_n, 0, None, None, None, None, None, None, sizes, None)
            assert n == len(want[3]) and list(sizes.get()) == [len(want[3]), len(want[2])]
            nw = len(want[2])
            jto, jwo, jw, jc, jd, jo, jst = jvm.longs(K + 1), jvm.longs(n + 1), jvm.ints(nw), jvm.ints(n), jvm.longs(K), jvm.longs(K), jvm.longs(5)
            assert jvm.call("nTopicPhrases", h, max_n, 0, jto, jwo, jw, jc, jd, jo, sizes, jst) == n
            assert_equal((jto.get(), jwo.get(), jw.get().astype(np.int32), jc.get().astype(np.int32), jd.get(), jo.get()), want[:6], ("java", max_n))
            st = want[6]
            assert list(jst.get()) == [st.runs, st.occurrences, st.distinct, st.kept, st.hash_collisions]
            assert list(jvm_bits(jvm, h, max_n, K, n, nw)) == list(jc.get())
        # too small: the sizes, the arrays untouched, no exception
        want = s.topic_phrases_raw(20)
        n, nw = len(want[3]), len(want[2])
        jwo, jw, jc, sizes = jvm.longs([-7] * n), jvm.ints([-7] * nw), jvm.ints([-7] * (n - 1)), jvm.longs(2)
        assert jvm.call("nTopicPhrases", h, 20, 0, None, jwo, jw, jc, None, None, sizes, None) == n
        assert list(sizes.get()) == [n, nw] and (jwo.get() == -7).all() and (jw.get() == -7).all() and (jc.get() == -7).all()

        # a wrong array length is refused before the library is reached
        def refused(*args):
            with pytest.raises(H.JavaException) as e:
                jvm.call("nTopicPhrases", *args)
            assert e.value.cls == IAE, e.value
        ok = dict(to=jvm.longs(K + 1), wo=jvm.longs(n + 1), w=jvm.ints(nw), c=jvm.ints(n), d=jvm.longs(K), o=jvm.longs(K), sz=jvm.longs(2), st=jvm.longs(5))
        refused(h, 20, 0, jvm.longs(K), ok["wo"], ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, jvm.longs(K + 2), ok["wo"], ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], jvm.longs(n), ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], jvm.longs(n + 2), ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], ok["wo"], ok["w"], None, ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], None, ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], None, ok["w"], None, ok["d"], ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], ok["wo"], ok["w"], ok["c"], jvm.longs(K + 1), ok["o"], ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], ok["wo"], ok["w"], ok["c"], ok["d"], jvm.longs(K - 1), ok["sz"], ok["st"])
        refused(h, 20, 0, ok["to"], ok["wo"], ok["w"], ok["c"], ok["d"], ok["o"], jvm.longs(1), ok["st"])
        refused(h, 20, 0, ok["to"], ok["wo"], ok["w"], ok["c"], ok["d"], ok["o"], None, ok["st"])
        refused(h, 20, 0, ok["to"], ok["wo"], ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], jvm.longs(4))
        assert jvm.call("nTopicPhrases", h, 20, 0, ok["to"], ok["wo"], ok["w"], ok["c"], ok["d"], ok["o"], ok["sz"], ok["st"]) == n   # and the right lengths pass
        with pytest.raises(H.JavaException) as e:                            # hash_bits outside 0..63: the library's refusal
            jvm.call("nTopicPhrases", h, 20, 64, None, None, None, None, None, None, jvm.longs(2), None)
        assert e.value.cls == "java/lang/RuntimeException" and "hash_bits" in e.value.msg
    finally:
        j.close()
    for closed in (j.handle, h):                                             # a closed sampler: its handle is 0; and the jlong it had is refused too
        with pytest.raises(H.JavaException) as e:
            jvm.call("nTopicPhrases", closed, 20, 0, None, None, None, None, None, None, jvm.longs(2), None)
        assert e.value.cls == "java/lang/IllegalStateException" and e.value.msg == "NativeSampler is closed"
    assert j.handle == 0 and h != 0


def jvm_bits(jvm, h, max_n, K, n, nw):
    """a second Java call with forced collisions: the same counts"""
    jc = jvm.ints(n)
    jvm.call("nTopicPhrases", h, max_n, 3, jvm.longs(K + 1), jvm.longs(n + 1), jvm.ints(nw), jc, None, None, jvm.longs(2), None)
    return jc.get()
