"""mvhdp_heldout_left_to_right on a device against the sequential restatement of its contract (tests/native/ltr_ref.c): position_sum bit
for bit, the integer outputs equal, the logs within 8 * 2^-53 * sum_n (|log S[n]| + log R) of numpy's logs of the same S (the device's log
is not glibc's: two ulp per term plus the summation).  The comparison target is the restatement, never the device's own output.
Shapes: K below, at and above the 64 lanes, ragged and several topics a lane (both gather paths: K a multiple of 4 or not); document
lengths around the 64-lane width and of 0, 1, 2 tokens; out-of-vocabulary tokens first, in the middle, last; a document beyond the LDS cap
of z; more work items than waves."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib, synth
from mvtopicmodel_amd.native import SWEEP_NO_APPLY, Hyper, NativeGroup
from tests import jni_harness as H
from tests import ltr_cases as lc
from tests import ltr_ref as lr
from tests.helpers import INV, STATE, uneven_hyper as hyper
from tests.native_build import jvm  # noqa: F401

pytestmark = pytest.mark.gpu
KS = [5, 64, 100, 130, 1000]


class Model:
    """a sampler whose counts were reached by two deferred sweeps of a synthetic corpus, and what the restatement needs of it"""

    def __init__(self, K, V, seed=3, D=200):
        c = synth.generate(K, V, D, [40] + [6] * (len(V) - 1), seed=seed)
        rng = np.random.default_rng(seed)
        self.K, self.V, self.hy = K, V, hyper(K, V, seed)
        self.s = s = NativeSampler(K, V)
        for m in range(c.M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m])
            s.set_assignments(m, rng.integers(0, K, len(c.tokens[m])).astype(np.int32))
        s.set_hyper(self.hy)
        s.build_counts()
        for it in range(2):
            s.sweep(it, 99)
        self.alpha = s.get_alpha()[0]

    def ref_args(self, m=0):
        nwk, nk = self.s.get_counts(m)
        return nwk, nk, float(self.hy.beta[m]), self.alpha[m, :self.K].copy(), float(self.hy.gamma[m] * self.hy.alpha_sum[m])

    def close(self):
        self.s.close()


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(K):
        if K not in made:
            made[K] = Model(K, [150 if K < 1000 else 200])
        return made[K]
    yield get
    for mdl in made.values():
        mdl.close()


def assert_equals_ref(got, ref, what):
    assert got.position_sum.dtype == np.float64 and np.array_equal(got.position_sum.view(np.uint64), ref.S.view(np.uint64)), \
        (what, np.flatnonzero(got.position_sum != ref.S)[:8])
    assert np.array_equal(got.doc_tokens, ref.doc_tokens), what
    assert (got.tokens, got.oov, got.visits) == (ref.tokens, ref.oov, ref.visits), (what, got.tokens, got.oov, got.visits, ref.tokens, ref.oov, ref.visits)
    err = np.abs(got.doc_log_likelihood - ref.doc_ll)
    print(what, "max doc_ll error / bound", float((err / np.maximum(ref.doc_bound, 1e-300)).max()) if len(err) else 0.0,
          "total error", abs(got.log_likelihood - ref.log_likelihood), "bound", ref.bound)
    assert (err <= ref.doc_bound).all(), (what, err.max())
    assert abs(got.log_likelihood - ref.log_likelihood) <= ref.bound, what


@pytest.mark.parametrize("resample", [0, 1])
@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_shapes_equal_the_restatement(models, K, R, resample):
    mdl = models(K)
    off, tok = lc.heldout_docs(mdl.V[0], n_docs=40, seed=K)
    assert set(np.diff(off)) == set(lc.LENGTHS)
    ref = lr.evaluate(*mdl.ref_args(), off, tok, particles=R, resample=bool(resample), seed=1234 + K)
    got = mdl.s.heldout_left_to_right(off, tok, particles=R, resample=bool(resample), seed=1234 + K, want_position_sums=True)
    assert ref.oov > 0 and (ref.doc_tokens == 0).sum() >= 2                  # an empty and an all-out-of-vocabulary document
    assert_equals_ref(got, ref, (K, R, resample))
    assert got.perplexity == float(np.exp(-got.log_likelihood / got.tokens)) and got.perplexity > 1


def test_a_long_document_keeps_z_beyond_the_lds_cap(models):
    mdl = models(100)
    rng = np.random.default_rng(6)
    off = np.array([0, 600], dtype=np.int64)
    tok = rng.integers(0, mdl.V[0], 600).astype(np.int32)
    tok[[0, 300, 555, 599]] = mdl.V[0]                                       # out of vocabulary on both sides of the cap
    ref = lr.evaluate(*mdl.ref_args(), off, tok, particles=2, seed=5)
    assert ref.visits == 2 * (596 * 597 // 2 + sum(int((tok[:i] < mdl.V[0]).sum()) for i in (0, 300, 555, 599)))
    got = mdl.s.heldout_left_to_right(off, tok, particles=2, seed=5, want_position_sums=True)
    assert_equals_ref(got, ref, "long")


def test_more_items_than_waves_go_through_the_queue(models):
    mdl = models(64)
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 9, 300)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = rng.integers(0, mdl.V[0] + 10, off[-1]).astype(np.int32)           # some out of vocabulary
    ref = lr.evaluate(*mdl.ref_args(), off, tok, particles=3, seed=77)
    got = mdl.s.heldout_left_to_right(off, tok, particles=3, seed=77, want_position_sums=True)   # 900 items, two a wave at least
    assert_equals_ref(got, ref, "queue")


@pytest.fixture(scope="module")
def peaked():
    s = NativeSampler(3, [2])
    hy = Hyper.defaults(3, [2], alpha=0.05, beta=lc.PEAKED_BETA)
    hy.alpha[0, :3] = lc.PEAKED_ALPHA
    hy.alpha_sum[0] = lc.PEAKED_ALPHA_SUM
    s.set_hyper(hy)
    s.set_counts(0, lc.PEAKED_NWK, lc.PEAKED_NK)
    yield s
    s.close()


@pytest.mark.parametrize("resample", [1, 0])
def test_position_one_is_unbiased_on_the_device(peaked, resample):
    exact, a, b, half, forgets = lc.peaked_expectation()
    off, tok = lc.PEAKED_DOC
    got = peaked.heldout_left_to_right(off, tok, particles=lc.PEAKED_R, resample=bool(resample), seed=11, want_position_sums=True)
    est = got.position_sum[1] / lc.PEAKED_R
    print("estimate", est, "exact", exact, "half-width", half)
    assert abs(est - exact) <= half
    assert all(abs(f - exact) > half for f in forgets)
    ref = lr.evaluate(lc.PEAKED_NWK, lc.PEAKED_NK, lc.PEAKED_BETA, lc.PEAKED_ALPHA, lc.PEAKED_ALPHA_SUM, off, tok, particles=lc.PEAKED_R, resample=bool(resample), seed=11)
    assert_equals_ref(got, ref, "peaked")


def test_two_calls_same_bytes_and_nothing_of_the_handle_moves(models):
    mdl = models(130)
    s = mdl.s
    off, tok = lc.heldout_docs(mdl.V[0], n_docs=20, seed=2)
    nwk, nk = s.get_counts(0)
    z = s.get_assignments(0)
    trees, tuning = s.trees_current(), bytes(s.get_tuning())
    one = s.heldout_left_to_right(off, tok, particles=3, seed=8, want_position_sums=True)
    two = s.heldout_left_to_right(off, tok, particles=3, seed=8, want_position_sums=True)
    for x, y in ((one.position_sum, two.position_sum), (one.doc_log_likelihood, two.doc_log_likelihood), (one.doc_tokens, two.doc_tokens)):
        assert x.tobytes() == y.tobytes()
    assert (one.log_likelihood, one.tokens, one.oov, one.visits) == (two.log_likelihood, two.tokens, two.oov, two.visits)
    other = s.heldout_left_to_right(off, tok, particles=3, seed=9, want_position_sums=True)
    assert other.position_sum.tobytes() != one.position_sum.tobytes()       # the seed reaches the draws
    nwk2, nk2 = s.get_counts(0)
    assert np.array_equal(nwk, nwk2) and np.array_equal(nk, nk2) and np.array_equal(z, s.get_assignments(0))
    assert s.trees_current() == trees and bytes(s.get_tuning()) == tuning


def test_doc_base_slice_alpha_override_and_another_view():
    K, V = 20, [60, 30, 25]
    mdl = Model(K, V, seed=5, D=120)
    try:
        s = mdl.s
        off, tok = lc.heldout_docs(V[0], n_docs=14, seed=3, lengths=[0, 1, 2, 7, 33])
        whole = s.heldout_left_to_right(off, tok, particles=2, seed=4, want_position_sums=True)
        assert_equals_ref(whole, lr.evaluate(*mdl.ref_args(0), off, tok, particles=2, seed=4), "view 0 of three")
        a, b = 3, 11
        part = s.heldout_left_to_right(off[a:b + 1] - off[a], tok[off[a]:off[b]], particles=2, seed=4, doc_base=a, want_position_sums=True)
        assert part.position_sum.tobytes() == whole.position_sum[off[a]:off[b]].tobytes()
        assert part.doc_log_likelihood.tobytes() == whole.doc_log_likelihood[a:b].tobytes()
        # the handle's own values as an override: nothing changes
        _, _, _, alpha, asum = mdl.ref_args(0)
        same = s.heldout_left_to_right(off, tok, particles=2, seed=4, alpha=alpha, alpha_sum=asum, want_position_sums=True)
        assert same.position_sum.tobytes() == whole.position_sum.tobytes() and same.doc_log_likelihood.tobytes() == whole.doc_log_likelihood.tobytes()
        # consistent values (gamma * alpha_k with its sum) are another estimate
        nwk, nk, beta, _, _ = mdl.ref_args(0)
        scaled = alpha * mdl.hy.gamma[0]
        got = s.heldout_left_to_right(off, tok, particles=2, seed=4, alpha=scaled, alpha_sum=float(scaled.sum()), want_position_sums=True)
        assert_equals_ref(got, lr.evaluate(nwk, nk, beta, scaled, float(scaled.sum()), off, tok, particles=2, seed=4), "override")
        assert got.position_sum.tobytes() != whole.position_sum.tobytes()
        # view 1: its own counts, beta, alpha row, gamma and vocabulary
        off1, tok1 = lc.heldout_docs(V[1], n_docs=14, seed=9, lengths=[0, 1, 2, 7, 33])
        got1 = s.heldout_left_to_right(off1, tok1, particles=2, seed=4, m=1, want_position_sums=True)
        assert_equals_ref(got1, lr.evaluate(*mdl.ref_args(1), off1, tok1, particles=2, seed=4), "view 1")
        # the counts as the handle holds them: behind a NO_APPLY sweep, until its deltas are applied, that is still the model before it
        s.sweep(2, 99, flags=SWEEP_NO_APPLY)
        held = s.heldout_left_to_right(off, tok, particles=2, seed=4, want_position_sums=True)
        assert held.position_sum.tobytes() == whole.position_sum.tobytes()
        s.apply_delta()
        moved = s.heldout_left_to_right(off, tok, particles=2, seed=4, want_position_sums=True)
        assert moved.position_sum.tobytes() != whole.position_sum.tobytes()
        assert_equals_ref(moved, lr.evaluate(*mdl.ref_args(0), off, tok, particles=2, seed=4), "after apply_delta")
    finally:
        mdl.close()


def raw_call(s, m, particles, off, tok, outs):
    a = _lib.HeldoutArgsC(m, particles, 1, 5, 0, None, 0.0)
    st = _lib.HeldoutStatsC(-7.0, -7, -7, -7)
    rc = s.L.mvhdp_heldout_left_to_right(s.h, C.byref(a), len(off) - 1, off.ctypes.data, tok.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data,
                                          outs[2].ctypes.data, C.byref(st))
    return rc, st


def test_error_paths_leave_every_output_untouched(models):
    mdl = models(5)
    off = np.array([0, 2, 3], dtype=np.int64)
    tok = np.array([1, 2, 3], dtype=np.int32)

    def untouched(s, m, particles, off, tok, code):
        outs = [np.full(len(off) - 1, -7.0), np.full(len(tok), -7.0), np.full(len(off) - 1, -7, dtype=np.int64)]
        rc, st = raw_call(s, m, particles, off, tok, outs)
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        assert all((o == -7).all() for o in outs) and (st.log_likelihood, st.tokens, st.oov, st.visits) == (-7.0, -7, -7, -7)

    with NativeSampler(5, [150]) as fresh:                                   # no counts yet
        fresh.set_hyper(mdl.hy)
        untouched(fresh, 0, 2, off, tok, STATE)
    s = mdl.s
    untouched(s, 0, 0, off, tok, INV)                                        # particles = 0
    untouched(s, 1, 2, off, tok, INV)                                        # m = M
    untouched(s, -1, 2, off, tok, INV)
    untouched(s, 0, 2, off, np.array([1, -2, 3], dtype=np.int32), INV)       # a negative token
    untouched(s, 0, 2, np.array([0, 3, 2], dtype=np.int64), tok, INV)        # doc_off goes down
    untouched(s, 0, 2, np.array([1, 2, 3], dtype=np.int64), tok, INV)        # ... or does not start at 0
    with pytest.raises(MvhdpError) as e:
        s.heldout_left_to_right(off, tok, particles=0)
    assert e.value.code == INV and "particles" in str(e.value)
    outs = [np.full(2, -7.0), np.full(3, -7.0), np.full(2, -7, dtype=np.int64)]
    rc, st = raw_call(s, 0, 2, off, tok, outs)                               # and the same buffers with good arguments are written
    assert rc == 0 and not any((o == -7).any() for o in outs) and st.tokens == 3
    empty = s.heldout_left_to_right(np.array([0], dtype=np.int64), np.zeros(0, dtype=np.int32), want_position_sums=True)
    assert (empty.log_likelihood, empty.tokens, empty.visits, len(empty.doc_log_likelihood)) == (0.0, 0, 0, 0)


def test_group_of_two_members_equals_one_handle(models):
    mdl = models(100)
    off, tok = lc.heldout_docs(mdl.V[0], n_docs=30, seed=12)
    one = mdl.s.heldout_left_to_right(off, tok, particles=3, seed=31, want_position_sums=True)
    nwk, nk = mdl.s.get_counts(0)
    members = []
    try:
        for _ in range(2):                                                   # every member holds the full counts
            s = NativeSampler(mdl.K, mdl.V)
            s.set_hyper(mdl.hy)
            s.set_counts(0, nwk, nk)
            members.append(s)
        handed = []                                                          # what the group hands each member: (documents, doc_base)
        for s in members:
            def spy(doc_off, tokens, particles, resample, seed, m, doc_base, *rest, _call=s.heldout_left_to_right):
                handed.append((len(doc_off) - 1, int(doc_base), int(doc_off[-1]) == len(tokens)))
                return _call(doc_off, tokens, particles, resample, seed, m, doc_base, *rest)
            s.heldout_left_to_right = spy
        g = NativeGroup.__new__(NativeGroup)                                 # (no collective is needed for this: the local members, as topic_phrases)
        g.members, g.g = members, None
        two = g.heldout_left_to_right(off, tok, particles=3, seed=31, want_position_sums=True)
        assert two.position_sum.tobytes() == one.position_sum.tobytes() and two.doc_log_likelihood.tobytes() == one.doc_log_likelihood.tobytes()
        assert np.array_equal(two.doc_tokens, one.doc_tokens)
        assert (two.log_likelihood, two.tokens, two.oov, two.visits) == (one.log_likelihood, one.tokens, one.oov, one.visits)
        # the cuts the method made: contiguous, both members used, each told where its range starts, and balanced by work (sum of L^2) --
        # no cut can do better than half the work give or take the document at the cut
        (n0, base0, ok0), (n1, base1, ok1) = handed
        assert ok0 and ok1 and (base0, base1) == (0, n0) and n0 + n1 == 30 and 0 < n0 < 30
        work = np.diff(off).astype(np.float64) ** 2
        assert abs(work[:n0].sum() - work.sum() / 2) <= work.max()
        # ... and a doc_base is passed on: the second member's documents are numbered from it
        handed.clear()
        g.heldout_left_to_right(off, tok, particles=1, seed=31, doc_base=100)
        assert [h[1] for h in handed] == [100, 100 + n0]
    finally:
        for s in members:
            s.close()


# ---- the Java path: the four shim sources as one library, under the test-side JNIEnv (tests/jni_harness.py) ---------------------------
IAE = "java/lang/IllegalArgumentException"


def test_the_java_entry_equals_the_binding(jvm):
    K, V = 12, [40]
    c = synth.generate(K, V, 60, [20], seed=2)
    z = np.random.default_rng(2).integers(0, K, len(c.tokens[0])).astype(np.int32)
    hy = hyper(K, V, 2)
    off, tok = lc.heldout_docs(V[0], n_docs=10, seed=5, lengths=[0, 1, 2, 9, 20])
    D, N = len(off) - 1, len(tok)
    with NativeSampler(K, V) as s:
        s.set_corpus(0, c.doc_off[0], c.tokens[0]); s.set_assignments(0, z); s.set_hyper(hy); s.build_counts()
        want = s.heldout_left_to_right(off, tok, particles=3, seed=17, want_position_sums=True)
        scaled = hy.alpha[0, :K] * 0.5
        want_a = s.heldout_left_to_right(off, tok, particles=3, seed=17, alpha=scaled, alpha_sum=float(scaled.sum()), want_position_sums=True)
    j = H.JniSampler(jvm, K, V)
    try:
        j.setCorpus(0, c.doc_off[0], c.tokens[0])
        j.setAssignments(0, z)
        j.setHyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, None)
        h = j.handle
        joff, jtok = jvm.longs(off), jvm.ints(tok)
        with pytest.raises(H.JavaException) as e:                            # a library error becomes a RuntimeException with its text
            jvm.call("nLeftToRight", h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, None, None, None, None)
        assert e.value.cls == "java/lang/RuntimeException" and "counts" in e.value.msg
        j.buildCounts()
        jll, jps, jdt, jst = jvm.doubles(D), jvm.doubles(N), jvm.longs(D), jvm.longs(3)
        total = jvm.call("nLeftToRight", h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, jll, jps, jdt, jst)
        assert total == want.log_likelihood and list(jst.get()) == [want.tokens, want.oov, want.visits]
        assert jll.get().tobytes() == want.doc_log_likelihood.tobytes() and jps.get().tobytes() == want.position_sum.tobytes()
        assert np.array_equal(jdt.get(), want.doc_tokens)
        assert jvm.call("nLeftToRight", h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, None, None, None, None) == want.log_likelihood   # every output is optional
        assert jvm.call("nLeftToRight", h, 0, 3, 1, 17, 0, jvm.doubles(scaled), float(scaled.sum()), joff, jtok, None, jps, None, None) == want_a.log_likelihood
        assert jps.get().tobytes() == want_a.position_sum.tobytes()

        # a wrong array length is refused before the library is reached
        def refused(*args):
            with pytest.raises(H.JavaException) as e:
                jvm.call("nLeftToRight", *args)
            assert e.value.cls == IAE, e.value
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, jvm.ints(tok[:-1]), jll, jps, jdt, jst)      # tokens too short
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, jvm.ints(np.append(tok, 0)), jll, jps, jdt, jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, None, jll, jps, jdt, jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, None, jtok, jll, jps, jdt, jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, jvm.longs(0), jtok, jll, jps, jdt, jst)
        refused(h, 0, 3, 1, 17, 0, jvm.doubles(K + 1), 1.0, joff, jtok, jll, jps, jdt, jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, jvm.doubles(D + 1), jps, jdt, jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, jll, jvm.doubles(N - 1), jdt, jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, jll, jps, jvm.longs(D - 1), jst)
        refused(h, 0, 3, 1, 17, 0, None, 0.0, joff, jtok, jll, jps, jdt, jvm.longs(4))
        with pytest.raises(H.JavaException) as e:                            # particles = 0: the library's refusal
            jvm.call("nLeftToRight", h, 0, 0, 1, 17, 0, None, 0.0, joff, jtok, None, None, None, None)
        assert e.value.cls == "java/lang/RuntimeException" and "particles" in e.value.msg
    finally:
        j.close()
    for closed in (j.handle, h):                                             # a closed sampler: its handle is 0; and the jlong it had is refused too
        with pytest.raises(H.JavaException) as e:
            jvm.call("nLeftToRight", closed, 0, 3, 1, 17, 0, None, 0.0, jvm.longs(off), jvm.ints(tok), None, None, None, None)
        assert e.value.cls == "java/lang/IllegalStateException" and e.value.msg == "NativeSampler is closed"
    assert j.handle == 0 and h != 0
