"""The JNI shim (mvtopicmodel_amd/java/mvhdp_jni.cpp) driving the real library on a device, through the test-side JNIEnv of
tests/jni_harness.py and the line-by-line transcription of NativeSampler.java there.

The JNI path and the Python binding drive the same deterministic library, so every comparison here is EXACT: what a `JniSampler`
returns equals, bit for bit, what a second `NativeSampler` given the same inputs returns, and the oracle's or the restatements'
(tests/diag_numpy.py, tests/emb_ref.py, tests/mix_ref.py) wherever the existing tests compare with them.  No tolerance is introduced
(the diagnostics' doubles, the softmax table and the similarities of embNearest -- whose restatement is the numpy cosine order of
tests/test_gpu_embeddings.py, tests/emb_ref.py having none -- are compared with their restatements under the bounds tests/test_gpu_diagnostics.py and
tests/test_gpu_embeddings.py already hold them to, and bit for bit with the binding).  After every entry the harness has checked the fake JVM's ledger.  No test here closes a handle or a group while a call on
it may be running, and none injects a failure into the library: those live on the CPU side (tests/test_jni_fake_jvm.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mvtopicmodel_amd import NativeGroup, NativeSampler, _lib, synth
from mvtopicmodel_amd.java_init import init_assignments
from mvtopicmodel_amd.native import (SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY, Diagnostics, EmbConfig, Hyper)
from tests import diag_numpy as dn
from tests import emb_ref as er
from tests import jni_harness as H
from tests.helpers import make_native, make_oracle, shards_of, small_corpus
from tests.jni_harness import JavaException, JniGroup, JniSampler
from tests.mix_cases import make_ref, same_state, same_stats, table
from tests.native_build import fake_rccl  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_FIELDS = [("tokens", "tokens"), ("changed", "changed"), ("newMassCnt", "new_mass_cnt"), ("topicDocMassCnt", "topic_doc_mass_cnt"),
              ("wordFTreeMassCnt", "word_ftree_mass_cnt"), ("oovSkipped", "oov_skipped"), ("abortedDocs", "aborted_docs"),
              ("exactFallbacks", "exact_fallbacks")]
ACT_FIELDS = [("activatedTopic", "activated_topic"), ("activatedModality", "activated_modality"), ("activationKey", "activation_key"),
              ("activations", "activations")]
IAE, ISE, RTE = "java/lang/IllegalArgumentException", "java/lang/IllegalStateException", "java/lang/RuntimeException"


@pytest.fixture(scope="module")
def jni_lib(tmp_path_factory):
    _lib.load_library()
    return H.build_shim(tmp_path_factory.mktemp("jni_gpu"), _lib.LIB_PATH)


@pytest.fixture(scope="module")
def jvm(jni_lib):
    return H.Jvm(jni_lib)


class Java:
    """a JniSampler built the way the Java host builds one, read the way the state comparisons read a sampler"""

    def __init__(self, jvm, c, hy, z, doc_id_base=0, presence=None):
        self.c, self.K, self.V, self.M = c, c.K, list(c.V), c.M
        self.j = j = JniSampler(jvm, c.K, c.V, 0, doc_id_base)
        for m in range(c.M):
            j.setCorpus(m, c.doc_off[m], c.tokens[m])
            j.setAssignments(m, z[m])
        for m, present in (presence or {}).items():
            j.setViewPresence(m, present)
        self.set_hyper(hy)
        j.buildCounts()

    def set_hyper(self, hy):
        self.j.setHyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, hy.inactive)

    def get_assignments(self, m):
        return self.j.getAssignments(m, len(self.c.tokens[m]))

    def get_counts(self, m):
        return self.j.getCounts(m, self.V[m], self.K)

    def get_alpha(self):
        return self.j.getAlpha(self.M, self.K)

    def close(self):
        self.j.close()


def same_sweep_stats(js, bs, where, timing=True):
    """a SweepStats of the JNI path against the binding's: every integer equal, the two times finite and not negative"""
    for jf, bf in INT_FIELDS + ACT_FIELDS:
        assert getattr(js, jf) == getattr(bs, bf), f"{where}: {jf}: {getattr(js, jf)} != {getattr(bs, bf)}"
    if timing:
        for t in (js.sweepKernelMs, js.totalMs):
            assert np.isfinite(t) and t >= 0.0, where
        assert js.totalMs >= js.sweepKernelMs > 0.0, where


def inactive_model(M):
    K, V = 40, [600, 80, 90][:M]
    c = small_corpus(K, V, 96, [40, 1, 2][:M], 7)
    inactive = np.zeros(K, dtype=np.uint8); inactive[[33, 37]] = 1
    hy = Hyper.defaults(K, V, inactive=inactive)
    hy.alpha[:, K] = [25.0, 3.0, 7.0][:M]                       # a non-trivial alpha[m][K]: births within three sweeps
    hy.alpha[:, :K] = 0.05 + 0.01 * (np.arange(K) % 7)
    o = make_oracle(c, hy)
    z = [o.get_assignments(m) for m in range(c.M)]
    for m in range(c.M):
        z[m][np.isin(z[m], [33, 37])] = 1
    for m in range(c.M):
        o.set_assignments(m, z[m])
    o.build_counts()
    return c, hy, z, o


# ---- deferred sweeps ----
@pytest.mark.parametrize("M", [1, 3])
def test_deferred_sweeps_equal_the_binding_and_the_oracle(jvm, M):
    c, hy, z, o = inactive_model(M)
    presence = {m: np.ones(c.D, dtype=np.uint8) for m in range(1, M)}       # an empty FeatureSequence is not a missing view
    s = make_native(c, hy, z)
    for m, p in presence.items():
        s.set_view_presence(m, p)
    j = Java(jvm, c, hy, z, presence=presence)
    born = 0
    for it in range(3):
        where = f"M {M} sweep {it}"
        ro = o.sweep(it, 123)
        bs = s.sweep(it, 123)
        js = j.j.sweep(it, 123, 0, None)
        same_sweep_stats(js, bs, where)
        same_stats(ro["stats"], bs, where)                     # (the binding against the oracle, as everywhere; so the JNI path too)
        assert js.tokens == c.total_tokens
        same_state(o, j, c.M, where + " (oracle)")
        same_state(s, j, c.M, where + " (binding)")
        (ja, ji), (ba, bi) = j.get_alpha(), s.get_alpha()
        assert np.array_equal(ja, ba) and np.array_equal(ji, bi), where
        assert np.array_equal(ja, o.get_alpha()) and np.array_equal(ji, o.get_inactive()), where
        born += js.activatedTopic >= 0
    assert born >= 1
    # the statistics that read the view presence
    if M > 1:
        assert np.array_equal(j.j.viewOverlapSums(M).reshape(M, M), s.view_overlap_sums())
        assert np.array_equal(j.j.modelLogLikelihood(M), s.model_log_likelihood())
        for m in range(M):
            assert tuple(j.j.gammaDocStatistics(m, 1.5, 9, 2)) == s.gamma_doc_statistics(m, 1.5, 9, 2)
        j.j.setViewPresence(1, None); s.set_view_presence(1, None)            # back to "present iff the span is non-empty"
        assert np.array_equal(j.j.viewOverlapSums(M).reshape(M, M), s.view_overlap_sums())
    s.close(); j.close(); o.close()


def test_view_weights_handed_in_equal_the_ones_drawn_on_the_device(jvm):
    c, hy, z, o = inactive_model(3)
    s = make_native(c, hy, z)
    s.sweep(0, 5)
    p = s.get_view_weights()                                   # [D][M][M] as the device drew them for (seed 5, sweep 0)
    j = Java(jvm, c, hy, z)
    js = j.j.sweep(0, 5, 0, p.ravel())
    ro = o.sweep(0, 5, p=p)
    same_state(s, j, c.M, "pOverride (binding, drawn on the device)")
    same_state(o, j, c.M, "pOverride (oracle, the same weights)")
    assert (js.tokens, js.changed, js.newMassCnt) == (ro["stats"]["tokens"], ro["stats"]["changed"], ro["stats"]["new_mass_cnt"])
    t = make_native(c, hy, z)
    p2 = np.full((c.D, c.M, c.M), 0.5); p2[:, np.arange(c.M), np.arange(c.M)] = 1.0
    bs = t.sweep(1, 5, p=p2)
    j2 = Java(jvm, c, hy, z)
    same_sweep_stats(j2.j.sweep(1, 5, 0, p2.ravel()), bs, "pOverride of the host's own")
    same_state(t, j2, c.M, "pOverride of the host's own")
    with pytest.raises(JavaException) as e:
        j2.j.sweep(2, 5, 0, p2.ravel()[:-1])
    assert e.value.cls == IAE and "pOverride" in e.value.msg
    for x in (s, t, j, j2, o):
        x.close()


def test_sweep_many_and_no_apply_with_apply_delta_equal_plain_sweeps(jvm):
    c, hy, z, o = inactive_model(3)
    s = make_native(c, hy, z)
    want = [s.sweep(it, 77) for it in range(4)]
    j = Java(jvm, c, hy, z)
    got = j.j.sweepMany(0, 4, 77, 0)
    for it in range(4):
        for jf, bf in INT_FIELDS:
            assert getattr(got[it], jf) == getattr(want[it], bf), (it, jf)
    same_state(s, j, c.M, "sweepMany(4)")
    assert np.array_equal(j.get_alpha()[0], s.get_alpha()[0]) and np.array_equal(j.get_alpha()[1], s.get_alpha()[1])
    k = Java(jvm, c, hy, z)
    for it in range(4):
        st = k.j.sweep(it, 77, SWEEP_NO_APPLY, None)
        assert (st.activatedTopic, st.activatedModality) == (want[it].activated_topic, want[it].activated_modality)
        k.j.applyDelta(st.activatedTopic, st.activatedModality)
        k.j.buildTrees()
    same_state(s, k, c.M, "NO_APPLY + applyDelta")
    assert np.array_equal(k.get_alpha()[0], s.get_alpha()[0]) and np.array_equal(k.get_alpha()[1], s.get_alpha()[1])
    for x in (s, j, k, o):
        x.close()


# ---- the statistics either side of the sweep ----
def test_statistics_entries_equal_the_binding_and_the_oracle(jvm):
    c, hy, z, o = inactive_model(3)
    s = make_native(c, hy, z)
    j = Java(jvm, c, hy, z)
    for it in range(2):
        o.sweep(it, 31); s.sweep(it, 31); j.j.sweep(it, 31, 0, None)
    K, M = c.K, c.M
    maxlen = int(max(np.diff(c.doc_off[m]).max() for m in range(M))) + 1
    for m in range(M):
        jh = j.j.getCountHistogram(m, 64)
        assert np.array_equal(jh, s.get_count_histogram(m, 64)) and np.array_equal(jh, o.count_histogram(m, 64))
        hist, lens = j.j.getDocTopicHist(m, K, maxlen, maxlen)
        bh, bl = s.get_doc_topic_hist(m, maxlen, maxlen)
        oh, ol = o.get_doc_topic_hist(m, maxlen, maxlen)
        assert np.array_equal(hist, bh) and np.array_equal(lens, bl)
        assert np.array_equal(hist, oh) and np.array_equal(lens, np.asarray(ol)[:maxlen])
        hist2, none = j.j.getDocTopicHist(m, K, maxlen)        # without docLengthCounts
        assert none is None and np.array_equal(hist2, hist)
        assert tuple(j.j.gammaDocStatistics(m, float(hy.gamma[m]), 5, 1)) == s.gamma_doc_statistics(m, float(hy.gamma[m]), 5, 1)
        conc = hy.gamma[m] * j.get_alpha()[0][m][:K]
        mk, act = j.j.dpTableStatistics(m, hist.ravel(), maxlen, conc, 17, 3, K)
        bmk, bact = s.dp_table_statistics(m, bh, conc, 17, 3)
        assert np.array_equal(mk, bmk) and np.array_equal(act.astype(np.uint8), bact)
        assert mk.sum() > 0
    assert np.array_equal(j.j.viewOverlapSums(M).reshape(M, M), s.view_overlap_sums())
    jl = j.j.modelLogLikelihood(M)
    assert np.array_equal(jl, s.model_log_likelihood()) and np.all(np.isfinite(jl)) and np.all(jl < 0)
    for x in (s, j, o):
        x.close()


# ---- diagnostics ----
def as_binding_diagnostics(d, K, N):
    R = _lib.DIAG_ROWS
    sc, ws = d.scores.get().reshape(len(R), K), d.wordScores.get().reshape(len(R), K, N)
    return Diagnostics(scores={n: sc[i] for i, n in enumerate(R)}, word_scores={n: ws[i] for i, n in enumerate(R)},
                       codoc=d.codoc.get().reshape(K, N, N), top_words=d.topTypes.get().reshape(K, N), top_counts=d.topCounts.get().reshape(K, N),
                       nonzero=d.nonzero.get(), num_rank1_docs=d.numRank1Documents.get(), num_nonzero_docs=d.numNonZeroDocuments.get(),
                       num_docs_at_proportions=d.numDocumentsAtProportions.get().reshape(K, 7), sum_count_log_count=d.sumCountLogCount.get(),
                       word_type_counts=d.wordTypeCounts.get(), num_tokens=int(d.numTokens.get()[0]), discr_weight_per_view=d.discrWeightPerModality.get())


def same_diagnostics(a, b, where):
    """two Diagnostics of the same library on the same state: every array the same bits (NaN where the other has NaN)"""
    for f in ("codoc", "top_words", "top_counts", "nonzero", "num_rank1_docs", "num_nonzero_docs", "num_docs_at_proportions", "sum_count_log_count",
              "word_type_counts", "discr_weight_per_view"):
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), f"{where}: {f}"
    assert a.num_tokens == b.num_tokens
    for n in _lib.DIAG_ROWS:
        assert np.array_equal(a.scores[n], b.scores[n], equal_nan=True), f"{where}: {n}"
        assert np.array_equal(a.word_scores[n], b.word_scores[n], equal_nan=True), f"{where}: {n} words"


def test_diagnostics_entries_equal_the_binding_and_the_numpy_restatement(jvm):
    from tests.test_gpu_diagnostics import assert_matches, reference
    c, hy, z, o = inactive_model(3)
    s = make_native(c, hy, z); s._hy = hy
    j = Java(jvm, c, hy, z)
    for it in range(2):
        s.sweep(it, 31); j.j.sweep(it, 31, 0, None)
    K, M, N = c.K, c.M, 7
    for m in range(M):
        t, cnt, nz = j.j.topWords(m, N + m, K)                 # (n differs from m in every call: exchanged arguments would show)
        rt, rc, rz = dn.top_words(s.get_counts(m)[0], N + m)
        assert np.array_equal(t, rt) and np.array_equal(cnt, rc) and np.array_equal(nz, rz), f"top words of view {m}"
        bt, bc, bz = s.top_words(m, N + m)
        assert np.array_equal(t, bt) and np.array_equal(cnt, bc) and np.array_equal(nz, bz)
        pv, tw = j.j.discrWeights(M, m, c.V[m])
        bpv, btw = s.discr_weights(m)
        assert np.array_equal(pv, bpv) and np.array_equal(tw, btw) and np.array_equal(tw, dn.type_discr_weight(s.get_counts(m)[0]))
    pv, none = j.j.discrWeights(M, 0)
    assert none is None and np.array_equal(pv, s.discr_weights())
    wl = (np.arange(c.V[0]) % 11 + 1).astype(np.int32)
    for word_length in (None, wl):
        d = as_binding_diagnostics(j.j.diagnostics(K, c.V[0], M, N, word_length), K, N)
        same_diagnostics(d, s.diagnostics(num_top_words=N, word_length=word_length), f"wordLength {word_length is not None}")
        nwk0, nk0 = s.get_counts(0)
        assert_matches(d, reference(s, N, c.doc_off[0], c.tokens[0], word_length), nwk0, nk0)
        assert np.all(np.isnan(d.scores["word-length"])) == (word_length is None)
    for x in (s, j, o):
        x.close()


# ---- embeddings ----
def emb_corpus(V0, K, seed):
    rng = np.random.default_rng(seed)
    lens = [0, 4, 8, 30, 12, 45, 2, 60, 25, 300, 33]
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(doc_off[-1])
    return doc_off, rng.integers(0, V0, n).astype(np.int32), rng.integers(0, K, n).astype(np.int32)


@pytest.mark.parametrize("topics", [True, False], ids=["topics", "words_only"])
def test_embedding_entries_equal_the_restatement_bit_for_bit(jvm, topics):
    K, V0, C = 3, 120, 16
    doc_off, tok, z = emb_corpus(V0, K, 5)
    cfg = EmbConfig.defaults(with_topics=topics, num_columns=C, num_context_columns=4 if topics else 0, sampling_table_size=10 ** 5, sampling_factor=0.3)
    jc = H.EmbConfig(numColumns=C, numContextColumns=cfg.num_context_columns, withTopics=topics, samplingTableSize=10 ** 5, samplingFactor=0.3)
    R = V0 + (K if topics else 0)
    given = np.random.default_rng(1).uniform(-0.5, 0.5, (R, C)) / C
    ref = er.EmbRef(V0, K, cfg, weights=given)
    j = JniSampler(jvm, K, [V0])
    j.setCorpus(0, doc_off, tok); j.setAssignments(0, z)
    with pytest.raises(JavaException) as e:
        j.embCountWords()                                      # before embInit: the library's own refusal
    assert e.value.cls == RTE and "(-2)" in e.value.msg
    j.embInit(jc, given.ravel(), 5)
    w, n = j.embGetVectors(R * C)
    assert np.array_equal(w.reshape(R, C), given) and not n.any()
    for rnd, epochs in ((0, 1), (1, 2)):
        j.embCountWords(); ref.count_words(tok)
        st = j.embTrain(epochs, 123, rnd, JniSampler.EMB_SERIAL)
        rs = ref.train(doc_off, tok, z if topics else None, epochs, seed=123, round_idx=rnd)
        assert (st.wordsSoFar, st.wordsSampled, st.wordsConsidered, st.docsSkipped, st.calls, st.negativesSkipped) == \
               (rs["words"], rs["sampled"], rs["considered"], rs["skipped"], rs["calls"], rs["negskip"])
        assert (st.residual, st.lastEpochResidual, st.lastEpochCalls) == (rs["residual"], rs["last_residual"], rs["last_calls"])
        assert st.wordsSoFar == epochs * len(tok) and np.isfinite(st.kernelMs) and st.kernelMs >= 0
        w, n = j.embGetVectors(R * C)
        assert np.array_equal(w.reshape(R, C), ref.w) and np.array_equal(n.reshape(R, C), ref.neg), f"round {rnd}"
    only_w, none = j.embGetVectors(R * C, want_negative=False)
    assert none is None and np.array_equal(only_w, w)
    counts, retention, total = j.embWordStats(V0)
    assert np.array_equal(counts, ref.counts) and np.array_equal(retention, ref.retention) and total == ref.total == 2 * len(tok)
    assert j.embWordStats(V0, want_counts=False, want_retention=False) == (None, None, total)
    for first, cnt in ((0, 257), (10 ** 5 - 100, 100), (31337, 1)):
        assert np.array_equal(j.embSamplingTable(first, cnt), ref.table_range(first, cnt))
    # set / get: the vectors of another state go in and come out, and training goes on from them
    w2 = ref.w[::-1].copy(); n2 = ref.neg * 0.5
    j.embSetVectors(w2.ravel(), n2.ravel())
    ref.w[:], ref.neg[:] = w2, n2
    j.embSetVectors(None, None)                                # (both null: nothing changes)
    w, n = j.embGetVectors(R * C)
    assert np.array_equal(w.reshape(R, C), w2) and np.array_equal(n.reshape(R, C), n2)
    # a second handle of the binding holding the same vectors
    b = NativeSampler(K, [V0]); b.set_corpus(0, doc_off, tok); b.set_assignments(0, z)
    b.emb_init(cfg, weights=w2); b.emb_set_vectors(w2, n2)
    if topics:
        for reset in (True, False, False):                     # the sums accumulate over calls (PTM:360)
            e_, S_ = j.embSoftmax(reset, K * V0, K)
            be, bS = b.emb_softmax(reset_sums=reset)
            assert np.array_equal(e_.reshape(K, V0), be) and np.array_equal(S_, bS)           # the binding: bit for bit
            re_, rS = ref.softmax(reset_sums=reset)            # the restatement: under the bounds of tests/test_gpu_embeddings.py
            np.testing.assert_allclose(e_.reshape(K, V0), re_, rtol=1e-14, atol=0)
            np.testing.assert_allclose(S_, rS, rtol=1e-12, atol=0)
        none, S_ = j.embSoftmax(False, None, K)
        assert none is None and np.array_equal(S_, b.emb_softmax(want_exp=False)[1])
    else:
        # no topic rows (embK = 0): the shim asks for EMPTY arrays (a [K*V_0] one is refused), and the library has nothing to take a
        # softmax of: its MVHDP_ERR_STATE comes back as the RuntimeException
        with pytest.raises(JavaException) as e:
            j.embSoftmax(True, K * V0, K)
        assert e.value.cls == IAE and "embSoftmax expDot" in e.value.msg
        with pytest.raises(JavaException) as e:
            j.embSoftmax(True, 0, 0)
        assert e.value.cls == RTE and "mvhdp_emb_softmax failed (-2)" in e.value.msg
    # findClosest
    q = w2[7] + 0.25 * w2[11]
    words, sims, tps, tsims = j.embNearest(q, 9, want_topics=topics)
    bw, bs_, bt, bts = b.emb_nearest(q, 9)
    assert np.array_equal(words, bw) and np.array_equal(sims, bs_) and words[0] == 7
    # the cosine order restated with numpy, as tests/test_gpu_embeddings.py::test_nearest_in_idsorter_order does (its bound for the values)
    cos = (w2 @ q) * (1.0 / np.sqrt(q @ q)) * (1.0 / np.sqrt((w2 * w2).sum(1)))
    order = sorted(range(V0), key=lambda i: (-cos[i], -i))[:9]
    assert list(words) == order
    np.testing.assert_allclose(sims, cos[order], rtol=1e-12)
    if topics:
        assert np.array_equal(tps, bt) and np.array_equal(tsims, bts, equal_nan=True) and list(tps[K:]) == [-1] * (9 - K)
        torder = sorted(range(K), key=lambda i: (-cos[V0 + i], -i))
        assert list(tps[:K]) == torder and np.isnan(tsims[K:]).all()
        np.testing.assert_allclose(tsims[:K], cos[V0 + np.array(torder)], rtol=1e-12)
    # a refused configuration leaves the embedding, and the shim's idea of its shape, as they were; release ends it
    with pytest.raises(JavaException) as e:
        j.embInit(H.EmbConfig(numColumns=0), None, 1)
    assert e.value.cls == RTE and "(-1)" in e.value.msg
    w, _ = j.embGetVectors(R * C)
    assert np.array_equal(w.reshape(R, C), w2)
    j.embRelease()
    with pytest.raises(JavaException) as e:
        j.embGetVectors(R * C)
    assert e.value.cls == ISE
    j.close(); b.close()


def test_vectors_mix_from_host_arrays_and_from_the_device_table(jvm):
    K, V = 30, [300, 40]
    c = small_corpus(K, V, 64, [30, 4], 31)
    hy = Hyper.defaults(K, V)
    e, S = table(K, V[0], 7)
    r = make_ref(c, hy)                                        # tests/mix_ref.py
    z = [r.get_assignments(m) for m in range(c.M)]
    s = make_native(c, hy, z)
    j = Java(jvm, c, hy, z)
    assert j.j.getVectorsMix(None) == (0.0, None)
    with pytest.raises(JavaException) as ex:
        j.j.getVectorsMix(V[0] * K)                            # off: the library's MVHDP_ERR_STATE
    assert ex.value.cls == RTE and "(-2)" in ex.value.msg
    r.set_vectors_mix(0.25, e, S); s.set_vectors_mix(0.25, e, S); j.j.setVectorsMix(0.25, e.ravel(), S)
    lam, mix = j.j.getVectorsMix(V[0] * K)
    blam, bmix = s.get_vectors_mix()
    assert lam == blam == 0.25 and np.array_equal(mix.reshape(V[0], K), bmix)
    for it in range(3):
        rr = r.sweep(it, 0xC0FFEE)
        bs = s.sweep(it, 0xC0FFEE)
        js = j.j.sweep(it, 0xC0FFEE, 0, None)
        same_stats(rr["stats"], bs, f"mixed sweep {it}")
        same_sweep_stats(js, bs, f"mixed sweep {it}")
        same_state(r, j, c.M, f"mixed sweep {it} (mix_ref)")
        same_state(s, j, c.M, f"mixed sweep {it} (binding)")
    # the table the last embSoftmax left on the device: both arrays null
    cfg = EmbConfig.defaults(num_columns=16, num_context_columns=4, sampling_table_size=10 ** 5, min_doc_length=2)
    jc = H.EmbConfig(numColumns=16, numContextColumns=4, samplingTableSize=10 ** 5, minDocLength=2)
    s.emb_init(cfg, seed=5); s.emb_count_words(); s.emb_train(1, seed=9, serial=True)
    j.j.embInit(jc, None, 5); j.j.embCountWords(); j.j.embTrain(1, 9, 0, JniSampler.EMB_SERIAL)
    be, bS = s.emb_softmax(reset_sums=True)
    je, jS = j.j.embSoftmax(True, K * V[0], K)
    assert np.array_equal(je.reshape(K, V[0]), be) and np.array_equal(jS, bS)
    s.set_vectors_mix(0.5); j.j.setVectorsMix(0.5, None, None)
    lam, mix = j.j.getVectorsMix(V[0] * K)
    assert lam == 0.5 and np.array_equal(mix.reshape(V[0], K), s.get_vectors_mix()[1])
    t = make_native(c, hy, [s.get_assignments(m) for m in range(c.M)])
    t.set_vectors_mix(0.5, be, bS)                             # ... equals handing the same arrays in
    assert np.array_equal(t.get_vectors_mix()[1], mix.reshape(V[0], K))
    same_sweep_stats(j.j.sweep(3, 1, 0, None), t.sweep(3, 1), "sweep with the device's table")
    same_state(t, j, c.M, "sweep with the device's table")
    j.j.setVectorsMix(0.0, None, None)
    assert j.j.getVectorsMix(None) == (0.0, None)
    for x in (r, s, t, j):
        x.close()


# ---- tuning ----
def births_model():
    """the corpus of tests/test_gpu_live.py::test_a_live_sweep_gives_birth_to_topics_chunk_by_chunk"""
    K, V = 60, [500, 60]
    c = small_corpus(K, V, 400, [40, 6], 45)
    inactive = np.zeros(K, dtype=np.uint8); inactive[40:] = 1
    hy = Hyper.defaults(K, V, inactive=inactive); hy.alpha[:, K] = 50.0
    o = make_oracle(c, hy)
    z = [o.get_assignments(m) for m in range(c.M)]
    for m in range(c.M):
        z[m][z[m] >= 40] = 7
    o.close()
    return c, hy, z


def test_set_tuning_of_get_tuning_keeps_the_live_rows_form(jvm):
    """setTuning(getTuning()) is what INTEGRATION.md tells a host to do to hand a learnt walk threshold to a shard.  A JniSampler
    that has done it gives birth, in one one-segment live sweep, to as many topics as a handle whose tuning was never touched (>= 8 on
    this corpus: that test's own threshold); the stored-tree form gives exactly one.  With nSetTuning zero-filling the struct the
    sampler fell back to the stored-tree form: 1 birth."""
    c, hy, z = births_model()
    flags = SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(1)
    s = make_native(c, hy, z)
    untouched = s.sweep(0, 5, flags=flags).activations
    before = s.get_tuning()
    s.close()
    j = Java(jvm, c, hy, z)
    j.j.setTuning(j.j.getTuning())
    js = j.j.sweep(0, 5, flags, None)
    assert untouched >= 8
    assert js.activations == untouched, f"{js.activations} births after setTuning(getTuning()), {untouched} with the tuning never touched"
    assert int(j.get_alpha()[1].sum()) == 20 - untouched
    # what the Java block does carry arrives: a pinned walk threshold comes back from getTuning
    tu = j.j.getTuning()
    assert (tu.forcePrimary, tu.narrow, tu.live16) == (before.force_primary, before.narrow, before.live16)
    tu.walkFixed, tu.walkTheta = 1, [0.5, 0.25] + [0.0] * 6
    j.j.setTuning(tu)
    back = j.j.getTuning()
    assert back.walkFixed == 1 and back.walkTheta[:2] == [0.5, 0.25]
    tu.forcePrimary = 3
    with pytest.raises(JavaException) as e:
        j.j.setTuning(tu)
    assert e.value.cls == RTE and "force_primary" in e.value.msg
    j.close()
    k = make_native(c, hy, z)
    k.set_tuning(live_rows=0)
    assert k.sweep(0, 5, flags=flags).activations == 1         # the stored-tree form: one birth per segment border
    k.close()


# ---- groups ----
def test_a_group_of_two_members_in_one_process_equals_the_single_handle(jvm):
    from tests.test_gpu_diagnostics import assert_matches, reference
    K, V = 48, [700, 90, 70]
    c = synth.generate(K, V, 260, [40, 5, 6], 97, chunk_docs=4096)
    z = init_assignments(K, c.doc_off, seed=1)
    hy = Hyper.defaults(K, V)
    M = c.M
    single = make_native(c, hy, z); single._hy = hy
    members = [Java(jvm, sub, hy, zs, doc_id_base=lo) for lo, sub, zs in shards_of(c, z, 2)]
    g = JniGroup(jvm, [m.j for m in members])
    g.buildCounts()
    for mem in members:
        for m in range(M):
            assert np.array_equal(mem.get_counts(m)[0], single.get_counts(m)[0])
    for it in range(2):
        want = single.sweep(it, 11)
        sts = g.sweep(it, 11, 0)
        assert len(sts) == 2 and sum(st.tokens for st in sts) == want.tokens == c.total_tokens
        assert sum(st.changed for st in sts) == want.changed
        for st in sts:
            assert (st.activatedTopic, st.activatedModality, st.activations) == (want.activated_topic, want.activated_modality, want.activations)
            assert np.isfinite(st.totalMs) and st.totalMs >= 0.0             # the exchange's milliseconds
    for m in range(M):
        zcat = np.concatenate([mem.get_assignments(m) for mem in members])
        assert np.array_equal(zcat, single.get_assignments(m)), f"z of view {m}"
        for mem in members:
            assert np.array_equal(mem.get_counts(m)[0], single.get_counts(m)[0]) and np.array_equal(mem.get_counts(m)[1], single.get_counts(m)[1])
    # the five group statistics and the diagnostics against the single handle
    maxlen = int(max(np.diff(c.doc_off[m]).max() for m in range(M))) + 1
    assert np.array_equal(g.modelLogLikelihood(M), single.model_log_likelihood())
    assert np.array_equal(g.viewOverlapSums(M).reshape(M, M), single.view_overlap_sums())
    for m in range(M):
        hist, lens = g.getDocTopicHist(m, K, maxlen, maxlen)
        sh, sl = single.get_doc_topic_hist(m, maxlen, maxlen)
        assert np.array_equal(hist, sh) and np.array_equal(lens, sl)
        assert np.array_equal(g.getDocTopicHist(m, K, maxlen)[0], sh)
        assert np.array_equal(g.getCountHistogram(m, 64), single.get_count_histogram(m, 64))
        assert tuple(g.gammaDocStatistics(m, 1.0, 5, 0)) == single.gamma_doc_statistics(m, 1.0, 5, 0)
    N = 6
    wl = (np.arange(V[0]) % 9 + 2).astype(np.int32)
    d = as_binding_diagnostics(g.diagnostics(K, V[0], M, N, wl), K, N)
    nwk0, nk0 = single.get_counts(0)
    assert_matches(d, reference(single, N, c.doc_off[0], c.tokens[0], wl), nwk0, nk0)
    sd = single.diagnostics(num_top_words=N, word_length=wl)
    for f in ("codoc", "top_words", "top_counts", "nonzero", "num_rank1_docs", "num_nonzero_docs", "num_docs_at_proportions", "word_type_counts"):
        assert np.array_equal(getattr(d, f), getattr(sd, f)), f
    assert d.num_tokens == sd.num_tokens
    # live sweeps with the exchange beside the next sweep, then drain: every replica is the count of the assignments again
    for it in (2, 3):
        g.sweep(it, 11, SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(1) | 0x100)
    g.drain()
    for m in range(M):
        zcat = np.concatenate([mem.get_assignments(m) for mem in members])
        want = np.zeros((V[m], K), dtype=np.int64)
        np.add.at(want, (c.tokens[m], zcat), 1)
        for mem in members:
            assert np.array_equal(mem.get_counts(m)[0].astype(np.int64), want)
    # abort: the next sweep fails (on every member together), a recount recovers
    g.abort()
    with pytest.raises(JavaException) as e:
        g.sweep(4, 11, 0)
    assert e.value.cls == RTE and "mvhdp_group_sweep failed" in e.value.msg
    g.buildCounts()
    assert sum(st.tokens for st in g.sweep(5, 11, 0)) == c.total_tokens
    with pytest.raises(JavaException) as e:
        JniGroup(jvm, [members[0].j, members[0].j])            # the library's refusal comes back with its message
    assert e.value.cls == RTE and "mvhdp_group_create failed" in e.value.msg
    g.close()
    for x in members + [single]:
        x.close()


def test_two_rank_processes_through_the_shim_equal_the_single_handle(tmp_path, jni_lib, fake_rccl):
    """nGroupUniqueId and nGroupCreateRank, which only a rank process can reach: two fresh processes on one device over
    tests/native/fake_rccl.c, each driving its shard through the shim (tests/jni_rank_worker.py)."""
    from tests import jni_rank_worker as W
    env = dict(os.environ, MVHDP_RCCL_LIB=fake_rccl, FAKE_RCCL_TIMEOUT_MS="20000")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "jni_rank_worker.py"), str(tmp_path), str(r), "2", jni_lib],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
    logs = [json.load(open(os.path.join(str(tmp_path), f"rank{r}.json"))) for r in range(2)]
    arrs = [dict(np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))) for r in range(2)]
    c, z = W.corpus()
    single = make_native(c, W.hyper(), z)
    want = [single.sweep(it, W.SEED) for it in range(2)]
    for it in range(2):
        assert sum(lg["sweeps"][it]["tokens"] for lg in logs) == want[it].tokens
        assert sum(lg["sweeps"][it]["changed"] for lg in logs) == want[it].changed
        assert all(np.isfinite(lg["sweeps"][it]["exchange_ms"]) and lg["sweeps"][it]["exchange_ms"] >= 0 for lg in logs)
    for m in range(c.M):
        assert np.array_equal(np.concatenate([a[f"z{m}"] for a in arrs]), single.get_assignments(m)), f"z of view {m}"
        for a in arrs:
            assert np.array_equal(a[f"nwk{m}"], single.get_counts(m)[0]) and np.array_equal(a[f"nk{m}"], single.get_counts(m)[1])
    # modelLogLikelihood: across processes the ranks' document sums are added in rank order, so a rank's value equals the single
    # handle's to rounding only ("Statistics of a sharded model"); the exact reference is the Python binding as the same
    # rank of a group of the same sharding over the same state, which the worker forms after the shim's group has closed
    assert np.array_equal(arrs[0]["ll"], arrs[1]["ll"]) and np.all(np.isfinite(arrs[0]["ll"])) and np.all(arrs[0]["ll"] < 0)
    for a in arrs:
        assert np.array_equal(a["ll"], a["ll_binding"]), (a["ll"].tolist(), a["ll_binding"].tolist())
    assert all(lg["ledger_checked"] > 10 for lg in logs)
    single.close()
