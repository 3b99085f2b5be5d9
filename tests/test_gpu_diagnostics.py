"""mvhdp_top_words / mvhdp_discr_weights / mvhdp_diagnostics (FastQMVWVTopicModelDiagnostics on the device) against the numpy
restatement tests/diag_numpy.py.  Integers and typeDiscrWeight bit for bit; the other doubles to 1e-10 relative (the signed sums of
uniform_dist / corpus_dist to 1e-12 of the sum of the absolute terms); NaN / Inf at the same places."""
import ctypes as C
import os

import numpy as np
import pytest

from mvtopicmodel_amd import NativeSampler, synth
from mvtopicmodel_amd._lib import DIAG_ROWS, DiagArgsC, DiagOutC, MvhdpError
from mvtopicmodel_amd.java_init import init_assignments
from mvtopicmodel_amd.native import Hyper, SWEEP_LIVE, java_string_lengths
from tests import diag_numpy as dn
from tests import test_diag_kats as kat
from tests.helpers import make_native, small_corpus, untouched

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SIGNED = ("uniform_dist", "corpus_dist")


def reference(s, N, doc_off0, tokens0, word_length=None):
    nwk = [s.get_counts(m)[0] for m in range(s.M)]
    nk0 = s.get_counts(0)[1]
    alpha, _ = s.get_alpha()
    hy = s._hy
    return dn.diagnostics(nwk, nk0, alpha[0], float(hy.gamma[0]), float(hy.alpha_sum[0]), float(hy.beta[0]),
                          doc_off0, tokens0, s.get_assignments(0), N, word_length)


def _same_special(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN places differ"
    assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), f"{what}: Inf places differ"
    return np.isfinite(a) & np.isfinite(b)


def assert_matches(d, ref, nwk0=None, nk0=None):
    N = ref["top_types"].shape[1]
    assert np.array_equal(d.top_words, ref["top_types"])
    assert np.array_equal(d.top_counts, ref["top_counts"])
    assert np.array_equal(d.nonzero, ref["nonzero"])
    assert np.array_equal(d.codoc, ref["codoc"])
    assert np.array_equal(d.num_rank1_docs, ref["num_rank1_docs"])
    assert np.array_equal(d.num_nonzero_docs, ref["num_nonzero_docs"])
    assert np.array_equal(d.num_docs_at_proportions, ref["num_docs_at_proportions"])
    assert np.array_equal(d.word_type_counts, ref["word_type_counts"])
    assert d.num_tokens == ref["num_tokens"]
    np.testing.assert_allclose(d.sum_count_log_count, ref["sum_count_log_count"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(d.discr_weight_per_view, ref["discr_weight_per_view"], rtol=1e-10, atol=0)
    for name in DIAG_ROWS:
        for got, want, what in ((d.scores[name], ref["scores"][name], name), (d.word_scores[name][:, :N], ref["word_scores"][name], name + " words")):
            fin = _same_special(got, want, what)
            if name in SIGNED and not what.endswith("words"):
                scale = dn.uniform_abs_sum(nwk0, nk0) if name == "uniform_dist" else dn.corpus_abs_sum(nwk0, nk0, ref["word_type_counts"], ref["num_tokens"])
                err = np.abs(got - want)[fin]
                assert np.all(err <= 1e-12 * scale[fin] + 1e-300), (name, err.max())
            else:
                np.testing.assert_allclose(got[fin], want[fin], rtol=1e-10, atol=0, err_msg=what)


def check(s, N, doc_off0, tokens0, vocabulary=None):
    wl = None if vocabulary is None else java_string_lengths(vocabulary)
    d = s.diagnostics(num_top_words=N, vocabulary=vocabulary)
    ref = reference(s, N, doc_off0, tokens0, wl)
    nwk0, nk0 = s.get_counts(0)
    assert_matches(d, ref, nwk0, nk0)
    pv, tw = s.discr_weights(0)
    assert np.array_equal(tw, ref["type_discr_weight0"])                   # one division of two exact integer sums
    for m in range(s.M):
        t, c, z = s.top_words(m, N)
        rt, rc, rz = dn.top_words(s.get_counts(m)[0], N)
        assert np.array_equal(t, rt) and np.array_equal(c, rc) and np.array_equal(z, rz), f"top words of view {m}"
    return d


def _keep_hyper(s, hy):
    s.set_hyper(hy)
    s._hy = hy


def native_from(c, hy, z):
    s = make_native(c, hy, z)
    s._hy = hy
    return s


# ---------------------------------------------------------------------------------------------------------------
def kat_sampler():
    K = kat.K
    V = [4, 2, 2]
    s = NativeSampler(K, V)
    s.set_corpus(0, kat.DOC_OFF, kat.TOKENS)
    s.set_assignments(0, kat.Z)
    empty = np.zeros(len(kat.DOC_OFF), np.int64)
    for m in (1, 2):
        s.set_corpus(m, empty, np.zeros(0, np.int32))
    s.set_view_presence(0, np.array([1, 1, 1, 1, 0], np.uint8))           # entity 3: view 0 present and empty; entity 4: absent
    hy = Hyper.defaults(K, V)
    hy.alpha[0] = kat.ALPHA0
    hy.alpha_sum[0] = 1.0
    _keep_hyper(s, hy)
    s.build_counts()
    s.set_counts(1, kat.NWK1, kat.NWK1.sum(axis=0))
    s.set_counts(2, kat.NWK2, kat.NWK2.sum(axis=0))
    return s


def test_hand_built_model_known_answers():
    with kat_sampler() as s:
        d = s.diagnostics(num_top_words=kat.N, word_length=kat.WORD_LENGTH)
        ref = kat._run()
        assert d.top_words.tolist() == [[1, 0, -1], [2, 3, 1], [-1, -1, -1]]
        assert d.codoc[0].tolist() == [[1, 1, 1], [1, 2, 2], [1, 2, 2]]
        assert d.num_rank1_docs.tolist() == [2, 1, 0]
        assert d.num_tokens == 8
        assert_matches(d, ref, kat.NWK0, kat.NK0)
        pv = s.discr_weights()
        np.testing.assert_allclose(pv, [32 / 45, 13 / 18, 25 / 36], rtol=1e-15)
        assert s.discr_weights(1)[1].tolist() == [0.5, 1.0]
        assert np.isnan(d.scores["rank_1_docs"][2]) and d.scores["eff_num_words"][2] == np.inf


GOLDEN = ["m3_k20", "m1_k100", "m3_k100_inactive", "m5_k1000_powerlaw"]


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("N", [1, 20, 49, 64])
def test_goldens(name, N):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    K, V = int(g["K"]), [int(v) for v in g["V"]]
    hy = Hyper(alpha=g["alpha"], alpha_sum=g["alpha_sum"], beta=g["beta"], beta_sum=g["beta_sum"], gamma=g["gamma"],
               p_a=g["p_a"], p_b=g["p_b"], inactive=g["inactive"])
    with NativeSampler(K, V) as s:
        for m in range(len(V)):
            s.set_corpus(m, g[f"doc_off{m}"], g[f"tokens{m}"])
            s.set_assignments(m, g[f"z3_{m}"])
        _keep_hyper(s, hy)
        s.build_counts()
        check(s, N, g["doc_off0"], g["tokens0"])


def test_c1_sms_fixture_with_its_vocabulary():
    f = np.load(os.path.join(HERE, "golden", "c1_smsspam.npz"))
    doc_off, tokens, vocab = f["doc_off"], f["tokens"], [str(w) for w in f["vocab"]]
    K, V = 50, [len(vocab)]
    z = init_assignments(K, [doc_off], seed=3)
    c = synth.Corpus(K, V, [doc_off], [tokens], "C1")
    hy = Hyper.defaults(K, V)
    with native_from(c, hy, z) as s:
        for it in range(3):
            s.sweep(it, 21)
        check(s, 20, doc_off, tokens, vocabulary=vocab)


@pytest.mark.parametrize("K", [5, 64, 300, 2048])
def test_small_corpora_over_topic_counts(K):
    V = [900, 60, 40]
    c = small_corpus(K, V, 240, [60, 5, 4], 400 + K)
    hy = Hyper.defaults(K, V)
    z = [init_assignments(K, [c.doc_off[m]], seed=5 + m)[0] for m in range(c.M)]
    with native_from(c, hy, z) as s:
        s.sweep(0, 3)
        check(s, 20, c.doc_off[0], c.tokens[0])


def test_after_live_sweeps_on_the_16_bit_mirror(monkeypatch):
    monkeypatch.setenv("MVHDP_LIVE16", "1")
    K, V = 300, [3000, 300, 300]
    c = small_corpus(K, V, 300, [127, 7, 15], 32)
    hy = Hyper.defaults(K, V)
    z = [init_assignments(K, [c.doc_off[m]], seed=7 + m)[0] for m in range(c.M)]
    with native_from(c, hy, z) as s:
        for it in range(3):
            s.sweep(it, 77, flags=SWEEP_LIVE)
        check(s, 20, c.doc_off[0], c.tokens[0])


def test_two_calls_give_identical_bits():
    K, V = 200, [2000, 100]
    c = small_corpus(K, V, 400, [90, 6], 55)
    z = [init_assignments(K, [c.doc_off[m]], seed=9 + m)[0] for m in range(c.M)]
    with native_from(c, Hyper.defaults(K, V), z) as s:
        a, b = s.diagnostics(), s.diagnostics()
        for name in DIAG_ROWS:
            assert a.scores[name].tobytes() == b.scores[name].tobytes() and a.word_scores[name].tobytes() == b.word_scores[name].tobytes()
        assert a.sum_count_log_count.tobytes() == b.sum_count_log_count.tobytes()
        assert a.discr_weight_per_view.tobytes() == b.discr_weight_per_view.tobytes()


def _raw_call(s, N, wl=None):
    """mvhdp_diagnostics through ctypes with sentinel-filled outputs: (rc, the arrays)."""
    K, V0, M = s.K, s.V[0], s.M
    a = dict(scores=np.full((13, K), 7.0), word_scores=np.full((13, K, 64), 7.0), codoc=np.full((K, 64, 64), 7, np.int32),
             top_types=np.full((K, 64), 7, np.int32), top_counts=np.full((K, 64), 7, np.int32), nonzero=np.full(K, 7, np.int32),
             num_rank1_docs=np.full(K, 7, np.int32), num_nonzero_docs=np.full(K, 7, np.int32),
             num_docs_at_proportions=np.full((K, 7), 7, np.int32), sum_count_log_count=np.full(K, 7.0),
             word_type_counts=np.full(V0, 7, np.int32), num_tokens=np.full(1, 7, np.int64), discr_weight_per_view=np.full(M, 7.0))
    args = DiagArgsC(N, None if wl is None else wl.ctypes.data)
    out = DiagOutC(**{f: a[f].ctypes.data for f, _ in DiagOutC._fields_})
    return s.L.mvhdp_diagnostics(s.h, C.byref(args), C.byref(out)), a


def test_errors_leave_the_outputs_untouched():
    K, V = 20, [300, 40]
    c = small_corpus(K, V, 60, [30, 4], 77)
    z = [init_assignments(K, [c.doc_off[m]], seed=1 + m)[0] for m in range(c.M)]
    with native_from(c, Hyper.defaults(K, V), z) as s:
        for n in (0, 65):
            rc, a = _raw_call(s, n)
            assert rc == -1 and untouched(a, 7)
            t = np.full((K, 70), 7, np.int32); cc = t.copy(); nz = np.full(K, 7, np.int32)
            assert s.L.mvhdp_top_words(s.h, 0, n, t.ctypes.data, cc.ctypes.data, nz.ctypes.data) == -1
            assert np.all(t == 7) and np.all(cc == 7) and np.all(nz == 7)
        for m in (-1, 2):
            t = np.full((K, 20), 7, np.int32); cc = t.copy(); nz = np.full(K, 7, np.int32)
            assert s.L.mvhdp_top_words(s.h, m, 20, t.ctypes.data, cc.ctypes.data, nz.ctypes.data) == -1
            pv = np.full(2, 7.0)
            assert s.L.mvhdp_discr_weights(s.h, pv.ctypes.data, m, None) == -1 and np.all(pv == 7)
        assert s.L.mvhdp_top_words(s.h, 0, 20, None, None, None) == -1
        assert s.L.mvhdp_discr_weights(s.h, None, 0, None) == -1
        assert s.L.mvhdp_diagnostics(s.h, None, None) == -1
        with pytest.raises(MvhdpError):
            s.top_words(0, 65)
        # an unassigned view-0 token: the counts are set to the counts of the rest, as a host that skipped it would hold them
        zz = z[0].copy()
        zz[5] = -1
        s.set_assignments(0, zz)
        s.build_counts()
        rc, a = _raw_call(s, 20)
        assert rc == -2 and untouched(a, 7), rc
        s.set_assignments(0, z[0])
        s.build_counts()
        rc, a = _raw_call(s, 20)
        assert rc == 0
    # an out-of-vocabulary view-0 token
    t0 = c.tokens[0].copy()
    t0[3] = V[0] + 5
    with NativeSampler(K, V) as s:
        s.set_corpus(0, c.doc_off[0], t0)
        s.set_corpus(1, c.doc_off[1], c.tokens[1])
        for m in range(2):
            s.set_assignments(m, z[m])
        s.set_hyper(Hyper.defaults(K, V))
        s.build_counts()
        rc, a = _raw_call(s, 20)
        assert rc == -2 and untouched(a, 7), rc


def test_c4_full_size_integers():
    """The whole C4 corpus (1 M entities, view 0: about 127 M tokens) under random assignments: the integers equal the checker's."""
    c = synth.make_config("C4")
    K, V = c.K, c.V
    rng = np.random.default_rng(4)
    z = [rng.integers(0, K, size=len(c.tokens[m]), dtype=np.int32) for m in range(c.M)]
    with native_from(c, Hyper.defaults(K, V), z) as s:
        d = s.diagnostics(num_top_words=20)
        nwk0, nk0 = s.get_counts(0)
        t, cn, nz = dn.top_words(nwk0, 20)
        assert np.array_equal(d.top_words, t) and np.array_equal(d.top_counts, cn) and np.array_equal(d.nonzero, nz)
        ds = dn.document_statistics(c.doc_off[0], c.tokens[0], z[0], K, V[0], t, nz, 20, 1.0, np.full(K, 0.1), K * 0.1)
        for f in ("codoc", "num_rank1_docs", "num_nonzero_docs", "num_docs_at_proportions", "word_type_counts"):
            assert np.array_equal(getattr(d, f), ds[f]), f
        assert d.num_tokens == ds["num_tokens"]
