"""Word and topic embeddings on the device (mvhdp_emb_*, csrc/mvhdp_emb.hip) against the sequential restatement tests/native/emb_ref.c:
the sampling table index for index, the serial trainer bit for bit, the Hogwild trainer by its draw-determined counters and by the
quality it reaches on a planted corpus, the softmax table, findClosest, the error paths."""
import time

import numpy as np
import pytest

from mvtopicmodel_amd import NativeSampler
from mvtopicmodel_amd._lib import MvhdpError
from mvtopicmodel_amd.native import EmbConfig
from tests import emb_ref as er

pytestmark = pytest.mark.gpu
STATS = ("words_so_far", "words_sampled", "words_considered", "docs_skipped", "calls", "negatives_skipped")
REF = dict(words_so_far="words", words_sampled="sampled", words_considered="considered", docs_skipped="skipped", calls="calls",
           negatives_skipped="negskip")


def corpus(V0, K, lens, seed):
    rng = np.random.default_rng(seed)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(doc_off[-1])
    return doc_off, rng.integers(0, V0, n).astype(np.int32), rng.integers(0, K, n).astype(np.int32)


def sampler(K, V0, doc_off, tok, z):
    s = NativeSampler(K, [V0])
    s.set_corpus(0, doc_off, tok)
    s.set_assignments(0, z)
    return s


def test_sampling_table_equals_the_restatement():
    V0, K = 400, 3
    rng = np.random.default_rng(2)
    lens = rng.integers(1, 60, 300)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = np.minimum(rng.zipf(1.3, int(doc_off[-1])) - 1, V0 - 1).astype(np.int32)
    z = np.zeros(len(tok), np.int32)
    for size in (10 ** 6, 10 ** 8):
        cfg = EmbConfig.defaults(num_columns=16, num_context_columns=4, sampling_table_size=size)
        with sampler(K, V0, doc_off, tok, z) as s:
            s.emb_init(cfg, seed=1)
            s.emb_count_words()
            ref = er.EmbRef(V0, K, cfg)
            ref.count_words(tok, table=False)
            c, r, t = s.emb_word_stats()
            assert np.array_equal(c, ref.counts) and t == ref.total and np.array_equal(r, ref.retention)
            if size == 10 ** 6:
                assert np.array_equal(s.emb_sampling_table(0, size), ref.table_range(0, size))
            else:
                idx = rng.choice(size, 10 ** 5, replace=False)          # 10^5 scattered indices over the whole table
                idx[:3] = [0, 1, size - 1]
                table = s.emb_sampling_table(0, size)                   # (one copy of the 400 MB table)
                assert np.array_equal(table[idx], ref.table_at(idx))


def _serial_case(C, Cc, topics, V0, K=3):
    lens = [0, 4, 8, 30, 12, 45, 2, 60, 25, 900, 33]              # empty, shorter than min_doc_length / the window, one beyond the LDS buffer
    doc_off, tok, z = corpus(V0, K, lens, seed=C + Cc + V0)
    cfg = EmbConfig.defaults(with_topics=topics, num_columns=C, num_context_columns=Cc if topics else 0, sampling_table_size=10 ** 5,
                             sampling_factor=0.3)
    return doc_off, tok, z, cfg


GRID = [(C, Cc, t, V0) for C in (16, 64, 200, 256) for Cc in (0, 8, 50) for t in (True, False) for V0 in (4, 300)
        if Cc < C and (t or Cc == 0)]


@pytest.mark.parametrize("C,Cc,topics,V0", GRID)
def test_serial_trainer_is_bit_exact(C, Cc, topics, V0):
    K = 3
    doc_off, tok, z, cfg = _serial_case(C, Cc, topics, V0, K)
    ref = er.EmbRef(V0, K, cfg, seed=5)
    with sampler(K, V0, doc_off, tok, z) as s:
        s.emb_init(cfg, seed=5)
        w, n = s.emb_get_vectors()
        assert np.array_equal(w, ref.w) and np.array_equal(n, ref.neg)
        for rnd, epochs in ((0, 1), (1, 2)):                          # two count / train rounds: the cumulative counts
            s.emb_count_words(); ref.count_words(tok)
            st = s.emb_train(epochs, seed=123, round_idx=rnd, serial=True)
            rs = ref.train(doc_off, tok, z if topics else None, epochs, seed=123, round_idx=rnd)
            for f in STATS:
                assert getattr(st, f) == rs[REF[f]], f
            assert st.words_so_far == epochs * len(tok)
            assert st.residual == rs["residual"] and st.last_epoch_residual == rs["last_residual"] and st.last_epoch_calls == rs["last_calls"]
            w, n = s.emb_get_vectors()
            assert np.array_equal(w, ref.w), f"weights differ at round {rnd}: {np.argwhere(w != ref.w)[:5]}"
            assert np.array_equal(n, ref.neg), f"negative weights differ at round {rnd}"
        assert st.negatives_skipped > 0 if V0 == 4 else True


def test_hogwild_draws_equal_the_serial_ones():
    K, V0 = 3, 300
    doc_off, tok, z, cfg = _serial_case(64, 8, True, V0, K)
    out = []
    for serial in (True, False):
        with sampler(K, V0, doc_off, tok, z) as s:
            s.emb_init(cfg, seed=5)
            s.emb_count_words()
            out.append((s.emb_train(2, seed=9, serial=serial), s.emb_get_vectors()))
    for f in STATS:
        assert getattr(out[0][0], f) == getattr(out[1][0], f), f
    assert all(np.isfinite(x).all() for x in out[1][1])


def planted(n_clusters=20, per=25, D=8000, L=20, noise=0.35, seed=4):
    """Overlapping clusters: a document draws from one or two clusters, and each of its tokens is, with probability `noise`, a word of
    the NEXT cluster (so neighbouring clusters share contexts) under the document cluster's topic.  D = 8000 entities: more than the
    device keeps resident, so the topic rows and the frequent words are updated by many waves at once."""
    rng = np.random.default_rng(seed)
    V0 = n_clusters * per
    toks, zs = [], []
    for d in range(D):
        cl = rng.choice(n_clusters, size=1 + (d % 2), replace=False)
        c = rng.choice(cl, L)
        wc = np.where(rng.random(L) < noise, (c + 1) % n_clusters, c)
        toks.append(wc * per + rng.integers(0, per, L)); zs.append(c)
    doc_off = np.arange(0, D * L + 1, L, dtype=np.int64)
    return V0, n_clusters, doc_off, np.concatenate(toks).astype(np.int32), np.concatenate(zs).astype(np.int32), per


def quality(w, V0, K, per):
    x = w / np.linalg.norm(w, axis=1, keepdims=True)
    cl = np.arange(V0) // per
    sim = x[:V0] @ x[:V0].T
    np.fill_diagonal(sim, -2)
    nn = np.argsort(-sim, axis=1)[:, :10]
    words = float((cl[nn] == cl[:, None]).mean())
    ts = x[V0:] @ x[:V0].T
    tn = np.argsort(-ts, axis=1)[:, :10]
    topics = float((cl[tn] == np.arange(K)[:, None]).mean())
    return words, topics


def test_hogwild_quality_matches_the_serial_trainer(capsys):
    """Thresholds set from the first MI355X run on this corpus, with margin: serial / Hogwild word purity 1.000 / 1.000, topic purity
    0.990 / 0.990-0.995, last-epoch mean residual 0.00572 / 0.00584 (2 % apart; profiles/embeddings.md)."""
    V0, K, doc_off, tok, z, per = planted()
    cfg = EmbConfig.defaults(num_columns=32, num_context_columns=8, sampling_table_size=10 ** 6, sampling_factor=0.05)
    res = {}
    for serial in (True, False):
        with sampler(K, V0, doc_off, tok, z) as s:
            s.emb_init(cfg, seed=3)
            s.emb_count_words()
            st = s.emb_train(1, seed=8, serial=serial)
            w, _ = s.emb_get_vectors()
            res[serial] = quality(w, V0, K, per) + (st.last_epoch_residual / st.last_epoch_calls, st.kernel_ms)
    with capsys.disabled():
        print(f"\n[emb quality] serial words {res[True][0]:.3f} topics {res[True][1]:.3f} residual {res[True][2]:.5f} {res[True][3]:.1f} ms | "
              f"hogwild words {res[False][0]:.3f} topics {res[False][1]:.3f} residual {res[False][2]:.5f} {res[False][3]:.1f} ms")
    assert res[True][0] > 0.9 and res[True][1] > 0.9
    assert res[False][0] >= res[True][0] - 0.05
    assert res[False][1] >= res[True][1] - 0.05
    assert abs(res[False][2] - res[True][2]) <= 0.06 * abs(res[True][2])


def test_hot_rows_stay_finite_and_the_residual_falls():
    V0, K = 20, 2
    doc_off, tok, z = corpus(V0, K, [30] * 4000, seed=6)
    cfg = EmbConfig.defaults(num_columns=64, num_context_columns=16, sampling_table_size=10 ** 6, sampling_factor=0.5)
    with sampler(K, V0, doc_off, tok, z) as s:
        s.emb_init(cfg, seed=1)
        s.emb_count_words()
        r = []
        for rnd in range(3):
            st = s.emb_train(1, seed=2, round_idx=rnd)
            r.append(st.last_epoch_residual / st.last_epoch_calls)
        w, n = s.emb_get_vectors()
        assert np.isfinite(w).all() and np.isfinite(n).all()
        assert r[2] < r[0], r


def test_softmax_equals_the_restatement():
    K, V0 = 7, 300
    doc_off, tok, z, cfg = _serial_case(200, 50, True, V0, K)
    ref = er.EmbRef(V0, K, cfg, seed=5)
    with sampler(K, V0, doc_off, tok, z) as s:
        s.emb_init(cfg, seed=5)
        s.emb_count_words(); ref.count_words(tok)
        s.emb_train(1, seed=1, serial=True); ref.train(doc_off, tok, z, 1, seed=1)
        for reset in (True, False, False):                         # PTM:360: the sums accumulate across calls
            e, sm = s.emb_softmax(reset_sums=reset)
            re_, rs = ref.softmax(reset_sums=reset)
            np.testing.assert_allclose(e, re_, rtol=1e-14, atol=0)
            np.testing.assert_allclose(sm, rs, rtol=1e-12, atol=0)
        assert np.allclose(sm, 3 * ref.softmax(reset_sums=True)[1], rtol=1e-12)


def test_nearest_in_idsorter_order():
    K, V0 = 5, 300
    doc_off, tok, z, cfg = _serial_case(64, 8, True, V0, K)
    with sampler(K, V0, doc_off, tok, z) as s:
        s.emb_init(cfg, seed=5)
        s.emb_count_words()
        s.emb_train(1, seed=1)
        w, _ = s.emb_get_vectors()
        q = w[17].copy()                                            # findClosest(copy(queryWord))
        words, wsim, topics, tsim = s.emb_nearest(q, 10)
        cos = (w @ q) * (1.0 / np.sqrt(q @ q)) * (1.0 / np.sqrt((w * w).sum(1)))
        order = sorted(range(V0), key=lambda i: (-cos[i], -i))[:10]
        assert words[0] == 17 and list(words) == order
        np.testing.assert_allclose(wsim, cos[order], rtol=1e-12)
        torder = sorted(range(K), key=lambda i: (-cos[V0 + i], -i))
        assert list(topics[:K]) == torder and (topics[K:] == -1).all() and np.isnan(tsim[K:]).all()


def test_error_paths_and_round_trips():
    K, V0 = 3, 50
    doc_off, tok, z = corpus(V0, K, [20] * 10, seed=1)
    with sampler(K, V0, doc_off, tok, z) as s:
        with pytest.raises(MvhdpError) as e:
            s.emb_count_words()
        assert e.value.code == -2                                   # before emb_init
        for bad in (dict(num_columns=0), dict(num_columns=257), dict(num_columns=16, num_context_columns=16), dict(window=0),
                    dict(num_samples=33), dict(min_doc_length=0), dict(sampling_table_size=0), dict(sampling_factor=0.0)):
            kw = dict(num_columns=16, num_context_columns=4, sampling_table_size=1000)
            kw.update(bad)
            with pytest.raises(MvhdpError) as e:
                s.emb_init(EmbConfig.defaults(**kw))
            assert e.value.code == -1, bad
        cfg = EmbConfig.defaults(num_columns=16, num_context_columns=4, sampling_table_size=1000, sampling_factor=0.5, min_doc_length=2)
        s.emb_init(cfg, seed=2)
        with pytest.raises(MvhdpError) as e:
            s.emb_train(1, seed=1)
        assert e.value.code == -2                                   # before count_words
        s.emb_count_words()
        w0, n0 = s.emb_get_vectors()
        zb = z.copy(); zb[7] = -1                                   # an unassigned topic: refused, nothing touched
        s.set_assignments(0, zb)
        with pytest.raises(MvhdpError) as e:
            s.emb_train(1, seed=1)
        assert e.value.code == -1
        w1, n1 = s.emb_get_vectors()
        assert np.array_equal(w0, w1) and np.array_equal(n0, n1)
        s.set_assignments(0, z)
        s.emb_train(1, seed=1)
        w, n = s.emb_get_vectors()
        s.emb_set_vectors(w0 * 2, None)
        w2, n2 = s.emb_get_vectors()
        assert np.array_equal(w2, w0 * 2) and np.array_equal(n2, n)
        rng = np.random.default_rng(0)
        s.emb_init(cfg, weights=w0 + 1.0)
        assert np.array_equal(s.emb_get_vectors()[0], w0 + 1.0) and not s.emb_get_vectors()[1].any()
        with pytest.raises(MvhdpError):
            s.emb_sampling_table(0, 1)                              # a fresh init has no table
        s.emb_count_words()
        with pytest.raises(MvhdpError):
            s.emb_sampling_table(999, 2)
        with pytest.raises(MvhdpError):
            s.emb_nearest(rng.standard_normal(16), 65)
        s.emb_release()
        with pytest.raises(MvhdpError):
            s.emb_get_vectors()
        s.emb_init(EmbConfig.defaults(with_topics=False, num_columns=16, sampling_table_size=1000, sampling_factor=0.5))
        with pytest.raises(MvhdpError) as e:
            s.emb_softmax()
        assert e.value.code == -2                                   # no topic rows
        assert s.emb_get_vectors()[0].shape == (V0, 16)
    # a bad token is refused by the count
    with NativeSampler(K, [V0]) as s:
        t2 = tok.copy(); t2[3] = V0 + 1
        s.set_corpus(0, doc_off, t2)
        s.emb_init(cfg)
        with pytest.raises(MvhdpError) as e:
            s.emb_count_words()
        assert e.value.code == -1


def test_one_hogwild_epoch_over_c4_view0(capsys):
    from mvtopicmodel_amd import synth
    from mvtopicmodel_amd.java_init import init_assignments
    cfgc = synth.CONFIGS["C4"]
    K, V0 = cfgc["K"], cfgc["V"][0]
    c = synth.make_config("C4")
    z0 = init_assignments(K, [c.doc_off[0]], seed=1)[0]
    with sampler(K, V0, c.doc_off[0], c.tokens[0], z0) as s:
        s.emb_init(EmbConfig.defaults(), seed=1)
        t0 = time.perf_counter()
        s.emb_count_words()
        t1 = time.perf_counter()
        st = s.emb_train(1, seed=1)
        t2 = time.perf_counter()
        w, n = s.emb_get_vectors()
        with capsys.disabled():
            print(f"\n[emb C4] count+table {1e3 * (t1 - t0):.0f} ms, epoch {1e3 * (t2 - t1):.0f} ms wall / {st.kernel_ms:.0f} ms kernels, "
                  f"{st.words_so_far / (st.kernel_ms * 1e-3) / 1e6:.1f} M input tokens/s, {st.calls / (st.kernel_ms * 1e-3) / 1e6:.1f} M calls/s, "
                  f"calls {st.calls}, kept {st.words_sampled}, mean residual {st.last_epoch_residual / st.last_epoch_calls:.5f}")
        assert st.words_so_far == len(c.tokens[0])
        assert np.isfinite(w).all() and np.isfinite(n).all()
        assert t2 - t1 < 300
