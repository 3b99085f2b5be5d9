"""CPU known answers of the embedding restatement (tests/native/emb_ref.c): against a literal Python transcription of the Java loops
(TopicWordEmbeddingRunnable.run / gradientLearn, sequential dot products, the same Philox draws), the sampling-table builder against
the literal while loop of TWE:393-399, the two quirks kept (cumulative counts, sigmoidCache[size] = 0), and its Philox against the
oracle's known-answer implementation."""
import math

import numpy as np
import pytest

from mvtopicmodel_amd.native import EmbConfig
from tests import emb_ref as er

M32 = 0xFFFFFFFF


def py_philox(c, k):
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def py_draw64(n, purpose, ent, epoch, k0, k1):
    x = py_philox([n >> 1, purpose, ent, epoch], [k0, k1])
    return (x[2] << 32 | x[3]) if n & 1 else (x[0] << 32 | x[1])


def java_train(ref, doc_off, tok, z, epochs, seed, rnd):
    """TWER:82-293 transcribed line by line (the dot products in column order), with the device's draws and its per-document rate."""
    cfg = ref.cfg
    V0, C, Cc, ns = ref.V0, ref.C, ref.Cc, cfg.num_samples
    w = [list(r) for r in ref.w]
    neg = [list(r) for r in ref.neg]
    cache, table, size = list(ref.cache), ref.table, cfg.sampling_table_size
    k0, k1 = (seed & M32) ^ rnd, seed >> 32
    scale = cfg.sigmoid_cache_size / (cfg.max_exp - cfg.min_exp)
    N0, topics = int(doc_off[-1]), z is not None
    st = dict(words=0, sampled=0, considered=0, skipped=0, calls=0, negskip=0, residual=0.0)
    state = {}

    def learn(inp, out, lr, ctx, ent, ep):
        lo, hi = (0, Cc) if ctx else (Cc, C)
        grad = [0.0] * C
        ip = 0.0
        for col in range(lo, hi):
            ip += neg[inp][col] * w[out][col]
        if ip < cfg.min_exp:
            g = lr
        elif ip > cfg.max_exp:
            g = 0.0
        else:
            g = lr * (1.0 - cache[math.floor((ip - cfg.min_exp) * scale)])
        for col in range(lo, hi):
            grad[col] = g * neg[inp][col]
            neg[inp][col] += g * w[out][col]
        state["res"] += g
        inv = 1.0 / ns if ns else 0.0
        for q in range(ns):
            t = int(table[(py_draw64(state["call"] * ns + q, 0x502, ent, ep, k0, k1) * size) >> 64])
            if t == inp:
                st["negskip"] += 1
                continue
            ip = 0.0
            for col in range(lo, hi):
                ip += neg[t][col] * w[out][col]
            if ip < cfg.min_exp:
                g = 0.0
            elif ip > cfg.max_exp:
                g = -lr
            else:
                g = lr * -cache[math.floor((ip - cfg.min_exp) * scale)]
            for col in range(lo, hi):
                grad[col] += g * neg[t][col]
                neg[t][col] += g * w[out][col]
            state["res"] -= g * inv
        state["call"] += 1
        st["calls"] += 1
        for col in range(lo, hi):
            w[out][col] += grad[col]

    for ep in range(epochs):
        state["res"] = 0.0
        for d in range(len(doc_off) - 1):
            b, e = int(doc_off[d]), int(doc_off[d + 1])
            ent = d
            state["call"] = 0
            lr = max(0.025 * 0.0001, 0.025 * (1.0 - float(ep * N0 + b) / float(epochs * ref.total)))
            buf, top = [], []
            for pos in range(e - b):
                st["words"] += 1
                u = (py_draw64(pos, 0x500, ent, ep, k0, k1) >> 11) * 2.0 ** -53
                if u < ref.retention[tok[b + pos]]:
                    buf.append(int(tok[b + pos])); top.append(int(z[b + pos]) if topics else 0)
                    st["sampled"] += 1
            if len(buf) < cfg.min_doc_length:
                st["skipped"] += 1
                continue
            for p in range(len(buf)):
                st["considered"] += 1
                a, ta = buf[p], V0 + top[p]
                if topics:
                    learn(a, ta, lr, True, ent, ep); learn(a, ta, lr, False, ent, ep); learn(ta, a, lr, False, ent, ep)
                sw = ((py_draw64(p, 0x501, ent, ep, k0, k1) * cfg.window) >> 64) + 1
                for q in range(max(0, p - sw), min(len(buf) - 1, p + sw) + 1):
                    if q == p:
                        continue
                    learn(a, buf[q], lr, False, ent, ep)
                    if topics:
                        learn(ta, V0 + top[q], lr, True, ent, ep)
        st["residual"] += state["res"]
    return np.array(w), np.array(neg), st


def tiny_corpus(V0, K, lens, seed):
    rng = np.random.default_rng(seed)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = rng.integers(0, V0, int(doc_off[-1])).astype(np.int32)
    z = rng.integers(0, K, int(doc_off[-1])).astype(np.int32)
    return doc_off, tok, z


def test_philox_matches_the_oracle(oracle_lib):
    import ctypes as C
    rng = np.random.default_rng(5)
    for _ in range(200):
        ctr = [int(x) for x in rng.integers(0, 2 ** 32, 4)]
        key = [int(x) for x in rng.integers(0, 2 ** 32, 2)]
        c = (C.c_uint32 * 4)(*ctr); k = (C.c_uint32 * 2)(*key); o = (C.c_uint32 * 4)()
        oracle_lib.orc_philox4x32_10(c, k, o)
        assert er.philox(ctr, key) == list(o) == py_philox(ctr, key)
    assert er.philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


@pytest.mark.parametrize("V0", [1, 7, 300])
def test_the_table_builder_equals_the_literal_loop(V0):
    """TWE:393-399 as written against one lower_bound per index (the device's form), every index at size 10^6; ties, zero counts."""
    rng = np.random.default_rng(V0)
    cfg = EmbConfig.defaults(sampling_table_size=10 ** 6)
    ref = er.EmbRef(V0, 1, cfg)
    tok = rng.choice(V0, size=5000, p=np.arange(V0, 0, -1) / (V0 * (V0 + 1) / 2)).astype(np.int32)
    if V0 > 10:
        tok = tok[tok != 3]                                             # a word that never occurs (count 0, last in the order)
    ref.count_words(tok)
    assert np.array_equal(ref.table, ref.table_literal())
    assert ref.table[0] == ref.sorted[0]
    # Python's literal loop at a smaller size
    cfg2 = EmbConfig.defaults(sampling_table_size=10 ** 4)
    r2 = er.EmbRef(V0, 1, cfg2)
    r2.count_words(tok)
    S, order, lit = r2.dist[-1], 0, []
    for i in range(cfg2.sampling_table_size):
        lit.append(r2.sorted[order])
        while S * i / cfg2.sampling_table_size > r2.dist[order]:
            order += 1
    assert np.array_equal(r2.table, np.array(lit, dtype=np.int32))


def test_counts_and_total_are_cumulative():
    """countWords never resets wordCounts / totalWords (TWE:362,369): a second call doubles both, and retention follows them."""
    V0 = 20
    rng = np.random.default_rng(1)
    tok = rng.integers(0, V0, 500).astype(np.int32)
    ref = er.EmbRef(V0, 1, EmbConfig.defaults(sampling_table_size=1000, sampling_factor=0.01))
    ref.count_words(tok)
    c1, t1 = ref.counts.copy(), ref.total
    ref.count_words(tok)
    assert np.array_equal(ref.counts, 2 * c1) and ref.total == 2 * t1 == 1000
    s = ref.counts / (0.01 * ref.total)
    assert np.array_equal(ref.retention, np.minimum((np.sqrt(s) + 1) / s, 1.0))


def test_sigmoid_cache_keeps_its_unset_last_entry():
    """sigmoidCache[1000] stays 0.0 (TWE:157-162), and an inner product of exactly +6 reads it: floor(12 * (1000 / 12)) = 1000."""
    c = er.cache()
    assert len(c) == 1001 and c[1000] == 0.0 and c[999] > 0.99
    assert c[500] == 0.5 and c[0] == 1.0 / (1.0 + math.exp(6.0))
    assert math.floor((6.0 - -6.0) * (1000 / 12.0)) == 1000
    lr = 0.025
    assert er.lib().er_residual(6.0, lr, 1, er.ptr(c), 1000, -6.0, 6.0) == lr                        # lr * (1 - 0.0)
    assert er.lib().er_residual(6.0, lr, 0, er.ptr(c), 1000, -6.0, 6.0) == 0.0                       # lr * -0.0
    assert er.lib().er_residual(5.99, lr, 1, er.ptr(c), 1000, -6.0, 6.0) < 0.0001


@pytest.mark.parametrize("topics", [True, False])
def test_restatement_equals_the_java_transcription(topics):
    V0, K = 6, 2
    cfg = EmbConfig.defaults(with_topics=topics, num_columns=8, num_context_columns=3 if topics else 0, window=2, num_samples=3,
                             min_doc_length=4, sampling_table_size=5000, sampling_factor=0.2)
    doc_off, tok, z = tiny_corpus(V0, K, [12, 3, 9, 15], seed=3)
    ref = er.EmbRef(V0, K, cfg, seed=11)
    ref.count_words(tok)
    w0, n0 = ref.w.copy(), ref.neg.copy()
    st = ref.train(doc_off, tok, z if topics else None, 2, seed=77, round_idx=1)
    ref2 = er.EmbRef(V0, K, cfg, seed=11)
    ref2.count_words(tok)
    assert np.array_equal(ref2.w, w0) and np.array_equal(ref2.neg, n0)
    jw, jn, jst = java_train(ref2, doc_off, tok, z if topics else None, 2, 77, 1)
    for f in ("words", "sampled", "considered", "skipped", "calls", "negskip"):
        assert st[f] == jst[f], f
    assert st["calls"] > 50 and st["skipped"] >= 1
    np.testing.assert_allclose(ref.w, jw, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref.neg, jn, rtol=1e-12, atol=1e-15)
    assert abs(st["residual"] - jst["residual"]) <= 1e-12 * abs(jst["residual"])
    assert not np.array_equal(ref.w, w0)


def test_init_weights_follow_the_stream():
    ref = er.EmbRef(5, 2, EmbConfig.defaults(num_columns=7, num_context_columns=2), seed=(3 << 32) | 9)
    for r in range(7):
        for c in range(7):
            u = (py_draw64(c, 0x503, r, 0, 9, 3) >> 11) * 2.0 ** -53
            assert ref.w[r, c] == (u - 0.5) / 7
    assert not ref.neg.any()
