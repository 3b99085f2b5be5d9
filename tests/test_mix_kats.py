"""The restatement of the deferred sweep with the useVectorsLambda mix (tests/native/mix_ref.c) pinned from three sides, on the CPU:
(a) with the mix off -- and with lambda = 0 run through the mix expression -- it IS the oracle, bit for bit;
(b) a literal Python transcription of WRK:496-536 and PTM:2668-2680 on a tiny model gives its decisions and masses bit for bit;
(c) answers derived by hand: lambda = 1 forgets n_wk in view 0 and leaves the other views alone; a flat table gives a root in closed form."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd.native import Hyper
from mvtopicmodel_amd.synth import Corpus
from oracle.binding import Oracle
from tests.helpers import small_corpus
from tests.mix_cases import inactive_case, make_ref, ragged_corpus, same_state, same_stats, table
from tests.mix_ref import make_mix


def _cases():
    out = {}
    K, V = 5, [60]
    out["m1_k5"] = (small_corpus(K, V, 20, [12], 3), Hyper.defaults(K, V), None)
    K, V = 100, [400, 50, 40]
    out["m3_k100"] = (small_corpus(K, V, 30, [50, 6, 5], 4), Hyper.defaults(K, V), None)
    out["m3_k40_inactive"] = inactive_case(40, (300, 50, 40), 40, (30, 5, 4), 51)
    c, z0 = ragged_corpus(K=40)
    out["m2_k40_ragged"] = (c, Hyper.defaults(c.K, c.V), z0)
    # an EMPTY view: the middle one of three holds no token in any entity (docLength 0 everywhere, the i != m filter with a whole view gone)
    K, V = 40, [200, 30, 25]
    full = small_corpus(K, V, 25, [30, 4, 5], 6)
    c = Corpus(K, V, [full.doc_off[0], np.zeros(full.D + 1, dtype=np.int64), full.doc_off[2]],
               [full.tokens[0], np.zeros(0, dtype=np.int32), full.tokens[2]])
    out["m3_k40_empty_view"] = (c, Hyper.defaults(K, V), None)
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("through", [False, True], ids=["off", "lambda0_through_mix"])
def test_lambda_zero_is_the_oracle(name, through):
    c, hy, z0 = CASES[name]
    o = make_ref(c, hy, z0, cls=Oracle)
    r = make_ref(c, hy, z0)
    if through:
        e, S = table(c.K, c.V[0], 7)
        r.set_vectors_mix(0.0, e, S, through_mix_path=True)
        assert r.mix is not None and not r.mix.any() and r.oml == 1.0
    trace = [(d, m, 0) for d in range(c.D) for m in range(c.M) if c.doc_off[m][d + 1] > c.doc_off[m][d]][:40]
    for it in range(4):
        ro = o.sweep(it, 99, want_dbg=True, trace=trace)
        rr = r.sweep(it, 99, want_dbg=True, trace=trace)
        same_stats(ro["stats"], rr["stats"], f"{name} sweep {it}")
        assert ro["stats"]["activation_key"] == rr["stats"]["activation_key"]
        same_state(o, r, c.M, f"{name} sweep {it}")
        for m in range(c.M):
            assert np.array_equal(ro["dbg"][m], rr["dbg"][m]), f"{name} sweep {it}: tok_dbg of view {m}"
            for w in range(c.V[m]):                                     # (the trees this sweep sampled from)
                assert np.array_equal(o.get_tree(m, w), r.get_tree(m, w)), (name, it, m, w)
        assert np.array_equal(ro["trace"], rr["trace"], equal_nan=True)
        assert np.array_equal(o.get_alpha(), r.get_alpha()) and np.array_equal(o.get_inactive(), r.get_inactive())
    # NO_APPLY and a list sweep, too
    ro = o.sweep(9, 5, flags=2, want_delta=True); rr = r.sweep(9, 5, flags=2, want_delta=True)
    assert np.array_equal(ro["delta_nwk"], rr["delta_nwk"]) and np.array_equal(ro["delta_nk"], rr["delta_nk"])
    same_state(o, r, c.M, f"{name} NO_APPLY")
    o.apply_delta(ro["delta_nwk"], ro["delta_nk"]); r.apply_delta(rr["delta_nwk"], rr["delta_nk"])
    docs = np.arange(c.D - 1, -1, -2)
    ro = o.sweep_list(10, 5, docs); rr = r.sweep_list(10, 5, docs)
    same_stats(ro["stats"], rr["stats"], f"{name} list")
    same_state(o, r, c.M, f"{name} list")
    o.close(); r.close()


# ---------------------------------------------------------------------------------------------------------------------
# (b) the reference's own lines, transcribed into Python floats (IEEE doubles, nothing fused)
def _transcription(r, c, hy, lam, e, S, p, sweep_idx, seed):
    """One deferred sweep over model state read from the restatement `r` BEFORE its sweep: returns (z after, tok_dbg rows per view,
    tree[1] per view-0 type).  WRK:327-471 keep the entity's books; WRK:496-536 and PTM:2668-2680 are copied expression for expression."""
    L = r.L
    K, M, D = c.K, c.M, c.D
    useVectorsLambda = float(lam)
    expDotProductValues, sumExpValues = e, S
    beta, betaSum, gamma, alpha, alphaSum = hy.beta, hy.beta_sum, hy.gamma, hy.alpha, hy.alpha_sum
    cnts = [r.get_counts(m) for m in range(M)]
    typeTopicCounts = [cn[0] for cn in cnts]
    tokensPerTopic = [cn[1] for cn in cnts]
    inactive = np.zeros(K, dtype=np.uint8) if hy.inactive is None else hy.inactive
    first_inactive = int(np.flatnonzero(inactive)[0]) if inactive.any() else -1
    z = [r.get_assignments(m).copy() for m in range(M)]
    # PTM:2660-2696
    trees = []
    for m in range(M):
        tm = np.zeros((c.V[m], 2 * K))
        for w in range(c.V[m]):
            temp = np.zeros(K)
            currentTypeTopicCounts = typeTopicCounts[m][w]
            for currentTopic in range(K):
                if inactive.any() and inactive[currentTopic]:
                    temp[currentTopic] = 0
                else:
                    if useVectorsLambda != 0 and m == 0:
                        p_wt = (useVectorsLambda * (float(expDotProductValues[currentTopic][w]) / float(sumExpValues[currentTopic])) + (1 - useVectorsLambda)
                                * ((int(currentTypeTopicCounts[currentTopic]) + float(beta[m])) / (int(tokensPerTopic[m][currentTopic]) + float(betaSum[m]))))
                    else:
                        p_wt = (int(currentTypeTopicCounts[currentTopic]) + float(beta[m])) / (int(tokensPerTopic[m][currentTopic]) + float(betaSum[m]))
                    temp[currentTopic] = float(gamma[m]) * float(alpha[m][currentTopic]) * p_wt
            L.orc_ftree_construct(tm[w].ctypes.data_as(C.c_void_p), K, temp.ctypes.data_as(C.c_void_p))
        trees.append(tm)
    dbg = [np.zeros((len(z[m]), 4)) for m in range(M)]
    u1, u2 = C.c_double(), C.c_double()
    for d in range(D):
        span = [(int(c.doc_off[m][d]), int(c.doc_off[m][d + 1])) for m in range(M)]
        docLength = [b_e[1] - b_e[0] for b_e in span]
        localTopicCounts = np.zeros((M, K), dtype=np.int64)
        for m in range(M):
            for i in range(*span[m]):
                if z[m][i] != -1:
                    localTopicCounts[m][z[m][i]] += 1
        localTopicIndex = [t for t in range(K) if localTopicCounts[:, t].any()]
        pd = p[d]
        for m in range(M):
            totalMassOtherModalities = np.zeros(K)
            for topic in localTopicIndex:
                for i in range(M):
                    if i != m and docLength[i] != 0:
                        totalMassOtherModalities[topic] += float(pd[m][i]) * (int(localTopicCounts[i][topic]) + float(gamma[i]) * float(alpha[i][topic])) \
                            / (docLength[i] + float(gamma[i]) * float(alphaSum[i]))
                totalMassOtherModalities[topic] = totalMassOtherModalities[topic] * (docLength[m] + float(gamma[m]) * float(alphaSum[m]))
            newTopicMassAllModalities = 0.0
            for i in range(M):
                newTopicMassAllModalities += float(pd[m][i]) * (float(gamma[i]) * float(alpha[i][K])) / (docLength[i] + float(gamma[i]) * float(alphaSum[i]))
            newTopicMassAllModalities = newTopicMassAllModalities * (docLength[m] + float(gamma[m]) * float(alphaSum[m]))
            for position in range(docLength[m]):
                gi = span[m][0] + position
                type_ = int(c.tokens[m][gi])
                if type_ >= c.V[m]:
                    continue
                oldTopic = int(z[m][gi])
                currentTypeTopicCounts = typeTopicCounts[m][type_]
                tree = trees[m][type_]
                if oldTopic != -1:
                    localTopicCounts[m][oldTopic] -= 1
                    if not localTopicCounts[:, oldTopic].any():
                        localTopicIndex.remove(oldTopic)
                nonZeroTopics = len(localTopicIndex)
                # ---- WRK:496-536 ----
                topicDocWordMass = 0.0
                topicDocWordMasses = np.zeros(max(nonZeroTopics, 1))
                for denseIndex in range(nonZeroTopics):
                    topic = localTopicIndex[denseIndex]
                    n = int(localTopicCounts[m][topic])
                    if useVectorsLambda != 0 and m == 0:
                        p_wt = (useVectorsLambda * (float(expDotProductValues[topic][type_]) / float(sumExpValues[topic])) + (1 - useVectorsLambda)
                                * ((int(currentTypeTopicCounts[topic]) + float(beta[m])) / (int(tokensPerTopic[m][topic]) + float(betaSum[m]))))
                    else:
                        p_wt = (int(currentTypeTopicCounts[topic]) + float(beta[m])) / (int(tokensPerTopic[m][topic]) + float(betaSum[m]))
                    topicDocWordMass += (float(pd[m][m]) * n + float(totalMassOtherModalities[topic])) * p_wt
                    topicDocWordMasses[denseIndex] = topicDocWordMass
                newTopicMass = 0.0 if first_inactive < 0 else newTopicMassAllModalities / K
                L.orc_token_uniforms(int(seed), int(sweep_idx), d, m, position, C.byref(u1), C.byref(u2))
                nextUniform = u1.value
                sample = nextUniform * (newTopicMass + topicDocWordMass + float(tree[1]))
                dbg[m][gi] = (newTopicMass, topicDocWordMass, float(tree[1]), sample)
                if sample < newTopicMass:
                    newTopic = first_inactive
                else:
                    sample -= newTopicMass
                    if sample < topicDocWordMass:
                        newTopic = localTopicIndex[L.orc_lower_bound(topicDocWordMasses.ctypes.data_as(C.c_void_p), sample, nonZeroTopics)]
                    else:
                        newTopic = L.orc_ftree_sample(tree.ctypes.data_as(C.c_void_p), K, u2.value)
                if newTopic == -1:
                    newTopic = K - 1
                z[m][gi] = newTopic
                localTopicCounts[m][newTopic] += 1
    return z, dbg, trees


@pytest.mark.parametrize("lam", [0.3, 1.0])
def test_python_transcription_of_the_reference_lines(lam):
    K, V = 12, [40, 9]
    c = small_corpus(K, V, 8, [14, 3], 23)
    hy = Hyper.defaults(K, V)
    hy.alpha[:] = np.linspace(0.05, 0.4, K + 1)[None, :]
    hy.alpha_sum[:] = hy.alpha[:, :K].sum(axis=1)
    hy.gamma[:] = [1.0, 0.7]
    inactive = np.zeros(K, dtype=np.uint8); inactive[10] = 1
    hy.inactive = inactive
    hy.alpha[:, K] = 3.0
    e, S = table(K, V[0], 5)
    S = S * 1.7                                                     # (accumulated sums: not those of the table)
    r = make_ref(c, hy)
    z0 = [r.get_assignments(m) for m in range(2)]
    for m in range(2):
        z0[m][z0[m] == 10] = 2
        r.set_assignments(m, z0[m])
    r.build_counts()
    r.set_vectors_mix(lam, e, S)
    for it in range(2):
        p = r.draw_p_philox(77, it)
        hy_now = Hyper(r.get_alpha(), hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, r.get_inactive())
        z, dbg, trees = _transcription(r, c, hy_now, lam, e, S, p, it, 77)
        rr = r.sweep(it, 77, p=p, want_dbg=True)
        assert rr["stats"]["aborted_docs"] == 0
        for m in range(2):
            assert np.array_equal(z[m], r.get_assignments(m)), f"lambda {lam} sweep {it} view {m}: decisions"
            assert np.array_equal(dbg[m], rr["dbg"][m]), f"lambda {lam} sweep {it} view {m}: masses"
            for w in range(V[m]):
                assert np.array_equal(trees[m][w], r.get_tree(m, w))
    assert rr["stats"]["new_mass_cnt"] + rr["stats"]["topic_doc_mass_cnt"] + rr["stats"]["word_ftree_mass_cnt"] == rr["stats"]["tokens"]
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) by hand
def test_lambda_one_forgets_the_counts_in_view_0_only():
    K, V = 20, [80, 15]
    c = small_corpus(K, V, 16, [20, 4], 31)
    hy = Hyper.defaults(K, V)
    e, S = table(K, V[0], 9)
    a, b, off = make_ref(c, hy), make_ref(c, hy), make_ref(c, hy)
    a.set_vectors_mix(1.0, e, S); b.set_vectors_mix(1.0, e, S)
    rng = np.random.RandomState(1)
    nwk0, nk0 = b.get_counts(0)
    other = rng.randint(0, 50, nwk0.shape).astype(np.int32)        # other view-0 counts under the same assignments
    b.set_counts(0, other, other.sum(axis=0).astype(np.int32))
    p = a.draw_p_philox(3, 0)
    ra = a.sweep(0, 3, p=p, flags=2, want_dbg=True); rb = b.sweep(0, 3, p=p, flags=2, want_dbg=True)
    roff = off.sweep(0, 3, p=p, flags=2, want_dbg=True)
    assert np.array_equal(ra["dbg"][0], rb["dbg"][0]), "view-0 masses depend on n_wk at lambda = 1"
    assert np.array_equal(a.get_assignments(0), b.get_assignments(0))
    assert not np.array_equal(ra["dbg"][0], roff["dbg"][0])
    for w in range(V[0]):
        assert np.array_equal(a.get_tree(0, w), b.get_tree(0, w))
        # p_wt = 1 * (e / S) + 0 * ratio: the leaf is gamma * alpha_k * (e / S) exactly
        want = hy.gamma[0] * hy.alpha[0, :K] * (1.0 * (e[:, w] / S) + 0.0)
        assert np.array_equal(a.get_tree(0, w)[K:], want)
    for w in range(V[1]):                                           # views m > 0: the trees of lambda = 0
        assert np.array_equal(a.get_tree(1, w), off.get_tree(1, w))
    # an entity's view-1 tokens see the mix only through its view-0 decisions: where those agree, so do the view-1 masses
    z_on, z_off = a.get_assignments(0), off.get_assignments(0)
    for d in range(c.D):
        s0 = slice(int(c.doc_off[0][d]), int(c.doc_off[0][d + 1])); s1 = slice(int(c.doc_off[1][d]), int(c.doc_off[1][d + 1]))
        if np.array_equal(z_on[s0], z_off[s0]):
            assert np.array_equal(ra["dbg"][1][s1], roff["dbg"][1][s1])
    for o in (a, b, off):
        o.close()


@pytest.mark.parametrize("lam", [0.25, 0.5])
def test_flat_table_root_in_closed_form(lam):
    K, V = 13, [30, 7]
    c = small_corpus(K, V, 10, [15, 3], 41)
    hy = Hyper.defaults(K, V)
    hy.alpha[:] = np.linspace(0.02, 0.5, K + 1)[None, :]
    hy.gamma[:] = [0.9, 1.0]
    r = make_ref(c, hy)
    cval = 1.0 / 64                                                 # e / S = c for every cell (exactly: powers of two)
    e = np.full((K, V[0]), 0.5); S = np.full(K, 32.0)
    r.set_vectors_mix(lam, e, S)
    assert np.array_equal(r.mix, np.full((V[0], K), lam * cval))
    assert np.array_equal(make_mix(lam, e, S), r.mix)
    r.build_trees()
    nwk, nk = r.get_counts(0)
    for w in range(V[0]):
        q = (nwk[w] + hy.beta[0]) / (nk + hy.beta_sum[0])
        t = np.zeros(2 * K)
        t[K:] = hy.gamma[0] * hy.alpha[0, :K] * (lam * cval + (1 - lam) * q)
        for i in range(K - 1, 0, -1):                               # FT:96-109: the tree's own pairwise order
            t[i] = t[2 * i] + t[2 * i + 1]
        got = r.get_tree(0, w)
        assert got[1] == t[1] and np.array_equal(got[1:], t[1:]), w
    r.close()
