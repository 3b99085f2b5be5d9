"""Cases shared by the CPU and the GPU tests of mvhdp_fold_in: document batches over M views with the span lengths at which the kernel
changes its path, views missing for some documents or for all, out-of-vocabulary tokens at chosen places; a random frozen model for the
tests that need no device; and the peaked one-token model whose topic frequencies are known exactly."""
import math

import numpy as np

from tests import foldin_ref as fr

LENGTHS = [0, 1, 2, 63, 64, 65, 200]
SIDE_LENGTHS = [0, 0, 1, 2, 6, 63, 64, 65, 200]               # a side view is missing for about a fifth of the documents


def foldin_docs(V, n_docs=40, seed=1, lengths=LENGTHS, null_view=None):
    """(doc_off, tokens), two lists of length M.  View 0's spans take every length of `lengths` at least once, the other views' spans are
    drawn from SIDE_LENGTHS (0 = the document lacks the view); one document has every span empty; view `null_view` is None: no document
    has it.  Per view every second span of length >= 2 gets an out-of-vocabulary token (V_m, V_m + 7 or 2^31 - 1) at its first, a middle or
    its last position, and one span of length 2 of view 0 is out of vocabulary throughout."""
    rng = np.random.default_rng(seed)
    M = len(V)
    assert n_docs > len(lengths) + 1
    lens0 = np.array(list(lengths) + list(rng.choice(lengths, n_docs - len(lengths))))
    rng.shuffle(lens0)
    offs, toks = [], []
    empty_doc = int(np.flatnonzero(lens0 == 0)[0])
    for m in range(M):
        if m == null_view:
            offs.append(None); toks.append(None)
            continue
        lens = lens0.copy() if m == 0 else rng.choice(SIDE_LENGTHS, n_docs)
        lens[empty_doc] = 0
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        tok = rng.integers(0, V[m], off[-1]).astype(np.int32)
        oov = [V[m], V[m] + 7, 2 ** 31 - 1]
        marked = 0
        for i, d in enumerate(d for d in range(n_docs) if lens[d] >= 2):
            if i % 2 == 0:
                L = int(lens[d])
                tok[off[d] + [0, L // 2, L - 1][marked % 3]] = oov[marked % 3]
                marked += 1
        if m == 0:
            twos = [d for d in range(n_docs) if lens[d] == 2]
            tok[off[twos[-1]]:off[twos[-1] + 1]] = V[m]
            assert marked >= 3
        offs.append(off); toks.append(tok)
    return offs, toks


def slice_docs(offs, toks, a, b):
    """documents [a, b) of a batch, as a batch of their own"""
    so, st = [], []
    for o, t in zip(offs, toks):
        if o is None:
            so.append(None); st.append(None)
        else:
            so.append(o[a:b + 1] - o[a]); st.append(t[o[a]:o[b]])
    return so, st


def random_model(K, V, seed=0, inactive=None):
    """a frozen model that needs no device: random counts, uneven alpha, gamma != 1, alphaSum != sum(alpha), betaSum = beta * V"""
    rng = np.random.default_rng(seed)
    M = len(V)
    nwk = [rng.integers(0, 30, (v, K)).astype(np.int32) for v in V]
    nk = np.stack([x.sum(0) for x in nwk]).astype(np.int32)
    beta = np.linspace(0.01, 0.02, M)
    alpha = rng.uniform(0.05, 0.15, (M, K))
    p_a = np.full((M, M), 0.2); p_b = np.full((M, M), 1.0)
    if M > 1:
        p_a[0, M - 1] = 0.0                                                  # a zero of the default coupling
    return fr.Model(nwk, nk, beta, beta * np.array(V), np.linspace(0.8, 0.9, M), alpha, alpha.sum(1) * 1.25,
                    None if inactive is None else np.asarray(inactive, dtype=np.uint8), p_a, p_b)


# ---- one view, K = 3, one-token documents: the topic of the only visit is drawn from a_0[k] * phi[k] / total exactly ------------------
PEAKED_NWK = np.array([[90, 5, 5], [2, 3, 95]], dtype=np.int32)             # word 0 lives in topic 0
PEAKED_NK = PEAKED_NWK.sum(0).astype(np.int32)
PEAKED_BETA = 0.01
PEAKED_ALPHA = np.array([0.05, 0.05, 0.05])
PEAKED_ALPHA_SUM = 0.15
PEAKED_GAMMA = 0.9
PEAKED_D = 20000


def peaked_model():
    return fr.Model([PEAKED_NWK], PEAKED_NK[None, :], np.array([PEAKED_BETA]), np.array([PEAKED_BETA * 2]), np.array([PEAKED_GAMMA]),
                    PEAKED_ALPHA[None, :], np.array([PEAKED_ALPHA_SUM]), None, np.array([[0.2]]), np.array([[1.0]]))


def peaked_docs():
    return [np.arange(PEAKED_D + 1, dtype=np.int64)], [np.zeros(PEAKED_D, dtype=np.int32)]


def peaked_expectation():
    """(exact topic probabilities of the one visit, five binomial standard deviations per topic at PEAKED_D draws, the prior alone)"""
    a = PEAKED_GAMMA * PEAKED_ALPHA
    phi = (PEAKED_NWK[0] + PEAKED_BETA) / (PEAKED_NK + PEAKED_BETA * 2)
    p = a * phi / (a * phi).sum()
    half = 5 * np.sqrt(p * (1 - p) / PEAKED_D)
    return p, half, a / a.sum()


def frequencies(z0):
    return np.bincount(z0, minlength=3)[:3] / len(z0)
