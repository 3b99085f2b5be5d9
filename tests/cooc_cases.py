"""Inputs of the word co-occurrence tests (mvhdp_word_cooccurrence), made on the host alone.  Test infrastructure.

The hand-sized corpus of tests/test_cooc_kats.py is HAND_*.  The device cases are those of tests/cohort_cases.py (spans of 0, 1, 64, 65 and
700 tokens, holes with out-of-vocabulary types) with one entity of 4 100 tokens appended to every view, so that an entity crosses every
chunk of window starts and every upload chunk of a caller's corpus."""
import numpy as np

from tests import cohort_cases as cc

V_VALUES = cc.V_VALUES
LONG = 4100

# ---- the hand-sized corpus: 5 entities over V = 6 ------------------------------------------------------------------------------------
HAND_V = 6
# spans of 0, 1, 3, 4 and 7 tokens; type 7 is out of the vocabulary; entity 3 repeats word 1 inside a window of two; entity 4 holds word 0 at
# both ends
HAND_DOCS = [[], [2], [0, 7, 1], [1, 1, 3, 0], [0, 2, 4, 2, 3, 1, 0]]
HAND_SETS = [[0, 1, -1], [2, 3, 5], [0, -1, 0]]


def hand_corpus():
    off = np.concatenate([[0], np.cumsum([len(d) for d in HAND_DOCS])]).astype(np.int64)
    return off, np.array([t for d in HAND_DOCS for t in d], dtype=np.int32)


# ---- device cases ---------------------------------------------------------------------------------------------------------------------
def make(K, V, seed=0, holes=True):
    """cohort_cases.make(K, V) with an entity of LONG tokens behind the others in views 0 and 1 (3 tokens in the further views)"""
    c = cc.make(K, V, seed=seed, holes=holes)
    rng = np.random.default_rng(77 * K + V[0] + seed)
    for m in range(c.M):
        L = LONG if m < 2 else 3
        tok = np.minimum(rng.geometric(min(0.5, 8.0 / V[m]), L) - 1, V[m] - 1).astype(np.int32)
        z = np.minimum(rng.geometric(min(0.5, 6.0 / K), L) - 1, K - 1).astype(np.int32)
        if holes and m < 2:
            tok[[5, LONG // 2]] = V[m] + 2
        c.doc_off[m] = np.concatenate([c.doc_off[m], [c.doc_off[m][-1] + L]]).astype(np.int64)
        c.tokens[m] = np.concatenate([c.tokens[m], tok])
        c.z[m] = np.concatenate([c.z[m], z])
    c.D += 1
    return c


def frequencies(c, m):
    t = c.tokens[m]
    return np.bincount(t[t < c.V[m]], minlength=c.V[m])


def special_sets(c, m, n):
    """Seven rows of n slots: all empty; a row with an empty slot in the middle; a single word; the most frequent word in two slots of one
    row; a word that never occurs (where there is one, else the rarest); n distinct words (as many as V allows); the rarest words.
    Returns (rows [7][n], the most frequent word, the never-occurring word or None)."""
    V = c.V[m]
    f = frequencies(c, m)
    by_freq = np.argsort(-f, kind="stable")
    hot = int(by_freq[0])
    never = int(np.flatnonzero(f == 0)[0]) if (f == 0).any() else None
    rows = np.full((7, n), -1, dtype=np.int32)
    k = min(n, V)
    rows[1, :k] = by_freq[:k]
    if n >= 3:
        rows[1, n // 2] = -1
    rows[2, n - 1] = by_freq[min(1, V - 1)]
    rows[3, 0] = hot
    rows[3, n - 1] = hot
    if n >= 3:
        rows[3, 1] = by_freq[min(2, V - 1)]
    rows[4, 0] = never if never is not None else by_freq[-1]
    if n >= 2:
        rows[4, 1] = hot
    rows[5, :k] = np.arange(V - k, V)[::-1]
    rows[6, :k] = by_freq[::-1][:k]
    return rows, hot, never


def with_hot_word(sets, hot):
    """the same rows with the most frequent word in the last slot of every row: one hot cell per set"""
    out = np.array(sets, dtype=np.int32, copy=True)
    out[:, -1] = hot
    return out
