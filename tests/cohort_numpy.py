"""TEST INFRASTRUCTURE ONLY: the literal restatement of mvhdp_cohort_top_words (include/mvhdp.h) in numpy and Python integers.  Listing by
listing and token by token in the contract's words; the share order compares two rationals by `int` cross products, never by a float."""
from functools import cmp_to_key

import numpy as np

BY_COUNT, BY_SHARE = "count", "share"


class StateError(Exception):
    """what the entry answers with MVHDP_ERR_STATE"""


class Counted:
    """c [G][V][K], tokens [G][K], docs [G][K] (int64), skipped and counted (int) of one view and one list of cohorts"""

    def __init__(self, c, tokens, docs, skipped):
        self.c, self.tokens, self.docs, self.skipped = c, tokens, docs, skipped
        self.counted = int(tokens.sum())
        self.nonzero = (c >= 1).sum(axis=1).astype(np.int32)


def count(K, V, doc_off, tok, z, cohorts):
    """every listing of every cohort: a token is counted when 0 <= type < V and 0 <= z < K, skipped when z == -1 or type >= V; a z
    outside [-1, K) or a negative type is an error"""
    G = len(cohorts)
    c = np.zeros((G, V, K), dtype=np.int64)
    tokens = np.zeros((G, K), dtype=np.int64)
    docs = np.zeros((G, K), dtype=np.int64)
    skipped = 0
    for g, members in enumerate(cohorts):
        for d in members:
            seen = set()
            for i in range(int(doc_off[d]), int(doc_off[d + 1])):
                w, k = int(tok[i]), int(z[i])
                if k < -1 or k >= K or w < 0:
                    raise StateError((g, d, i, w, k))
                if k == -1 or w >= V:
                    skipped += 1
                    continue
                c[g, w, k] += 1
                tokens[g, k] += 1
                seen.add(k)
            for k in seen:
                docs[g, k] += 1
    return Counted(c, tokens, docs, skipped)


def _by_count(a, b):
    """a before b: count descending, equal counts by descending type id; entries are (type, count, global count)"""
    if a[1] != b[1]:
        return -1 if a[1] > b[1] else 1
    return -1 if a[0] > b[0] else (1 if a[0] < b[0] else 0)


def _by_share(a, b):
    """a before b: c_a / n_a against c_b / n_b by cross products of Python integers; equal shares by count, then by type id, descending"""
    l, r = a[1] * b[2], b[1] * a[2]
    if l != r:
        return -1 if l > r else 1
    return _by_count(a, b)


def select(counted, n, order=BY_COUNT, min_count=1, nwk=None):
    """(types [G][K][n] with -1 in the unfilled slots, counts [G][K][n] with 0 there), int32; nwk [V][K]: the global counts (BY_SHARE)"""
    G, V, K = counted.c.shape
    types = np.full((G, K, n), -1, dtype=np.int32)
    counts = np.zeros((G, K, n), dtype=np.int32)
    cmp = _by_share if order == BY_SHARE else _by_count
    for g in range(G):
        for k in range(K):
            col = counted.c[g, :, k]
            ent = [(int(w), int(col[w]), int(nwk[w, k]) if order == BY_SHARE else 1) for w in np.flatnonzero(col >= min_count)]
            ent.sort(key=cmp_to_key(cmp))
            for i, (w, cnt, _) in enumerate(ent[:n]):
                types[g, k, i], counts[g, k, i] = w, cnt
    return types, counts


def cohort_top_words(K, V, doc_off, tok, z, cohorts, n=20, order=BY_COUNT, min_count=1, nwk=None):
    """the whole call: (types, counts, nonzero, tokens, docs, Counted)"""
    cd = count(K, V, doc_off, tok, z, cohorts)
    types, counts = select(cd, n, order, min_count, nwk)
    return types, counts, cd.nonzero, cd.tokens, cd.docs, cd


def recount(K, V, tok, z):
    """n_wk [V][K] and n_k [K] of one view from its tokens, as a plain recount gives them (tokens that the entry would skip left out)"""
    tok, z = np.asarray(tok), np.asarray(z)
    ok = (z >= 0) & (z < K) & (tok >= 0) & (tok < V)
    nwk = np.zeros((V, K), dtype=np.int64)
    np.add.at(nwk, (tok[ok], z[ok]), 1)
    return nwk, nwk.sum(axis=0)


def top_words(nwk, n):
    """mvhdp_top_words of a count table: (types [K][n], counts [K][n], nonzero [K])"""
    V, K = nwk.shape
    types = np.full((K, n), -1, dtype=np.int32)
    counts = np.zeros((K, n), dtype=np.int32)
    for k in range(K):
        ent = sorted(((int(w), int(nwk[w, k]), 1) for w in np.flatnonzero(nwk[:, k] > 0)), key=cmp_to_key(_by_count))
        for i, (w, cnt, _) in enumerate(ent[:n]):
            types[k, i], counts[k, i] = w, cnt
    return types, counts, (nwk > 0).sum(axis=0).astype(np.int32)
