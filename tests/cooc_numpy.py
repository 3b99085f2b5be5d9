"""TEST INFRASTRUCTURE ONLY: the literal restatement of mvhdp_word_cooccurrence (include/mvhdp.h) in numpy and Python integers.  Entity by
entity and window start by window start in the contract's words: the set of types in the window, their memberships, one per pair of
present slots.  Nothing is carried from one window to the next except a memo of windows that hold the same set of listed types."""
from types import SimpleNamespace

import numpy as np


class NegativeType(Exception):
    """what the entry answers with MVHDP_ERR_INVALID_ARG (the caller's corpus) or MVHDP_ERR_STATE (the handle's)"""


def memberships(sets, V):
    """the inverted index of the sets: type w sits in (ms[i], mj[i]) for i in first[w] .. first[w + 1]; listed [V]"""
    filled = np.argwhere(sets >= 0)
    types = sets[filled[:, 0], filled[:, 1]]
    assert (types < V).all() and (sets >= -1).all()
    o = np.argsort(types, kind="stable")
    mt = types[o]
    listed = np.zeros(V, dtype=bool)
    listed[mt] = True
    return filled[o, 0].astype(np.int64), filled[o, 1].astype(np.int64), np.searchsorted(mt, np.arange(V + 1)), listed


def cooc(V, doc_off, tok, sets, window=0, d0=0, d1=None):
    """the whole call: co [S][n][n] int64, windows, and the stats, as a namespace"""
    sets = np.asarray(sets, dtype=np.int64)
    S, n = sets.shape
    doc_off, tok = np.asarray(doc_off, dtype=np.int64), np.asarray(tok, dtype=np.int64)
    D = len(doc_off) - 1
    d1 = D if d1 is None else d1
    assert 0 <= d0 <= d1 <= D and window >= 0 and 1 <= n <= 64
    ms, mj, first, listed = memberships(sets, V)
    co = np.zeros(S * n * n, dtype=np.int64)
    r = SimpleNamespace(windows=0, entities=0, tokens=0, hits=0, oov=0, distinct_words=int(listed.sum()), memberships=len(ms))
    memo = {}
    for d in range(d0, d1):
        span = tok[doc_off[d]:doc_off[d + 1]]
        L = len(span)
        if L == 0:
            continue
        if (span < 0).any():
            raise NegativeType(d)
        r.entities += 1
        r.tokens += L
        r.oov += int((span >= V).sum())
        r.hits += int(listed[span[span < V]].sum())
        W = L if window == 0 else window
        for i in range(max(L - W, 0) + 1):
            r.windows += 1
            types = np.unique(span[i:min(i + W, L)])
            types = types[types < V]
            types = types[listed[types]]
            if len(types) == 0:
                continue
            key = types.tobytes()
            cells = memo.get(key)
            if cells is None:
                at = np.concatenate([np.arange(first[t], first[t + 1]) for t in types])
                s, j = ms[at], mj[at]
                o = np.argsort(s, kind="stable")
                s, j = s[o], j[o]                                            # the present slots, set by set
                start = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
                size = np.diff(np.r_[start, len(s)])
                begin, count = np.repeat(start, size), np.repeat(size, size)  # per present slot: its set's run of present slots
                a = np.repeat(np.arange(len(s)), count)
                b = begin[a] + np.arange(len(a)) - np.repeat(np.cumsum(count) - count, count)
                cells = (s[a] * n + j[a]) * n + j[b]                         # every pair of present slots of a set, (i, i) included
                memo[key] = cells
            co[cells] += 1
    r.co = co.reshape(S, n, n)
    return r
