"""Inputs of the remap tests (mvhdp_remap_topics), made on the host alone.  Test infrastructure.

Corpora of a few hundred entities and a few thousand tokens whose shapes sit on the borders of the device code: K around the 64 lanes of
a wave, more than one cell per lane and the limit of 2048; one and three views, one of them without a token; spans of 0, 1 and 65 tokens;
view lengths that are no multiple of the four tokens of a 16-byte load (a tail of 1, 2 and 3 tokens over the views; every view's z is an
allocation of its own and starts on a 16-byte border, so no call through the ABI gives the loop a head); some tokens unassigned; one or
two inactive topics."""
from types import SimpleNamespace

import numpy as np

from mvtopicmodel_amd.native import Hyper

K_VALUES = [1, 2, 63, 64, 65, 100, 257, 2048]
M_VALUES = [1, 3]
SPANS = [0, 1, 65]                                           # view 0 holds an entity of each length
D = 200
MAP_NAMES = ["identity", "pair", "cycle", "reversal", "onto_one", "drop_all", "across_lanes", "mixed", "chain"]


def make(K, M, seed=0, inactive=True, unassigned=True, new_mass=0.05, empty_view=None):
    """A corpus of M views over D entities.  empty_view: the view without a token (default: view 1 of three when K is even).  Topics are
    geometric draws over the active topics, so a few topics are heavy and the tail is thin or empty.  inactive: the last topic, and at
    K >= 63 the middle one too, are inactive and hold nothing.  alpha is different in every cell, so that a moved cell shows."""
    rng = np.random.default_rng(7919 * K + 31 * M + seed)
    if empty_view is None:
        empty_view = 1 if (M == 3 and K % 2 == 0) else -1
    off_topics = ([K - 1] + ([K // 2] if K >= 63 else [])) if (inactive and K >= 3) else []
    active = np.array([k for k in range(K) if k not in off_topics], dtype=np.int32)
    V = [max(3, min(97, 2 * K + 1)), 11, 5][:M]
    c = SimpleNamespace(K=K, M=M, V=V, D=D, doc_off=[], tokens=[], z=[])
    for m in range(M):
        lens = rng.integers(0, [24, 8, 4][m], D)
        lens[rng.random(D) < 0.1] = 0
        if m == 0:
            lens[rng.permutation(D - 10)[:len(SPANS)]] = SPANS           # (the last entities take the tail tokens below)
        if m == empty_view:
            lens[:] = 0
        elif int(lens.sum()) % 4 != 1 + m % 3:               # a tail of 1, 2 or 3 tokens behind the last 16-byte load
            lens[D - 1 - m] += (1 + m % 3 - int(lens.sum())) % 4
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        N = int(off[-1])
        tok = np.minimum(rng.geometric(min(0.5, 6.0 / V[m]), N) - 1, V[m] - 1).astype(np.int32)
        z = active[np.minimum(rng.geometric(min(0.5, 8.0 / len(active)), N) - 1, len(active) - 1)].astype(np.int32)
        if unassigned and N > 20:
            z[rng.permutation(N)[:5]] = -1
        c.doc_off.append(off); c.tokens.append(tok); c.z.append(z)
    hy = Hyper.defaults(K, V)
    hy.alpha[:, :K] = 0.01 + 0.2 * rng.random((M, K))
    hy.alpha[:, K] = new_mass
    hy.alpha[:, off_topics] = 0.0
    hy.alpha_sum[:] = hy.alpha[:, :K].sum(1)
    hy.inactive = np.zeros(K, dtype=np.uint8)
    hy.inactive[off_topics] = 1
    c.hy = hy
    return c


def merge_and_drop(K):
    """the map of the chain tests (K >= 8): topics 1 and 2 merge into 0, topic 3 is dropped, topic 5 moves onto the emptied 1"""
    t = np.arange(K, dtype=np.int32)
    t[1] = 0; t[2] = 0; t[3] = -1; t[5] = 1
    return t


def maps(K):
    """name -> map [K] int32; a map that needs more topics than K has is left out"""
    ident = np.arange(K, dtype=np.int32)
    out = {"identity": ident.copy(), "reversal": ident[::-1].copy(), "onto_one": np.full(K, K // 2, dtype=np.int32),
           "drop_all": np.full(K, -1, dtype=np.int32), "cycle": np.roll(ident, -1)}          # cycle: k -> k + 1, K - 1 -> 0
    if K >= 2:
        pair = ident.copy(); pair[1] = 0
        out["pair"] = pair
    if K >= 3:
        chain = ident.copy(); chain[0] = 1; chain[1] = 2     # [1, 2, 2, 3, ...]: topic 0's tokens stop at 1
        out["chain"] = chain
    if K >= 65:
        across = ident.copy(); across[[0, 1, 63, 64]] = 64   # sources on both sides of the 64th lane, onto a second cell of lane 0
        out["across_lanes"] = across
    if K >= 8:
        mixed = merge_and_drop(K)
        mixed[6], mixed[7] = 7, 6                            # and a swap
        mixed[K - 1] = 4 if K > 8 else mixed[K - 1]          # the inactive last topic joins an active one
        out["mixed"] = mixed
    assert set(out) <= set(MAP_NAMES)
    return out


def split(c, at):
    """the two shards of a case: entities [0, at) and [at, D), each a case of its own (doc_id_base = its first entity)"""
    parts = []
    for lo, hi in ((0, at), (at, c.D)):
        p = SimpleNamespace(K=c.K, M=c.M, V=c.V, D=hi - lo, hy=c.hy, base=lo, doc_off=[], tokens=[], z=[])
        for m in range(c.M):
            a, b = int(c.doc_off[m][lo]), int(c.doc_off[m][hi])
            p.doc_off.append((c.doc_off[m][lo:hi + 1] - a).astype(np.int64))
            p.tokens.append(c.tokens[m][a:b].copy()); p.z.append(c.z[m][a:b].copy())
        parts.append(p)
    return parts
