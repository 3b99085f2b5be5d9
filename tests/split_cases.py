"""Inputs of the split tests (mvhdp_split_topic), made on the host alone.  Test infrastructure.

The corpora are those of tests/remap_cases.py (200 entities, a few thousand tokens; its geometric topic draw makes topic 0 heavy: the
source) with entities appended whose shapes the device code can trip on:
  an entity of view 0 whose 65 tokens all carry the source (one record more than a wave's chunk);
  an entity with 1500 source tokens among 1600 in view 0 (crosses every chunk of 64, every tile of 1024 tokens and several blocks);
  an entity whose only source tokens sit in the last view while its view 0 is empty (M > 1);
  an entity with source tokens in all three views, so that the coupling acts (M == 3);
and the last type of view 0 carries the source wherever it occurs, so that c_w - own reaches 0.  The free topic a split may take is the
inactive last one (at K >= 63 the middle one too: the one target = -1 picks); at K == 2 topic 1 is emptied into that role.
DOC_ID_BASE is the shifted base of the restatement's tests (the high counter word is not zero); a handle admits doc_id_base + D < 2^29
only (mvhdp_set_corpus), so the device tests take HANDLE_DOC_ID_BASE, the largest base their corpus fits under."""
from types import SimpleNamespace

import numpy as np

from mvtopicmodel_amd.native import Hyper
from tests import remap_cases as rc

K_VALUES = [2, 65, 2048]
M_VALUES = [1, 3]
ITERATIONS = [0, 1, 5]
DOC_ID_BASE = 2 ** 32 + 5
SOURCE = 0


def handle_doc_id_base(c):
    return 2 ** 29 - 1 - c.D


def make(K, M, seed=0, new_mass=0.05):
    c = rc.make(K, M, seed=seed, inactive=True, unassigned=True, new_mass=new_mass, empty_view=-1)
    rng = np.random.default_rng(104729 * K + 17 * M + seed)
    other = 1 if K > 2 else -1                               # K == 2 has no second topic in use: those tokens are unassigned
    if K == 2:                                               # topic 1 becomes the free, inactive index
        for m in range(M):
            c.z[m][c.z[m] == 1] = 0
        c.hy.alpha[:, 1] = 0.0
        c.hy.alpha_sum[:] = c.hy.alpha[:, :K].sum(1)
        c.hy.inactive[1] = 1
    c.z[0][c.tokens[0] == c.V[0] - 1] = SOURCE               # a type that occurs in the source alone

    def types(m, n):
        return np.minimum(rng.geometric(min(0.5, 6.0 / c.V[m]), n) - 1, c.V[m] - 1).astype(np.int32)

    def entity(spec):
        """spec: per view (tokens, source tokens among them), scattered"""
        out = []
        for m in range(M):
            n, ns = spec.get(m, (0, 0))
            z = np.full(n, other, dtype=np.int32)
            z[rng.permutation(n)[:ns]] = SOURCE
            t = types(m, n)
            if m == 0:
                t[(t == c.V[0] - 1) & (z != SOURCE)] = 0     # the source-only type stays the source's
            out.append((t, z))
        return out

    extra = [entity({0: (65, 65)}), entity({0: (1600, 1500)})]
    if M > 1:
        extra.append(entity({M - 1: (7, 7)}))
    if M == 3:
        e = entity({0: (30, 20), 1: (9, 6), 2: (5, 5)})
        e[0][0][0] = c.V[0] - 1; e[0][1][0] = SOURCE         # the source-only type occurs at least once
        extra.append(e)
    else:
        e = entity({0: (3, 3)})
        e[0][0][0] = c.V[0] - 1
        extra.append(e)
    for m in range(M):
        lens = np.concatenate([np.diff(c.doc_off[m]), [len(e[m][0]) for e in extra]])
        c.doc_off[m] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        c.tokens[m] = np.concatenate([c.tokens[m]] + [e[m][0] for e in extra]).astype(np.int32)
        c.z[m] = np.concatenate([c.z[m]] + [e[m][1] for e in extra]).astype(np.int32)
    c.D = rc.D + len(extra)
    c.source = SOURCE
    c.free = [k for k in range(K) if c.hy.inactive[k]]        # every inactive topic of these cases is free
    c.special = dict(all65=rc.D, long1500=rc.D + 1, side_only=rc.D + 2 if M > 1 else None, all_views=rc.D + 3 if M == 3 else None)
    return c


def hints(c, seed=0):
    """a hint row for view 0 (a fifth of the types pinned to a, a fifth to b), none for the other views"""
    rng = np.random.default_rng(seed + 5)
    r = rng.random(c.V[0])
    row = np.full(c.V[0], -1, dtype=np.int8)
    row[r < 0.2] = 0
    row[r > 0.8] = 1
    return [row] + [None] * (c.M - 1)


def coupling(M, seed=0):
    """a non-default coupling: not symmetric, a zero off the diagonal, a diagonal that is not 1"""
    rng = np.random.default_rng(seed + 11)
    P = 0.1 + rng.random((M, M))
    if M > 1:
        P[0, M - 1] = 0.0
    return P


def planted(hinted=True, seed=0, D=200, K=8):
    """Topic 0 is the union of two disjoint vocabularies (types 0..19 and 20..39 of one view), every entity draws its topic-0 tokens from
    one of them only; the other topics live on types 40..59.  Two anchor types of each vocabulary are hinted: 0, 1 stay (a), 20, 21 go
    (b).  want_side[w] is the side of a topic-0 type's vocabulary."""
    rng = np.random.default_rng(977 + seed)
    V = [60]
    lens0 = rng.integers(10, 30, D)
    lens1 = rng.integers(5, 15, D)
    toks, zs = [], []
    for d in range(D):
        lo = 0 if d % 2 == 0 else 20
        t0 = rng.integers(lo, lo + 20, lens0[d])
        t1 = rng.integers(40, 60, lens1[d])
        t = np.concatenate([t0, t1]); zz = np.concatenate([np.zeros(lens0[d], np.int64), rng.integers(1, K - 1, lens1[d])])
        p = rng.permutation(len(t))
        toks.append(t[p]); zs.append(zz[p])
    off = np.concatenate([[0], np.cumsum(lens0 + lens1)]).astype(np.int64)
    hy = Hyper.defaults(K, V)
    hy.alpha[:, K - 1] = 0.0
    hy.alpha_sum[:] = hy.alpha[:, :K].sum(1)
    hy.inactive = np.zeros(K, dtype=np.uint8)
    hy.inactive[K - 1] = 1
    c = SimpleNamespace(K=K, M=1, V=V, D=D, doc_off=[off], tokens=[np.concatenate(toks).astype(np.int32)], z=[np.concatenate(zs).astype(np.int32)],
                        hy=hy, source=0, free=[K - 1])
    row = np.full(60, -1, dtype=np.int8)
    if hinted:
        row[[0, 1]] = 0
        row[[20, 21]] = 1
    c.hint = [row]
    c.want_side = np.concatenate([np.zeros(20, np.int8), np.ones(20, np.int8), np.full(20, -1, np.int8)])
    return c


def purity(c, z_after, target):
    """the share of the split set that lies with its vocabulary's anchors"""
    on = c.z[0] == c.source
    side = (z_after[0][on] == target).astype(np.int8)
    return float((side == c.want_side[c.tokens[0][on]]).mean())
