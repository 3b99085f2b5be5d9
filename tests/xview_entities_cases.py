"""Inputs of the entities-for-an-item tests, made on the host alone: the multi-view corpora of tests/xview_cases.py, query sets over the
predicted view (one item, weighted sets with repeats, a weight of 0, an empty query), a corpus with a run of identical entities (equal
theta rows, hence equal scores for every query), and (query, entity) pairs.  Test infrastructure."""
import copy

import numpy as np

from tests import xview_cases as xc

K_VALUES = [1, 15, 16, 17, 64, 100, 400]         # 15, 16, 17: at the slab of 16 topics
NQ_VALUES = [1, 63, 64, 65, 129, 130]            # at the 64-row and the 128-column tile border
CAND_VALUES = [1, 127, 128, 129, 300]
D, VM = 300, 127
# (K, nq, candidates): every K, every nq and every candidate count at least once, the three sets crossed where tiles and slabs meet
SHAPES = ([(K, 65, 300) for K in K_VALUES] + [(17, nq, 129) for nq in NQ_VALUES] + [(64, 63, C) for C in CAND_VALUES]
          + [(16, 64, 128), (15, 130, 127), (100, 129, 300), (400, 1, 1)])


def make(K, D=D, Vm=VM, M=3, seed=0, inactive=None):
    return xc.make(K, Vm, D, M, seed=seed, inactive=inactive)


def queries(c, nq, seed=0):
    """(items, weights): nq lists over view m's types.  Query 0 is a single item; then, in turn: one item, a weighted set of 2..6 items
    with a repeat, a set with a weight of exactly 0.0, and (once, when nq > 4) an empty query."""
    rng = np.random.default_rng(77 + seed + nq)
    V = c.V[c.m]
    items, weights = [], []
    for j in range(nq):
        kind = j % 4 if j else 0
        if j == 4:
            items.append([]); weights.append([])
            continue
        if kind in (0, 1) or V == 1:
            items.append([int(rng.integers(0, V))]); weights.append([1.0])
            continue
        n = int(rng.integers(2, 7))
        q = [int(x) for x in rng.integers(0, V, n)]
        q[-1] = q[0]                                                         # a repeated item: each occurrence adds
        w = [float(x) for x in rng.choice([0.5, 1.0, 2.0, 3.0, 0.3], n)]
        if kind == 3:
            w[1] = 0.0
        items.append(q); weights.append(w)
    return items, weights


def pairs(c, nq, c0, c1, n, items, seed=0):
    """(query [n], entity [n]): unsorted, with repeats; a share of them entities that hold an item of the query (excluded themselves)"""
    rng = np.random.default_rng(5 + seed)
    q = rng.integers(0, nq, n).astype(np.int64)
    e = rng.integers(c0, c1, n).astype(np.int64)
    off, tok = c.doc_off[c.m], c.tokens[c.m]
    for i in range(0, n, 3):
        if not items[q[i]]:
            continue
        holders = [d for d in range(c0, c1) if np.isin(tok[off[d]:off[d + 1]], items[q[i]]).any()]
        if holders:
            e[i] = holders[int(rng.integers(0, len(holders)))]
    q[n // 2:n // 2 + 2] = q[0]; e[n // 2:n // 2 + 2] = e[0]                 # the same pair three times
    return q, e


def with_clones(c, first, count, template=None):
    """a copy of the case in which the entities [first, first + count) hold, in every view, the document of `template` (an entity with
    every view present, so nothing is carried over): identical theta rows"""
    if template is None:
        template = next(d for d in range(c.D) if d not in (c.full, c.no_target, c.no_source) and not (first <= d < first + count)
                        and all(c.doc_off[v][d + 1] > c.doc_off[v][d] for v in range(c.M)))
    out = copy.copy(c)
    out.doc_off, out.tokens, out.z = [], [], []
    for v in range(c.M):
        off = c.doc_off[v]
        spans_t = [c.tokens[v][off[d]:off[d + 1]] for d in range(c.D)]
        spans_z = [c.z[v][off[d]:off[d + 1]] for d in range(c.D)]
        for d in range(first, first + count):
            spans_t[d], spans_z[d] = spans_t[template], spans_z[template]
        out.doc_off.append(np.concatenate([[0], np.cumsum([len(s) for s in spans_t])]).astype(np.int64))
        out.tokens.append(np.concatenate(spans_t).astype(np.int32))
        out.z.append(np.concatenate(spans_z).astype(np.int32))
    return out, template
