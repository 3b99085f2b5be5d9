"""mvhdp_split_topic without a GPU: hand-written known answers of the restatement the device is compared with (tests/native/split_ref.c
through tests/split_ref.py), what every split conserves, the layout of the two structs as include/mvhdp.h states it, the planted case that
shows the conditional is the right one, and the helpers of mvtopicmodel_amd/surgery.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from mvtopicmodel_amd import _lib, surgery
from mvtopicmodel_amd.native import Hyper
from tests import split_cases as sc
from tests import split_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = -1


def i32(*x):
    return np.array(x, dtype=np.int32)


def tiny(alpha_src=0.5, beta=0.25, V=2, K=2):
    """one view, topic 1 free and inactive"""
    hy = Hyper.defaults(K, [V], beta=beta)
    hy.alpha[0, 0] = alpha_src
    hy.alpha[0, 1:K] = 0.0
    hy.alpha_sum[:] = hy.alpha[:, :K].sum(1)
    hy.inactive = np.zeros(K, dtype=np.uint8)
    hy.inactive[1:] = 1
    return hy


# ---- the restatement: known answers ------------------------------------------------------------------------------------------------------
def test_one_entity_two_tokens_one_iteration_by_hand():
    hy = tiny()                                              # alpha 0.5: ah = 0.25, A = gamma * ah = 0.25; beta 0.25, betaSum 0.5
    off, tok, z = [np.array([0, 2])], [i32(0, 1)], [i32(0, 0)]
    seed, g = 12345, 7
    u0 = [sr.unit(g, 0, 0, p, seed) for p in (0, 1)]
    side = [1 if u >= 0.5 else 0 for u in u0]
    r0 = sr.run(2, [2], off, tok, z, hy, 0, 1, iterations=0, seed=seed, doc_id_base=g)
    assert r0.rc == 0 and r0.z[0].tolist() == side and r0.flips.tolist() == [] and r0.flips_last == 0
    # iteration 1 by hand: the counts of the sides are frozen at what iteration 0 left
    cw = np.zeros((2, 2), dtype=np.int64)                    # [type][side]
    for w, s in zip((0, 1), side):
        cw[w, s] += 1
    c = cw.sum(0)
    e = [side.count(0), side.count(1)]
    A, beta, bsum = 0.25, 0.25, 0.5
    want, trace, flips = list(side), [], 0
    for pos, w in enumerate((0, 1)):
        y = want[pos]
        e[y] -= 1
        wt = []
        for x in (0, 1):
            own = 1 if x == y else 0
            r = 1.0 / (float(c[x] - own) + bsum)
            phi = (float(cw[w, x] - own) + beta) * r
            wt.append((1.0 * float(e[x]) + A) * phi)         # one view: base = A + 0.0 * Lp
        total = wt[0] + wt[1]
        u = sr.unit(g, 1, 0, pos, seed)
        s = 0 if u * total < wt[0] else 1
        trace.append((u, wt[0], wt[1], total))
        e[s] += 1
        flips += s != y
        want[pos] = s
    r1 = sr.run(2, [2], off, tok, z, hy, 0, 1, iterations=1, seed=seed, doc_id_base=g, trace=True)
    assert r1.z[0].tolist() == want and r1.flips.tolist() == [flips] and r1.flips_last == flips
    assert r1.trace.tolist() == [list(t) for t in trace]
    assert r1.alpha[0].tolist() == [0.25, 0.25, hy.alpha[0, 2]] and r1.inactive.tolist() == [0, 0]
    assert (r1.target, r1.activated) == (1, 1) and r1.split.tolist() == [2] and r1.moved.tolist() == [sum(want)]
    keep = sr.run(2, [2], off, tok, z, hy, 0, 1, iterations=1, seed=seed, doc_id_base=g, keep_alpha=True)
    assert keep.alpha[0].tolist() == [0.5, 0.25, hy.alpha[0, 2]] and keep.z[0].tolist() == want


def test_the_counter_takes_both_words_of_the_entity_id():
    lo = sr.unit(5, 0, 0, 3, 9)
    assert sr.unit(sc.DOC_ID_BASE, 0, 0, 3, 9) != lo and 0.0 <= lo < 1.0
    assert sr.unit(5, 0, 1, 3, 9) != lo and sr.unit(5, 1, 0, 3, 9) != lo and sr.unit(5, 0, 0, 3, 9 + 2 ** 32) != lo
    hy = tiny(V=3)
    off, tok, z = [np.array([0, 0, 40])], [np.arange(40, dtype=np.int32) % 3], [np.zeros(40, np.int32)]
    a = sr.run(2, [3], off, tok, z, hy, 0, 1, iterations=0, seed=1, doc_id_base=5)
    b = sr.run(2, [3], off, tok, z, hy, 0, 1, iterations=0, seed=1, doc_id_base=sc.DOC_ID_BASE)
    want = [1 if sr.unit(sc.DOC_ID_BASE + 1, 0, 0, p, 1) >= 0.5 else 0 for p in range(40)]    # entity 1 of the shifted base
    assert b.z[0].tolist() == want and a.z[0].tolist() != want


def test_the_hint_overrides_the_coin():
    hy = tiny(V=3)
    n = 60
    off, tok, z = [np.array([0, n])], [np.arange(n, dtype=np.int32) % 3], [np.zeros(n, np.int32)]
    hint = [np.array([0, 1, -1], dtype=np.int8)]
    r = sr.run(2, [3], off, tok, z, hy, 0, 1, iterations=0, seed=3, type_hint=hint)
    coin = sr.run(2, [3], off, tok, z, hy, 0, 1, iterations=0, seed=3)
    assert (r.z[0][tok[0] == 0] == 0).all() and (r.z[0][tok[0] == 1] == 1).all()
    assert np.array_equal(r.z[0][tok[0] == 2], coin.z[0][tok[0] == 2]) and 0 < coin.z[0].sum() < n
    assert not (coin.z[0][tok[0] == 0] == 0).all()
    assert sr.run(2, [3], off, tok, z, hy, 0, 1, type_hint=[np.array([0, 2, -1], dtype=np.int8)]).rc == INV
    assert sr.run(2, [3], off, tok, z, hy, 0, 1, type_hint=[np.array([0, -2, -1], dtype=np.int8)]).rc == INV


def test_a_total_of_zero_keeps_the_side():
    hy = tiny()
    off, tok, z = [np.array([0, 30])], [np.zeros(30, np.int32)], [np.zeros(30, np.int32)]
    start = sr.run(2, [2], off, tok, z, hy, 0, 1, iterations=0, seed=8)
    r = sr.run(2, [2], off, tok, z, hy, 0, 1, iterations=3, seed=8, coupling=np.zeros((1, 1)), trace=True)   # P[m][m] = 0 and alpha = 0 below
    assert r.flips.sum() > 0                                 # (with alpha > 0 the weights are not zero)
    hy0 = tiny(alpha_src=0.0)
    r = sr.run(2, [2], off, tok, z, hy0, 0, 1, iterations=3, seed=8, coupling=np.zeros((1, 1)), trace=True)
    assert (r.trace[:, 3] == 0.0).all() and len(r.trace) == 90
    assert np.array_equal(r.z[0], start.z[0]) and r.flips.tolist() == [0, 0, 0]


def test_refusals_of_the_arguments_and_the_target():
    hy = tiny(K=4)
    off, tok, z = [np.array([0, 3])], [i32(0, 1, 0)], [i32(0, 0, 2)]
    run = lambda **kw: sr.run(4, [2], off, tok, z, hy, **kw).rc
    assert run(source=0, target=1) == 0
    assert run(source=0) == 0 and sr.run(4, [2], off, tok, z, hy, 0).target == 1          # the lowest free index of the inactive set
    assert run(source=0, target=0) == INV and run(source=4, target=1) == INV and run(source=-1, target=1) == INV
    assert run(source=0, target=4) == INV and run(source=0, target=-2) == INV
    assert run(source=1, target=3) == INV                    # the source is inactive
    assert run(source=0, target=2) == INV                    # the target holds a token
    assert run(source=0, target=1, iterations=65536) == INV and run(source=0, target=1, iterations=-1) == INV
    assert run(source=0, target=1, iterations=65535 * 0) == 0 and run(source=0, target=1, flags=2) == INV
    assert run(source=0, target=1, coupling=np.array([[-1.0]])) == INV and run(source=0, target=1, coupling=np.array([[np.nan]])) == INV
    hy.alpha[0, 1] = 0.125                                   # alpha of the target is not 0.0
    assert run(source=0, target=1) == INV and sr.run(4, [2], off, tok, z, hy, 0).target == 3
    hy.inactive[:] = 0
    assert run(source=0) == INV                              # nothing to pick
    assert run(source=0, target=3) == 0                      # an active free index may be named
    assert sr.run(4, [2], off, tok, z, hy, 0, 3).activated == 0
    empty = sr.run(4, [2], off, tok, [i32(2, 2, 2)], hy, 0, 3, iterations=2)              # a source without tokens
    assert empty.rc == 0 and empty.split.tolist() == [0] and empty.flips.tolist() == [0, 0] and empty.alpha[0, :4].tolist() == [0.25, 0.125, 0.0, 0.25]


# ---- what every split conserves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", sc.M_VALUES)
@pytest.mark.parametrize("K", sc.K_VALUES)
def test_the_set_is_conserved_and_the_rest_untouched(K, M):
    c = sc.make(K, M)
    r = sr.run(K, c.V, c.doc_off, c.tokens, c.z, c.hy, c.source, iterations=3, seed=5, type_hint=sc.hints(c), coupling=sc.coupling(M),
               doc_id_base=sc.DOC_ID_BASE)
    assert r.rc == 0 and r.target == c.free[0] and r.activated == 1
    for m in range(M):
        on = c.z[m] == c.source
        assert np.array_equal(r.z[m][~on], c.z[m][~on])                                     # every other position untouched
        assert np.isin(r.z[m][on], [c.source, r.target]).all()
        assert not (c.z[m] == r.target).any()
        ends = c.doc_off[m]
        for d in range(c.D):                                                                # per entity and view
            a, b = ends[d], ends[d + 1]
            assert np.isin(r.z[m][a:b], [c.source, r.target]).sum() == (c.z[m][a:b] == c.source).sum()
        assert r.split[m] == on.sum() and r.moved[m] == (r.z[m] == r.target).sum()
    assert 0 < r.moved.sum() < r.split.sum() and len(r.flips) == 3 and r.flips_last == r.flips[-1]
    again = sr.run(K, c.V, c.doc_off, c.tokens, c.z, c.hy, c.source, iterations=3, seed=5, type_hint=sc.hints(c), coupling=sc.coupling(M),
                   doc_id_base=sc.DOC_ID_BASE)
    assert all(np.array_equal(x, y) for x, y in zip(r.z, again.z)) and again.alpha.tobytes() == r.alpha.tobytes()
    # the halves add up to the whole, bit for bit
    a0 = np.asarray(c.hy.alpha)[:, c.source]
    assert ((0.5 * a0) + (0.5 * a0)).tobytes() == a0.tobytes()
    assert r.alpha[:, c.source].tobytes() == (0.5 * a0).tobytes() == r.alpha[:, r.target].tobytes()
    rest = [k for k in range(K + 1) if k not in (c.source, r.target)]
    assert r.alpha[:, rest].tobytes() == np.asarray(c.hy.alpha)[:, rest].tobytes()
    assert r.inactive.tolist() == [0 if k == r.target else int(v) for k, v in enumerate(c.hy.inactive)]


@pytest.mark.parametrize("M", sc.M_VALUES)
@pytest.mark.parametrize("K", sc.K_VALUES)
def test_cases_hold_what_the_device_tests_rely_on(K, M):
    c = sc.make(K, M)
    assert c.D == (204 if M > 1 else 203) and all(len(o) == c.D + 1 for o in c.doc_off) and sc.handle_doc_id_base(c) + c.D < 2 ** 29
    span = lambda m, d: slice(int(c.doc_off[m][d]), int(c.doc_off[m][d + 1]))
    sp = c.special
    assert (c.z[0][span(0, sp["all65"])] == c.source).sum() == 65 == len(c.z[0][span(0, sp["all65"])])
    assert (c.z[0][span(0, sp["long1500"])] == c.source).sum() == 1500
    if M > 1:
        d = sp["side_only"]
        assert len(c.z[0][span(0, d)]) == 0 and (c.z[M - 1][span(M - 1, d)] == c.source).sum() == 7
    if M == 3:
        assert all((c.z[m][span(m, sp["all_views"])] == c.source).sum() > 0 for m in range(3))
    rare = c.tokens[0] == c.V[0] - 1
    assert rare.any() and (c.z[0][rare] == c.source).all()
    for m in range(M):
        assert len(c.tokens[m]) > 0 and not np.isin(c.z[m], c.free).any() and c.tokens[m].max() < c.V[m]
    assert len(c.free) >= 1 and (np.asarray(c.hy.alpha)[:, c.free] == 0.0).all() and not c.hy.inactive[c.source]
    assert np.array_equal(surgery.free_topics(sum(sr.counts_of(K, c.V[m], c.tokens[m], c.z[m])[1].astype(np.int64) for m in range(M)),
                                              c.hy.inactive, c.hy.alpha), c.free)


# ---- the ABI's structs and flag ----------------------------------------------------------------------------------------------------------
def test_struct_layouts_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "mvhdp.h")).read()
    assert int(re.search(r"#define\s+MVHDP_SPLIT_KEEP_ALPHA\s+(0x[0-9a-fA-F]+)u", hdr).group(1), 16) == _lib.SPLIT_KEEP_ALPHA == sr.KEEP_ALPHA == 1
    assert "uint32 flags; uint64 seed; two host pointers (40 bytes)" in hdr and "double kernel_ms (152 bytes)" in hdr
    A, S = _lib.SplitArgsC, _lib.SplitStatsC
    assert C.sizeof(A) == 40
    assert (A.source.offset, A.target.offset, A.iterations.offset, A.flags.offset, A.seed.offset, A.coupling.offset, A.type_hint.offset) == (0, 4, 8, 12, 16, 24, 32)
    assert C.sizeof(S) == 152
    assert (S.split.offset, S.moved.offset, S.flips_last.offset, S.target.offset, S.activated.offset, S.kernel_ms.offset) == (0, 64, 128, 136, 140, 144)
    assert struct.calcsize("iiIIQPP") == 40 and struct.calcsize("8q8qqiid") == 152
    assert "mvhdp_split_topic" in _lib.ABI_SYMBOLS
    assert "mvhdp_split.hip" in open(os.path.join(ROOT, "mvtopicmodel_amd", "csrc", "mvhdp_state.h")).read().split("#pragma once")[0]


# ---- the planted case: the conditional is the right one ----------------------------------------------------------------------------------
def test_a_planted_split_is_found():
    c = sc.planted(hinted=True)
    r = sr.run(c.K, c.V, c.doc_off, c.tokens, c.z, c.hy, c.source, iterations=20, seed=2, type_hint=c.hint)
    assert r.rc == 0 and r.target == c.K - 1
    p = sc.purity(c, r.z, r.target)
    assert p >= 0.9, (p, r.flips.tolist())
    assert r.flips[-1] < r.flips[0]


# ---- surgery.py --------------------------------------------------------------------------------------------------------------------------
def test_free_topics_and_hint_from_words():
    alpha = np.array([[0.5, 0.0, 0.0, 0.0, 0.0, 9.0], [0.5, 0.0, 0.0, 0.25, 0.0, 9.0]])      # [M][K + 1]
    got = surgery.free_topics([7, 0, 3, 0, 0], [0, 1, 1, 1, 0], alpha)
    assert got.tolist() == [1] and got.dtype == np.int32     # 2 holds tokens, 3 has alpha in a view, 4 is active
    assert surgery.free_topics([7, 0, 3, 0, 0], [0, 1, 1, 1, 1], alpha[:, :5]).tolist() == [1, 4]
    assert surgery.free_topics([1, 1], [0, 0], np.zeros((1, 3))).tolist() == []
    with pytest.raises(ValueError):
        surgery.free_topics([1, 1, 1], [0, 0], np.zeros((1, 3)))
    row = surgery.hint_from_words(6, stay=[0, 4], go=[5])
    assert row.dtype == np.int8 and row.tolist() == [0, -1, -1, -1, 0, 1]
    assert surgery.hint_from_words(3).tolist() == [-1, -1, -1]
    with pytest.raises(ValueError):
        surgery.hint_from_words(3, stay=[1], go=[1])
    with pytest.raises(ValueError):
        surgery.hint_from_words(3, go=[3])
