"""mvhdp_remap_topics without a GPU: hand-written known answers of the restatement the device is compared with (tests/remap_numpy.py), the
layout of the two structs as include/mvhdp.h states it, the case builder's promises, and the map builders of mvtopicmodel_amd/surgery.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from mvtopicmodel_amd import _lib, surgery
from tests import remap_cases as rc
from tests import remap_numpy as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def i32(*x):
    return np.array(x, dtype=np.int32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_the_chain_is_not_chased():
    z = [i32(0, 1, 2, -1, 0, 1)]
    alpha = np.array([[0.5, 0.25, 0.125, 9.0]])
    r = rn.remap(3, z, alpha, np.zeros(3, np.uint8), [1, 2, 2])
    assert r.z[0].tolist() == [1, 2, 2, -1, 1, 2]           # topic 0's tokens stop at 1
    assert r.moved.tolist() == [4] and r.dropped.tolist() == [0]
    assert r.alpha.tolist() == [[0.0, 0.5, 0.375, 9.0]]     # alpha[m][K] stays
    assert r.inactive.tolist() == [0, 0, 0] and (r.vacated, r.retired) == (1, 0)
    assert rn.remap(3, z, alpha, np.zeros(3, np.uint8), [1, 2, 2], rn.RETIRE).inactive.tolist() == [1, 0, 0]
    assert rn.remap(3, z, alpha, np.zeros(3, np.uint8), [1, 2, 2], rn.RETIRE).retired == 1


def test_merge_drop_and_move_in_two_views():
    z = [i32(0, 1, 2, 3, 3, -1), i32(2, 2, 1)]
    alpha = np.array([[1.0, 2.0, 3.0, 4.0, 7.0], [0.1, 0.2, 0.3, 0.4, 7.0]])
    inactive = np.array([0, 0, 0, 0], np.uint8)
    r = rn.remap(4, z, alpha, inactive, [0, 0, -1, 1])       # 1 joins 0, 2 is dropped, 3 moves onto the emptied 1
    assert r.z[0].tolist() == [0, 0, -1, 1, 1, -1] and r.z[1].tolist() == [-1, -1, 0]
    assert r.moved.tolist() == [3, 1] and r.dropped.tolist() == [1, 2]
    assert r.alpha.tolist() == [[3.0, 4.0, 0.0, 0.0, 7.0], [0.1 + 0.2, 0.4, 0.0, 0.0, 7.0]]
    assert r.inactive.tolist() == [0, 0, 0, 0] and (r.vacated, r.retired) == (2, 0)
    r = rn.remap(4, z, alpha, inactive, [0, 0, -1, 1], rn.RETIRE)
    assert r.inactive.tolist() == [0, 0, 1, 1] and (r.vacated, r.retired) == (2, 2)
    nwk, nk = rn.counts_of(4, 3, i32(0, 0, 1, 2, 2, 1), r.z[0])
    assert nk.tolist() == [2, 2, 0, 0] and nwk.tolist() == [[2, 0, 0, 0], [0, 0, 0, 0], [0, 2, 0, 0]]


def test_alpha_sums_run_in_ascending_k_and_one_source_moves_its_bits():
    a = [1e16, 1.0, -1e16, 1.0]                              # ((1e16 + 1) - 1e16) + 1 = 1, any other order gives 0 or 2
    assert ((a[0] + a[1]) + a[2]) + a[3] == 1.0 and (a[0] + a[2]) + (a[1] + a[3]) == 2.0
    alpha = np.array([a + [0.5]])
    r = rn.remap(4, [i32()], alpha, np.zeros(4, np.uint8), [2, 2, 2, 2])
    assert r.alpha.tolist() == [[0.0, 0.0, 1.0, 0.0, 0.5]]
    odd = np.array([[-0.0, 5e-324, 0.1 + 0.2, 1.0]])         # a permutation carries every bit pattern, minus zero and a denormal included
    r = rn.remap(3, [i32()], odd, np.zeros(3, np.uint8), [2, 0, 1])
    assert bits(r.alpha) == bits(odd[:, [1, 2, 0, 3]])
    assert np.signbit(r.alpha[0, 2]) and not np.signbit(rn.remap(3, [i32()], odd, np.zeros(3, np.uint8), [1, 1, 1]).alpha[0, 0])   # no source: +0.0


def test_inactive_iff_every_source_was_and_vacated_counts_what_was_in_use():
    inactive = np.array([0, 1, 1, 1, 0], np.uint8)
    alpha = np.ones((1, 6))
    z = [i32(0, 0, 4, 3)]                                    # the inactive topic 3 holds a token all the same
    r = rn.remap(5, z, alpha, inactive, [0, 0, 1, 1, 2])     # 1 joins the active 0; 2 and 3 (both inactive) make the new 1; 4 moves to 2
    assert r.inactive.tolist() == [0, 1, 0, 1, 0]            # 3 keeps its state, 4 stays "active" with alpha 0
    assert (r.vacated, r.retired) == (2, 1)                  # 3 (held a token; inactive as before) and 4 (was active)
    assert r.alpha[0, :5].tolist() == [2.0, 2.0, 1.0, 0.0, 0.0]
    r = rn.remap(5, z, alpha, inactive, [0, 0, 1, 1, 2], rn.RETIRE)
    assert r.inactive.tolist() == [0, 1, 0, 1, 1] and (r.vacated, r.retired) == (2, 2)
    r = rn.remap(5, [i32(0, 0, 4)], alpha, inactive, [0, 0, 1, 1, 2])
    assert (r.vacated, r.retired) == (1, 0)                  # an unused inactive index that nothing maps onto is not vacated


def test_everything_dropped_and_the_identity():
    z = [i32(0, 1, -1, 1)]
    alpha = np.array([[0.5, 0.25, 1.0]])
    r = rn.remap(2, z, alpha, np.zeros(2, np.uint8), [-1, -1])
    assert r.z[0].tolist() == [-1] * 4 and r.dropped.tolist() == [3] and r.moved.tolist() == [0] and r.vacated == 2
    assert r.alpha.tolist() == [[0.0, 0.0, 1.0]]
    r = rn.remap(2, z, alpha, np.array([0, 1], np.uint8), [0, 1])
    assert r.z[0].tolist() == z[0].tolist() and bits(r.alpha) == bits(alpha) and r.inactive.tolist() == [0, 1]
    assert (r.moved.sum(), r.dropped.sum(), r.vacated, r.retired) == (0, 0, 0, 0)


# ---- the ABI's structs and flag ------------------------------------------------------------------------------------------------------------
def test_struct_layouts_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "mvhdp.h")).read()
    assert int(re.search(r"#define\s+MVHDP_REMAP_RETIRE\s+(0x[0-9a-fA-F]+)u", hdr).group(1), 16) == _lib.REMAP_RETIRE == rn.RETIRE == 1
    assert "mvhdp_remap_args: a pointer and a uint32 (16 bytes)" in hdr and "kernel_ms (144 bytes)" in hdr
    A, S = _lib.RemapArgsC, _lib.RemapStatsC
    assert C.sizeof(A) == 16 and (A.map.offset, A.flags.offset) == (0, 8)
    assert C.sizeof(S) == 144 and (S.moved.offset, S.dropped.offset, S.vacated.offset, S.retired.offset, S.kernel_ms.offset) == (0, 64, 128, 132, 136)
    assert struct.calcsize("8q8qiid") == 144
    assert "mvhdp_remap_topics" in _lib.ABI_SYMBOLS and "mvhdp_group_remap_topics" in _lib.ABI_SYMBOLS


# ---- the case builder keeps its promises ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", rc.M_VALUES)
@pytest.mark.parametrize("K", rc.K_VALUES)
def test_cases_hold_what_the_device_tests_rely_on(K, M):
    c = rc.make(K, M)
    lens0 = np.diff(c.doc_off[0])
    assert set(rc.SPANS) <= set(lens0.tolist())
    total = sum(len(t) for t in c.tokens)
    assert 1000 < total < 6000 and c.D == 200
    empty = [m for m in range(M) if len(c.tokens[m]) == 0]
    assert empty == ([1] if (M == 3 and K % 2 == 0) else [])
    for m in range(M):
        if m not in empty:
            assert len(c.tokens[m]) % 4 == 1 + m % 3         # a tail of every length over the views
            assert (c.z[m] == -1).sum() == 5
        assert c.z[m].max(initial=-1) < K and c.tokens[m].max(initial=0) < c.V[m]
        assert not c.hy.inactive[c.z[m][c.z[m] >= 0]].any()  # inactive topics hold nothing
    assert int(c.hy.inactive.sum()) == (0 if K < 3 else 1 if K < 63 else 2)
    assert len(np.unique(c.hy.alpha[:, :K][:, c.hy.inactive == 0])) == M * int((c.hy.inactive == 0).sum())
    mp = rc.maps(K)
    assert {"identity", "cycle", "reversal", "onto_one", "drop_all"} <= set(mp)
    assert ("across_lanes" in mp) == (K >= 65) and ("chain" in mp) == (K >= 3) and ("mixed" in mp) == (K >= 8)
    for name, t in mp.items():
        assert t.dtype == np.int32 and t.shape == (K,) and t.min() >= -1 and t.max() < K, name
    if K >= 3:
        assert mp["chain"][:3].tolist() == [1, 2, 2] and sorted(mp["cycle"].tolist()) == list(range(K))
    if K >= 65:
        assert mp["across_lanes"][[0, 1, 63, 64]].tolist() == [64] * 4


def test_a_split_case_concatenates_to_the_whole():
    c = rc.make(65, 3, inactive=False)
    a, b = rc.split(c, 77)
    for m in range(c.M):
        assert np.array_equal(np.concatenate([a.z[m], b.z[m]]), c.z[m]) and np.array_equal(np.concatenate([a.tokens[m], b.tokens[m]]), c.tokens[m])
        assert a.doc_off[m][0] == 0 and b.doc_off[m][0] == 0 and a.doc_off[m][-1] + b.doc_off[m][-1] == c.doc_off[m][-1]
    assert (a.base, b.base, a.D + b.D) == (0, 77, c.D)


# ---- surgery.py ----------------------------------------------------------------------------------------------------------------------------
def test_merge_map_on_a_chain_and_a_tie():
    sim = np.zeros((5, 5))
    sim[0, 1] = sim[1, 0] = 0.9                              # 0 - 1 - 2 is a chain: 0 and 2 are not similar themselves
    sim[2, 1] = 0.8                                          # (one triangle is enough)
    sim[3, 4] = 0.7                                          # exactly the threshold: not merged
    np.fill_diagonal(sim, 1.0)                               # the diagonal merges nothing
    assert surgery.merge_map(sim, 0.7, [5, 9, 9, 1, 2]).tolist() == [1, 1, 1, 3, 4]        # 1 and 2 tie at 9: the lower id
    assert surgery.merge_map(sim, 0.7, [5, 1, 9, 1, 2]).tolist() == [2, 2, 2, 3, 4]
    assert surgery.merge_map(sim, 0.69, [5, 9, 9, 2, 2]).tolist() == [1, 1, 1, 3, 3]
    assert surgery.merge_map(sim, 1.0, [1, 1, 1, 1, 1]).tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        surgery.merge_map(sim[:4], 0.5, [1, 1, 1, 1, 1])


def test_prune_map_and_order_map():
    assert surgery.prune_map([10, 0, 3, 2], 3).tolist() == [0, -1, 2, -1]
    assert surgery.prune_map([10, 0, 3, 2], 0).tolist() == [0, 1, 2, 3]
    m = surgery.order_map([3, 7, 7, 0, 9], inactive=[0, 0, 0, 1, 1])
    assert m.tolist() == [2, 0, 1, 3, 4]                     # 1 and 2 tie: by id; the inactive 3 and 4 last in id order, whatever they weigh
    assert surgery.order_map([1, 2, 3]).tolist() == [2, 1, 0] and surgery.order_map([1, 2, 3]).dtype == np.int32
    rng = np.random.default_rng(5)
    for K in (1, 2, 64, 257):
        w = rng.integers(0, 6, K)
        off = rng.random(K) < 0.2
        m = surgery.order_map(w, off)
        assert sorted(m.tolist()) == list(range(K))          # a permutation
        new_w, new_off = np.empty(K, np.int64), np.empty(K, bool)
        new_w[m], new_off[m] = w, off
        n_on = int((~off).sum())
        assert not new_off[:n_on].any() and new_off[n_on:].all() and (np.diff(new_w[:n_on]) <= 0).all()


def test_compose_once_is_first_then_then():
    rng = np.random.default_rng(11)
    for K in (3, 65, 300):
        c = rc.make(K, 1, seed=K)
        a = rng.integers(-1, K, K).astype(np.int32)
        b = rng.integers(-1, K, K).astype(np.int32)
        alpha, off = np.array(c.hy.alpha), np.array(c.hy.inactive)
        one = rn.remap(K, c.z, alpha, off, a)
        two = rn.remap(K, one.z, alpha, off, b)
        both = rn.remap(K, c.z, alpha, off, surgery.compose(a, b))
        assert np.array_equal(both.z[0], two.z[0]) and (both.z[0] != c.z[0]).any()
    assert surgery.compose([1, 2, 2], [1, 2, 2]).tolist() == [2, 2, 2]                      # the chain, chased by hand
    assert surgery.compose([-1, 0], [1, 1]).tolist() == [-1, 1] and surgery.identity_map(3).tolist() == [0, 1, 2]
