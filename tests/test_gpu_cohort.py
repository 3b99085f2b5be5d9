"""mvhdp_cohort_top_words on a device against the literal restatement of its contract (tests/cohort_numpy.py): every output is an integer
and every integer is compared.  Corpora of a few thousand tokens (tests/cohort_cases.py) at the shapes where the device code takes
another path: K and V_m around the 64 lanes of a wave and the four-wave split of the selection, spans of 0, 1, 64, 65 and 700 tokens,
empty, single, repeated and overlapping cohorts, passes of one, two and all cohorts."""
import ctypes as C
from functools import cmp_to_key

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_NO_APPLY
from tests import cohort_cases as cc
from tests import cohort_numpy as cn
from tests.helpers import INV, STATE, load, untouched

pytestmark = pytest.mark.gpu
ONE, TWO, AUTO = "one table", "two tables", "auto"
# (order, n, min_count, scratch): every n, min_count and scratch size with either order
VARIANTS = [("count", 20, 1, AUTO), ("count", 1, 2, ONE), ("count", 64, 1, TWO), ("count", 20, 5, TWO),
            ("share", 20, 1, TWO), ("share", 64, 2, ONE), ("share", 1, 5, AUTO), ("share", 20, 2, AUTO)]


def scratch_of(c, m, which):
    return {ONE: 1, TWO: 2 * cc.table_bytes(c, m), AUTO: 0}[which]


def assert_equal(got, want, what):
    """got: a CohortWords; want: (types, counts, nonzero, tokens, docs) of the restatement"""
    for name, w in zip(("types", "counts", "nonzero", "tokens", "docs"), want):
        g = getattr(got, name)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:6])


def as_bytes(r):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (r.types, r.counts, r.nonzero, r.tokens, r.docs) if a is not None)


def check_view(s, c, m, z=None, variants=VARIANTS, what=None):
    """every variant of view m against the restatement; the counting is restated once and shared"""
    z = c.z[m] if z is None else z
    co = cc.cohorts(c)
    G = len(co)
    cd = cn.count(c.K, c.V[m], c.doc_off[m], c.tokens[m], z, co)
    nwk = s.get_counts(m)[0].astype(np.int64) if any(v[0] == "share" for v in variants) else None
    seen = dict(padding=False, tie=False)
    for order, n, min_count, scratch in variants:
        types, counts = cn.select(cd, n, order, min_count, nwk)
        got = s.cohort_top_words(m, co, n=n, order=order, min_count=min_count, scratch_bytes=scratch_of(c, m, scratch))
        assert_equal(got, (types, counts, cd.nonzero, cd.tokens, cd.docs), (what, c.K, c.V[m], m, order, n, min_count, scratch))
        st = got.stats
        per = {ONE: 1, TWO: 2, AUTO: G}[scratch]
        assert (st.listings, st.tokens, st.skipped) == (sum(len(x) for x in co), cd.counted, cd.skipped), (what, st)
        assert (st.passes, st.cohorts_per_pass) == ((G + per - 1) // per, per), (what, scratch, st)
        seen["padding"] |= bool((types[cd.tokens > 0] == -1).any())
        if order == "count":
            more = cn.select(cd, n + 1, order, min_count)[1]
            seen["tie"] |= bool(((more[:, :, n] > 0) & (more[:, :, n] == more[:, :, n - 1])).any())
    return cd, seen


@pytest.mark.parametrize("V", cc.V_VALUES)
@pytest.mark.parametrize("K", cc.K_VALUES)
def test_every_shape_equals_the_restatement(K, V):
    other = cc.V_VALUES[(cc.V_VALUES.index(V) + 1) % len(cc.V_VALUES)]
    c = cc.make(K, [V, other, 5])
    for m in (0, 1):
        assert set(cc.SPANS) <= set(np.diff(c.doc_off[m]).tolist())
    co = cc.cohorts(c)
    assert len(co) % 2 == 1 and [] in co and any(len(x) == 1 for x in co) and any(len(x) == 3 and len(set(x)) == 1 for x in co)
    with load(c) as s:
        for m in (0, 1):
            cd, seen = check_view(s, c, m)
            assert cd.skipped > 0 and seen["padding"]                        # the holes are listed; some list is shorter than n
            if c.V[m] > 1:
                assert seen["tie"], "no equal counts across the n-th place: reseed"
            # the trends-only call: the same tokens and docs, no lists, one pass whatever the scratch
            t = s.cohort_top_words(m, co, trends_only=True, scratch_bytes=1)
            assert t.types is None and t.counts is None and t.nonzero is None
            assert np.array_equal(t.tokens, cd.tokens) and np.array_equal(t.docs, cd.docs) and t.tokens.dtype == np.int64
            assert (t.stats.passes, t.stats.cohorts_per_pass, t.stats.tokens, t.stats.skipped) == (1, len(co), cd.counted, cd.skipped)


def test_the_member_off_form_and_the_host_derivations():
    c = cc.make(5, [65, 64, 5], seed=1)
    co = cc.cohorts(c)
    moff = np.concatenate([[0], np.cumsum([len(x) for x in co])])
    mem = np.concatenate([np.asarray(x, dtype=np.int64) for x in co])
    with load(c) as s:
        a = s.cohort_top_words(0, co, n=5)
        b = s.cohort_top_words(0, (moff, mem), n=5)
        assert as_bytes(a) == as_bytes(b)
        g = 5                                                                # every entity once
        assert np.allclose(a.trend().sum(1)[[g]], 1.0) and a.trend()[0].sum() == 0.0
        words = a.words(g, 0, vocabulary=[f"w{i}" for i in range(c.V[0])])
        assert len(words) == 5 and words[0] == (f"w{a.types[g, 0, 0]}", int(a.counts[g, 0, 0]))
        none = s.cohort_top_words(0, [], n=5)                                # no cohorts: empty arrays
        assert none.types.shape == (0, c.K, 5) and none.tokens.shape == (0, c.K) and none.stats.listings == 0


def test_after_a_deferred_and_after_a_live_sweep():
    c = cc.make(5, [65, 64, 5], seed=2, holes=False)
    some = VARIANTS[:1] + VARIANTS[4:5]
    with load(c) as s:
        s.sweep(0, 99)                                                       # a deferred sweep: z moves, its deltas are applied
        z = [s.get_assignments(m) for m in range(c.M)]
        assert (z[0] != c.z[0]).any()
        for m in (0, 1):
            check_view(s, c, m, z[m], some, "deferred")
        s.sweep(1, 7, flags=SWEEP_LIVE)
        z2 = [s.get_assignments(m) for m in range(c.M)]
        assert (z2[0] != z[0]).any()
        for m in (0, 1):
            check_view(s, c, m, z2[m], some, "live")
        s.sweep(2, 5, flags=SWEEP_NO_APPLY)                                  # its deltas wait: the counts are not those of z
        z3 = s.get_assignments(0)
        check_view(s, c, 0, z3, VARIANTS[:1], "pending")                     # BY_COUNT reads no counts
        with pytest.raises(MvhdpError) as e:
            s.cohort_top_words(0, [[0, 1]], order="share")
        assert e.value.code == STATE and "pending" in str(e.value)
        s.apply_delta()
        check_view(s, c, 0, z3, some, "applied")


def test_the_share_order_needs_64_bit_products():
    """global counts near 2^31 - 1 through mvhdp_set_counts: the shares 2 / 1431655000 > 3 / (2^31 - 1) > 1 / (2^31 - 1001), which the
    counts order otherwise and products wrapped to 32 bits order otherwise again"""
    big = 2 ** 31 - 1
    cells = {7: (3, big), 2: (1, big - 1000), 4: (2, 1431655000)}            # type: (count in the cohort, global count)
    want = [4, 7, 2]
    wrapped = sorted(cells, key=cmp_to_key(lambda a, b: -1 if (cells[a][0] * cells[b][1]) & 0xffffffff > (cells[b][0] * cells[a][1]) & 0xffffffff else 1))
    assert wrapped != want and sorted(cells, key=lambda t: -cells[t][0]) != want
    K, V = 2, 9
    tok = np.array([t for t, (cnt, _) in cells.items() for _ in range(cnt)] + [0], dtype=np.int32)
    z = np.array([1] * (len(tok) - 1) + [0], dtype=np.int32)
    off = np.array([0, len(tok)], dtype=np.int64)
    nwk = np.zeros((V, K), dtype=np.int32)
    nwk[0, 0] = 1
    for t, (_, n_all) in cells.items():
        nwk[t, 1] = n_all
    with NativeSampler(K, [V]) as s:
        s.set_corpus(0, off, tok)
        s.set_assignments(0, z)
        s.set_counts(0, nwk, np.array([1, big], dtype=np.int32))
        got = s.cohort_top_words(0, [[0]], n=3, order="share")
        ref = cn.cohort_top_words(K, V, off, tok, z, [[0]], n=3, order="share", nwk=nwk.astype(np.int64))
        assert_equal(got, ref[:5], "big cells")
        assert got.types[0, 1].tolist() == want and got.counts[0, 1].tolist() == [2, 3, 1]
        assert s.cohort_top_words(0, [[0]], n=3).types[0, 1].tolist() == [7, 4, 2]


def test_the_cohort_of_every_entity_is_top_words_and_the_counts():
    c = cc.make(64, [257, 65, 5], seed=3, holes=False)
    with load(c) as s:
        for m in (0, 1, 2):
            for n in (1, 20, 64):
                got = s.cohort_top_words(m, [list(range(c.D))], n=n)
                t, cnt, nz = s.top_words(m, n)
                assert np.array_equal(got.types[0], t) and np.array_equal(got.counts[0], cnt) and np.array_equal(got.nonzero[0], nz), (m, n)
            nwk, nk = s.get_counts(m)
            assert np.array_equal(got.tokens[0], nk) and got.stats.skipped == 0
            share = s.cohort_top_words(m, [list(range(c.D))], n=20, order="share")       # every share is 1: the order of the counts
            assert np.array_equal(share.types[0], s.top_words(m, 20)[0])


def test_the_guarantees():
    c = cc.make(65, [257, 64, 5], seed=4)
    co = cc.cohorts(c)
    with load(c) as s:
        s.build_trees()
        z = [s.get_assignments(v) for v in range(c.M)]
        counts = [s.get_counts(v) for v in range(c.M)]
        trees, written, tuning = s.trees_current(), s.counts_written(), bytes(s.get_tuning())
        trees = s.trees_current()                                            # (what counts_written itself left)
        for order in ("count", "share"):
            one = s.cohort_top_words(0, co, n=20, order=order, min_count=2)
            for scratch in (0, 1, 2 * cc.table_bytes(c, 0), 10 ** 12):
                assert as_bytes(one) == as_bytes(s.cohort_top_words(0, co, n=20, order=order, min_count=2, scratch_bytes=scratch)), (order, scratch)
            for g in (2, 4, 6):                                              # a cohort alone, and among the others in another place
                alone = s.cohort_top_words(0, [co[g]], n=20, order=order, min_count=2)
                among = s.cohort_top_words(0, [co[5], co[g], co[0]], n=20, order=order, min_count=2, scratch_bytes=1)
                for name in ("types", "counts", "nonzero", "tokens", "docs"):
                    assert np.array_equal(getattr(alone, name)[0], getattr(one, name)[g]) and np.array_equal(getattr(among, name)[1], getattr(one, name)[g]), (order, g, name)
        for v in range(c.M):
            nwk, nk = s.get_counts(v)
            assert np.array_equal(nwk, counts[v][0]) and np.array_equal(nk, counts[v][1]) and np.array_equal(z[v], s.get_assignments(v))
        assert s.trees_current() == trees and s.counts_written() == written and bytes(s.get_tuning()) == tuning


# ---- the error paths: every output pre-filled and found untouched ----
def raw_call(s, args, G, moff, mem, n=3, skip=(), sentinel=-7):
    K = s.K
    arr = dict(types=np.full((max(G, 1), K, n), sentinel, np.int32), counts=np.full((max(G, 1), K, n), sentinel, np.int32),
               nonzero=np.full((max(G, 1), K), sentinel, np.int32), tokens=np.full((max(G, 1), K), sentinel, np.int64), docs=np.full((max(G, 1), K), sentinel, np.int64))
    st = _lib.CohortStatsC(sentinel, sentinel, sentinel, sentinel, sentinel, float(sentinel))
    ptr = [None if k in skip else arr[k].ctypes.data for k in ("types", "counts", "nonzero", "tokens", "docs")]
    rc = s.L.mvhdp_cohort_top_words(s.h, None if args is None else C.byref(args), G, None if moff is None else moff.ctypes.data,
                                    None if mem is None else mem.ctypes.data, *ptr, C.byref(st))
    clean = untouched(arr, sentinel) and (st.listings, st.passes, st.kernel_ms) == (sentinel, sentinel, float(sentinel))
    return rc, clean


def i64(*x):
    return np.array(x, dtype=np.int64)


def test_error_paths_leave_the_outputs_alone():
    c = cc.make(5, [65, 64, 5], seed=5, holes=False)
    A = _lib.CohortArgsC
    good = A(0, 3, 0, 1, 0)
    with load(c) as s:
        D = c.D
        bad = [
            (None, 1, i64(0, 1), i64(0), ()),                                # NULL args
            (good, 1, None, i64(0), ()),                                     # NULL member_off
            (good, -1, i64(0), i64(0), ()),                                  # negative n_cohorts
            (A(-1, 3, 0, 1, 0), 1, i64(0, 1), i64(0), ()), (A(3, 3, 0, 1, 0), 1, i64(0, 1), i64(0), ()),          # m
            (A(0, 0, 0, 1, 0), 1, i64(0, 1), i64(0), ()), (A(0, 65, 0, 1, 0), 1, i64(0, 1), i64(0), ()),          # n
            (A(0, 3, 2, 1, 0), 1, i64(0, 1), i64(0), ()), (A(0, 3, -1, 1, 0), 1, i64(0, 1), i64(0), ()),          # order
            (A(0, 3, 0, 0, 0), 1, i64(0, 1), i64(0), ()), (A(0, 3, 0, 1, -1), 1, i64(0, 1), i64(0), ()),          # min_count, scratch_bytes
            (good, 1, i64(0, 1), i64(0), ("types",)), (good, 1, i64(0, 1), i64(0), ("counts",)),                    # one of the pair
            (good, 1, i64(1, 1), i64(0), ()), (good, 2, i64(0, 2, 1), i64(0, 1), ()),                               # member_off
            (good, 1, i64(0, 1), i64(D), ()), (good, 1, i64(0, 2), i64(0, -1), ()), (good, 1, i64(0, 1), None, ()),  # members
        ]
        for k, (args, G, moff, mem, skip) in enumerate(bad):
            rc, clean = raw_call(s, args, G, moff, mem, skip=skip)
            assert rc == INV and clean, (k, rc, clean)
            assert len(s.L.mvhdp_last_error(s.h)) > 10
        # the listings of one cohort may hold 2^31 - 1 tokens of the view: one entity of 700 tokens, listed often enough, is refused on the host
        d = int(np.argmax(np.diff(c.doc_off[0])))
        times = (2 ** 31 - 1) // 700 + 1
        rc, clean = raw_call(s, good, 2, i64(0, 1, 1 + times), np.concatenate([[0], np.full(times, d)]).astype(np.int64))
        assert rc == INV and clean and b"2^31" in s.L.mvhdp_last_error(s.h)
        # no cohorts: nothing to write, and the statistics are zero
        assert raw_call(s, good, 0, i64(0), None)[0] == 0
        # BY_SHARE on counts that are not those of z
        share = A(0, 3, 1, 1, 0)
        assert raw_call(s, share, 1, i64(0, 1), i64(0))[0] == 0
        s.set_assignments(0, c.z[0])                                         # assignments replaced: the counts are stale until recounted
        rc, clean = raw_call(s, share, 1, i64(0, 1), i64(0))
        assert rc == STATE and clean and b"current counts" in s.L.mvhdp_last_error(s.h)
        assert raw_call(s, good, 1, i64(0, 1), i64(0))[0] == 0               # BY_COUNT goes on
        s.build_counts()
        assert raw_call(s, share, 1, i64(0, 1), i64(0))[0] == 0
        # a negative type is refused where it is listed, with either set of outputs, and nowhere else
        t = c.tokens[0].copy()
        d0 = int(np.flatnonzero(np.diff(c.doc_off[0]) > 2)[0])
        t[c.doc_off[0][d0] + 1] = -1
        s.set_corpus(0, c.doc_off[0], t)
        s.set_assignments(0, c.z[0])
        other = i64((d0 + 1) % D)
        for skip in ((), ("types", "counts", "nonzero")):
            rc, clean = raw_call(s, good, 2, i64(0, 1, 2), np.concatenate([other, i64(d0)]), skip=skip)
            assert rc == STATE and clean and b"negative type" in s.L.mvhdp_last_error(s.h)
            assert raw_call(s, good, 2, i64(0, 1, 2), np.concatenate([other, other]), skip=skip)[0] == 0
        with pytest.raises(MvhdpError) as e:
            s.cohort_top_words(0, [[d0]])
        assert e.value.code == STATE
    with NativeSampler(3, [4, 5]) as fresh:                                  # no corpus of the view; no counts
        rc, clean = raw_call(fresh, A(1, 3, 0, 1, 0), 0, i64(0), None)
        assert rc == STATE and clean
        fresh.set_corpus(1, np.array([0, 2], np.int64), np.array([1, 1], np.int32))
        fresh.set_assignments(1, np.array([0, 2], np.int32))
        got = fresh.cohort_top_words(1, [[0, 0]], n=2)                       # BY_COUNT needs view m's corpus and nothing else
        assert got.tokens.tolist() == [[2, 0, 2]] and got.docs.tolist() == [[2, 0, 2]] and got.types[0, 0].tolist() == [1, -1]
        with pytest.raises(MvhdpError) as e:
            fresh.cohort_top_words(1, [[0]], order="share")
        assert e.value.code == STATE
        with pytest.raises(ValueError):
            fresh.cohort_top_words(1, [[0]], order="ratio")
