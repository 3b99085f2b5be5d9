"""mvhdp_remap_topics on a device against the literal restatement of its contract (tests/remap_numpy.py): every integer and every bit of
alpha.  The corpora (tests/remap_cases.py) hold a few thousand tokens at the shapes where the device code takes another path.  The
chain tests show that nothing derived from the old topics survives the call: a handle that was remapped and a fresh handle loaded with
the restatement's result go on sweeping alike, integer for integer."""
import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeGroup, NativeSampler, surgery
from mvtopicmodel_amd.native import (SWEEP_ASYNC_EXCHANGE, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY, SWEEP_SEGMENT_APPLY, SWEEP_SEGMENT_OVERLAP,
                                     EmbConfig)
from tests import remap_cases as rc
from tests import remap_numpy as rn
from tests.helpers import INV, STATE, UNSUPPORTED, assert_holds, assert_same_handles, hyper_with, load, state_of

pytestmark = pytest.mark.gpu


# ---- 1. every integer and bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", rc.M_VALUES)
@pytest.mark.parametrize("K", rc.K_VALUES)
def test_every_integer_and_bit_equals_the_restatement(K, M):
    c = rc.make(K, M)
    alpha0, off0 = np.array(c.hy.alpha), np.array(c.hy.inactive)
    with load(c) as s, load(c) as second:
        for name, tm in rc.maps(K).items():
            for retire in (False, True):
                what = (K, M, name, retire)
                for m in range(M):                                           # the starting state again (the map before moved it)
                    s.set_assignments(m, c.z[m])
                s.set_hyper(c.hy)
                s.build_counts()
                want = rn.remap(K, c.z, alpha0, off0, tm, rn.RETIRE if retire else 0)
                st = s.remap_topics(tm, retire=retire)
                assert_holds(s, c, want, rn.counts_of, what)
                assert np.array_equal(st.moved, want.moved) and np.array_equal(st.dropped, want.dropped), (what, st, want.moved, want.dropped)
                assert (st.vacated, st.retired) == (want.vacated, want.retired) and st.kernel_ms > 0.0, (what, st)
                if not retire:                                               # the counts are those mvhdp_build_counts makes of z'
                    for m in range(M):
                        second.set_assignments(m, want.z[m])
                    second.build_counts()
                    assert_same_handles(s, second, M, what)
        assert want.retired > 0 or K == 1                                    # (the last map vacates something)


# ---- 2. the chain goes on ---------------------------------------------------------------------------------------------------------------
def chain(c, tm, retire, expect_births):
    K, M = c.K, c.M
    sweeps = [(2, 0, "deferred"), (3, SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(4), "segment apply"),
              (4, SWEEP_SEGMENT_APPLY | SWEEP_SEGMENT_OVERLAP | SWEEP_LIVE_SEGMENTS(4), "segment overlap")]
    with load(c) as a:
        a.sweep(0, 17); a.sweep(1, 17)                                       # mirrors, class bytes, slot counts and trees of the OLD topics exist
        z = [a.get_assignments(m) for m in range(M)]
        alpha, off = a.get_alpha()
        want = rn.remap(K, z, alpha, off, tm, rn.RETIRE if retire else 0)
        st = a.remap_topics(tm, retire=retire)
        assert st.dropped.sum() > 0 and st.moved.sum() > 0 and np.array_equal(st.moved, want.moved)
        assert (st.vacated, st.retired) == (want.vacated, want.retired) and (st.retired > 0) == retire
        with load(c, z=want.z, hy=hyper_with(c, want.alpha, want.inactive)) as b:
            assert_same_handles(a, b, M, "before the sweeps")
            births = 0
            for idx, flags, name in sweeps:
                offs = [x.get_alpha()[1] for x in (a, b)]
                assert np.array_equal(offs[0], offs[1])
                if flags & SWEEP_SEGMENT_OVERLAP and offs[0].any():          # not with inactive topics: both refuse alike
                    for x in (a, b):
                        with pytest.raises(MvhdpError) as e:
                            x.sweep(idx, 17, flags=flags)
                        assert e.value.code == UNSUPPORTED
                    continue
                sa, sb = a.sweep(idx, 17, flags=flags), b.sweep(idx, 17, flags=flags)
                assert_same_handles(a, b, M, name)
                assert (sa.tokens, sa.changed, sa.activations, sa.activated_topic) == (sb.tokens, sb.changed, sb.activations, sb.activated_topic), name
                assert a.model_log_likelihood().tobytes() == b.model_log_likelihood().tobytes(), name
                assert a.get_alpha()[0].tobytes() == b.get_alpha()[0].tobytes(), name
                births += sa.activations if "segment" in name else 0
                for m in range(M):
                    assert (a.get_assignments(m) >= 0).all()
            assert (births > 0) == expect_births


@pytest.mark.parametrize("K", [65, 257])
def test_the_chain_goes_on_as_on_a_fresh_handle(K):
    chain(rc.make(K, 3, seed=1, inactive=False), rc.merge_and_drop(K), retire=False, expect_births=False)


def test_a_retired_index_is_born_again():
    c = rc.make(65, 3, seed=2, inactive=False, new_mass=1.0)                 # alpha[m][K] > 0: new-topic draws have mass
    chain(c, rc.merge_and_drop(65), retire=True, expect_births=True)


# ---- 3. a live sweep after drops ----------------------------------------------------------------------------------------------------------
def test_a_live_sweep_assigns_what_was_dropped():
    c = rc.make(100, 3, seed=3, empty_view=-1)
    with load(c) as s:
        s.sweep(0, 5)
        st = s.remap_topics(surgery.prune_map(sum(s.get_counts(m)[1].astype(np.int64) for m in range(c.M)), 40))
        assert st.dropped.sum() > 0 and any((s.get_assignments(m) < 0).any() for m in range(c.M))
        s.sweep(1, 5, flags=SWEEP_LIVE)
        for m in range(c.M):
            z = s.get_assignments(m)
            assert (z >= 0).all(), m
            nwk, nk = s.get_counts(m)
            ref_nwk, ref_nk = rn.counts_of(c.K, c.V[m], c.tokens[m], z)
            assert np.array_equal(nwk, ref_nwk) and np.array_equal(nk, ref_nk), m


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def refused(s, code, tm, needle, retire=False):
    before = state_of(s) if needle != "set_hyper" else None
    with pytest.raises(MvhdpError) as e:
        s.remap_topics(tm, retire=retire)
    assert e.value.code == code and needle in str(e.value), (code, needle, str(e.value))
    assert before is None or state_of(s) == before, needle


def test_refusals_leave_everything_as_it_was():
    c = rc.make(65, 3, seed=4, inactive=False)
    ident, K = surgery.identity_map(c.K), c.K
    tm = rc.merge_and_drop(K)
    with load(c) as s:
        for bad in (-2, K, 2 ** 31 - 1):
            t = tm.copy(); t[K - 1] = bad
            refused(s, INV, t, "outside")
        before = state_of(s)
        assert s.L.mvhdp_remap_topics(s.h, None, None) == INV and s.L.mvhdp_remap_topics(None, None, None) == INV
        from mvtopicmodel_amd._lib import RemapArgsC
        import ctypes as C
        assert s.L.mvhdp_remap_topics(s.h, C.byref(RemapArgsC(None, 0)), None) == INV
        assert s.L.mvhdp_remap_topics(s.h, C.byref(RemapArgsC(tm.ctypes.data, 2)), None) == INV          # an unknown flag
        assert state_of(s) == before
        with pytest.raises(ValueError):
            s.remap_topics(tm[:-1])
        s.set_assignments(0, c.z[0])                                         # the counts are stale
        refused(s, STATE, tm, "not current")
        s.build_counts()
        s.sweep(0, 9, flags=SWEEP_NO_APPLY)                                  # a NO_APPLY sweep's deltas wait
        refused(s, STATE, tm, "pending")
        s.apply_delta()
        s.apply_delta_begin()                                                # an open bracket
        refused(s, STATE, tm, "bracket")
        s.apply_delta_rows(0, sum(c.V)); s.apply_delta_end()
        rng = np.random.default_rng(0)
        e = rng.random((K, c.V[0])) + 0.1
        s.set_vectors_mix(0.25, e, e.sum(1))                                 # a mix: its columns belong to topics
        refused(s, UNSUPPORTED, tm, "mix")
        refused(s, UNSUPPORTED, ident, "mix", retire=True)
        s.set_vectors_mix(0.0)
        s.emb_init(EmbConfig.defaults(num_columns=8, num_context_columns=4, sampling_table_size=1000))
        refused(s, UNSUPPORTED, tm, "embeddings")
        s.emb_release()
        s.emb_init(EmbConfig.defaults(with_topics=False, num_columns=8, sampling_table_size=1000))      # no topic rows: nothing in the way
        assert s.remap_topics(tm).dropped.sum() > 0
    with load(c, counts=False) as s:                                         # no counts yet
        refused(s, STATE, tm, "not current")
    with NativeSampler(c.K, c.V) as s:                                       # before set_hyper
        for m in range(c.M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m]); s.set_assignments(m, c.z[m])
        s.build_counts()
        refused(s, STATE, tm, "set_hyper")
        z = s.get_assignments(0)
        assert np.array_equal(z, c.z[0]) and np.array_equal(s.get_counts(0)[1], rn.counts_of(K, c.V[0], c.tokens[0], z)[1])


# ---- 5. the side calls that read the counts -------------------------------------------------------------------------------------------------
def test_top_words_follow_a_permutation():
    c = rc.make(65, 3, seed=5)
    with load(c) as s:
        weight = sum(s.get_counts(m)[1].astype(np.int64) for m in range(c.M))
        perm = surgery.order_map(weight, s.get_alpha()[1])
        assert sorted(perm.tolist()) == list(range(c.K)) and (perm != np.arange(c.K)).any()
        before = [s.top_words(m, 7) for m in range(c.M)]
        st = s.remap_topics(perm)
        assert (st.dropped.sum(), st.vacated) == (0, 0) and st.moved.sum() > 0
        for m in range(c.M):
            for name, old, new in zip(("types", "counts", "nonzero"), before[m], s.top_words(m, 7)):
                assert np.array_equal(new[perm], old), (m, name)
        new_weight = sum(s.get_counts(m)[1].astype(np.int64) for m in range(c.M))
        assert np.array_equal(new_weight[perm], weight)
        n_on = int((s.get_alpha()[1] == 0).sum())
        assert (np.diff(new_weight[:n_on]) <= 0).all() and s.get_alpha()[1][n_on:].all()


# ---- 6. a group of two members on one device --------------------------------------------------------------------------------------------------
def test_a_group_remaps_as_one_handle_does():
    c = rc.make(65, 3, seed=6, inactive=False)
    tm = rc.merge_and_drop(c.K)
    parts = rc.split(c, 90)
    shards = [load(p, counts=False, doc_id_base=p.base) for p in parts]
    with load(c) as one, NativeGroup(shards) as g:
        g.build_counts()
        want = one.remap_topics(tm, retire=True)
        got = g.remap_topics(tm, retire=True)
        assert np.array_equal(got.moved, want.moved) and np.array_equal(got.dropped, want.dropped)       # summed over the members
        assert (got.vacated, got.retired) == (want.vacated, want.retired)

        def same_as_one(what):
            for m in range(c.M):
                assert np.array_equal(np.concatenate([sh.get_assignments(m) for sh in shards]), one.get_assignments(m)), (what, "z", m)
                for sh in shards:
                    a, b = sh.get_counts(m), one.get_counts(m)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, "counts", m)
            for sh in shards:
                assert sh.get_alpha()[0].tobytes() == one.get_alpha()[0].tobytes() and np.array_equal(sh.get_alpha()[1], one.get_alpha()[1]), what

        same_as_one("remap")
        one.sweep(0, 21); g.sweep(0, 21)
        same_as_one("the sweep after it")
        # a failed group: the aborted sweep leaves the counts stale until the collective recount
        g.abort()
        refused_group(g, shards, tm, "abort")
        with pytest.raises(MvhdpError):
            g.sweep(1, 21)
        refused_group(g, shards, tm, "not current")
        g.build_counts()
        g.remap_topics(surgery.identity_map(c.K))
    for sh in shards:
        sh.close()


def test_an_undrained_group_refuses():
    c = rc.make(65, 3, seed=7, inactive=False, unassigned=False)
    parts = rc.split(c, 90)
    shards = [load(p, counts=False, doc_id_base=p.base) for p in parts]
    with NativeGroup(shards) as g:
        g.build_counts()
        g.sweep(0, 3, flags=SWEEP_LIVE | SWEEP_ASYNC_EXCHANGE)               # its exchange is still on the wire
        refused_group(g, shards, rc.merge_and_drop(c.K), "drain")
        g.drain()
        assert g.remap_topics(rc.merge_and_drop(c.K)).moved.sum() > 0
    for sh in shards:
        sh.close()


def refused_group(g, shards, tm, needle):
    before = [state_of(sh) for sh in shards]
    with pytest.raises(MvhdpError) as e:
        g.remap_topics(tm)
    assert e.value.code == STATE and needle in str(e.value), str(e.value)
    assert [state_of(sh) for sh in shards] == before
