"""mvhdp_split_topic on a device against the sequential restatement of its contract (tests/native/split_ref.c): every integer, every bit of
alpha, the statistics and the flips of every iteration.  The corpora (tests/split_cases.py) hold a few thousand tokens at the shapes where
the device code takes another path.  The chain test shows that nothing derived from the old topics survives the call: a handle that was
split and a fresh handle loaded with the restatement's result go on sweeping alike, integer for integer.

The handles of the first test sit at the largest doc_id_base their corpus fits under (mvhdp_set_corpus admits doc_id_base + D < 2^29), so
the low counter word is far from zero; a base of 2^32 + 5, where the high word counts too, is beyond what a handle admits and is checked on
the restatement alone (tests/test_split_kats.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, surgery
from mvtopicmodel_amd._lib import SplitArgsC
from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY, SWEEP_SEGMENT_APPLY, EmbConfig
from tests import split_cases as sc
from tests import split_ref as sr
from tests.helpers import INV, STATE, UNSUPPORTED, assert_holds, assert_same_handles, hyper_with, load, state_of

pytestmark = pytest.mark.gpu


def reset(s, c):
    for m in range(c.M):
        s.set_assignments(m, c.z[m])
    s.set_hyper(c.hy)
    s.build_counts()


def assert_stats(st, want, what):
    assert np.array_equal(st.split, want.split) and np.array_equal(st.moved, want.moved), (what, st, want.split, want.moved)
    assert np.array_equal(st.flips, want.flips) and st.flips_last == want.flips_last, (what, st.flips, want.flips)
    assert (st.target, int(st.activated)) == (want.target, want.activated) and st.kernel_ms > 0.0, (what, st)


# ---- 1. every integer and bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", sc.M_VALUES)
@pytest.mark.parametrize("K", sc.K_VALUES)
def test_every_integer_and_bit_equals_the_restatement(K, M):
    c = sc.make(K, M)
    base = sc.handle_doc_id_base(c)
    hint, P = sc.hints(c), sc.coupling(M)
    with load(c, doc_id_base=base) as s, load(c, doc_id_base=base) as second:
        first = True
        for iterations, hinted, coupled, keep in itertools.product(sc.ITERATIONS, (False, True), (False, True), (False, True)):
            what = (K, M, iterations, hinted, coupled, keep)
            kw = dict(iterations=iterations, seed=1000 + iterations, coupling=P if coupled else None, type_hint=hint if hinted else None, keep_alpha=keep)
            if not first:
                reset(s, c)
            want = sr.run(K, c.V, c.doc_off, c.tokens, c.z, c.hy, c.source, doc_id_base=base, **kw)
            assert want.rc == 0 and 0 < want.moved.sum() < want.split.sum()
            st = s.split_topic(c.source, **kw)
            assert_holds(s, c, want, sr.counts_of, what)
            assert_stats(st, want, what)
            for m in range(M):                                               # the counts are those mvhdp_build_counts makes of z'
                second.set_assignments(m, want.z[m])
            second.build_counts()
            assert_same_handles(s, second, M, what)
            if first:                                                        # the same call on another handle: the same bytes
                reset(second, c)
                st2 = second.split_topic(c.source, **kw)
                assert state_of(second) == state_of(s) and np.array_equal(st2.flips, st.flips), what
            first = False
        assert want.flips.sum() > 0                                          # (the last configuration ran five iterations)


# ---- 2. the chain goes on ---------------------------------------------------------------------------------------------------------------
def test_the_chain_goes_on_as_on_a_fresh_handle():
    # alpha[m][K] > 0: new-topic draws have mass, the births' code runs in every sweep; it is small enough that the two sweeps in front
    # of the split leave the inactive set alone (0.05 has both its indices born by then)
    c = sc.make(65, 3, seed=2, new_mass=1e-9)
    K, M = c.K, c.M
    sweeps = [(2, 0, "deferred"), (3, SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(4), "segment apply")]
    with load(c) as a:
        a.sweep(0, 17); a.sweep(1, 17)                                       # mirrors, class bytes, slot counts and trees of the OLD topics exist
        z = [a.get_assignments(m) for m in range(M)]
        alpha, off = a.get_alpha()
        weight = sum(a.get_counts(m)[1].astype(np.int64) for m in range(M))
        free = surgery.free_topics(weight, off, alpha)
        assert len(free) > 0 and off[free[0]]                                # the target comes out of the inactive set
        source = int(np.argmax(weight))
        kw = dict(iterations=5, seed=77, type_hint=sc.hints(c))
        want = sr.run(K, c.V, c.doc_off, c.tokens, z, hyper_with(c, alpha, off), source, **kw)
        st = a.split_topic(source, **kw)
        assert_stats(st, want, "chain")
        assert st.activated and st.target == free[0] and 0 < st.moved.sum() < st.split.sum()
        with load(c, z=want.z, hy=hyper_with(c, want.alpha, want.inactive)) as b:
            assert_same_handles(a, b, M, "before the sweeps")
            for idx, flags, name in sweeps:
                offs = [x.get_alpha()[1] for x in (a, b)]
                assert np.array_equal(offs[0], offs[1])
                sa, sb = a.sweep(idx, 17, flags=flags), b.sweep(idx, 17, flags=flags)
                assert_same_handles(a, b, M, name)
                assert (sa.tokens, sa.changed, sa.activations, sa.activated_topic) == (sb.tokens, sb.changed, sb.activations, sb.activated_topic), name
                assert a.model_log_likelihood().tobytes() == b.model_log_likelihood().tobytes(), name
                assert a.get_alpha()[0].tobytes() == b.get_alpha()[0].tobytes(), name
            assert (a.get_assignments(0) == st.target).any()                 # the new topic lives on
            # A live sweep is racy by design (two handles in the same state do not agree after one: tests/test_gpu_handle_state.py), so
            # it is held to the live sweeps' invariants on both handles, not to each other.
            sa, sb = a.sweep(4, 17, flags=SWEEP_LIVE), b.sweep(4, 17, flags=SWEEP_LIVE)
            assert sa.tokens == sb.tokens == sum(len(t) for t in c.tokens)
            for x in (a, b):
                for m in range(M):
                    zx = x.get_assignments(m)
                    assert (zx >= 0).all(), m
                    nwk, nk = x.get_counts(m)
                    ref_nwk, ref_nk = sr.counts_of(K, c.V[m], c.tokens[m], zx)
                    assert np.array_equal(nwk, ref_nwk) and np.array_equal(nk, ref_nk), m


# ---- 3. split, then merge back -------------------------------------------------------------------------------------------------------------
def test_a_merge_undoes_the_split_and_a_retired_index_splits_again():
    c = sc.make(65, 3, seed=3)
    with load(c) as s:
        before = state_of(s)
        alpha0, off0 = s.get_alpha()
        st = s.split_topic(c.source, iterations=5, seed=9)
        after_split = state_of(s)
        assert st.target == c.free[0] and st.moved.sum() > 0 and after_split != before
        back = surgery.identity_map(c.K)
        back[st.target] = c.source
        rs = s.remap_topics(back)
        assert np.array_equal(rs.moved, st.moved)
        for m in range(c.M):
            assert np.array_equal(s.get_assignments(m), c.z[m]), m
            nwk, nk = s.get_counts(m)
            ref_nwk, ref_nk = sr.counts_of(c.K, c.V[m], c.tokens[m], c.z[m])
            assert np.array_equal(nwk, ref_nwk) and np.array_equal(nk, ref_nk), m
        alpha, off = s.get_alpha()
        assert alpha.tobytes() == alpha0.tobytes()                           # 0.5 a + 0.5 a == a
        assert not off[st.target] and off0[st.target]                        # the index is still in use
        rs = s.remap_topics(back, retire=True)                               # nothing maps onto it: it returns to the inactive set
        assert (rs.vacated, rs.retired, int(rs.moved.sum())) == (1, 1, 0)
        assert state_of(s) == before
        again = s.split_topic(c.source, iterations=5, seed=9)                # and a second split takes it again, to the same bytes
        assert again.target == st.target and again.activated and np.array_equal(again.flips, st.flips)
        assert state_of(s) == after_split


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------------
def refused(s, code, needle, source=0, **kw):
    before = state_of(s) if needle != "set_hyper" else None
    with pytest.raises(MvhdpError) as e:
        s.split_topic(source, **kw)
    assert e.value.code == code and needle in str(e.value), (code, needle, str(e.value))
    assert before is None or state_of(s) == before, needle


def test_refusals_leave_everything_as_it_was():
    c = sc.make(65, 3, seed=4)
    K, free, used = c.K, c.free[0], 1
    with load(c) as s:
        before = state_of(s)
        assert s.L.mvhdp_split_topic(s.h, None, None, None) == INV and s.L.mvhdp_split_topic(None, None, None, None) == INV
        assert s.L.mvhdp_split_topic(s.h, C.byref(SplitArgsC(0, free, 1, 2, 0, None, None)), None, None) == INV          # an unknown flag
        assert "flags" in s.L.mvhdp_last_error(s.h).decode()
        assert state_of(s) == before
        for src in (-1, K, 2 ** 31 - 1):
            refused(s, INV, "source out of range", source=src, target=free)
        for t in (-2, K):
            refused(s, INV, "target out of range", target=t)
        refused(s, INV, "source == target", target=0)
        refused(s, INV, "inactive set", source=free, target=c.free[1])
        refused(s, INV, "iterations", target=free, iterations=-1)
        refused(s, INV, "iterations", target=free, iterations=65536)
        refused(s, INV, "holds tokens", target=used)
        bad = sc.hints(c); bad[0] = bad[0].copy(); bad[0][3] = 2
        refused(s, INV, "type_hint", target=free, type_hint=bad)
        P = sc.coupling(c.M); P[1, 2] = -0.5
        refused(s, INV, "coupling", target=free, coupling=P)
        with pytest.raises(ValueError):
            s.split_topic(0, type_hint=[None])
        with pytest.raises(ValueError):
            s.split_topic(0, coupling=np.ones((2, 2)))
        hy = hyper_with(c, np.array(c.hy.alpha), np.array(c.hy.inactive))   # alpha of a free index is not 0.0: no longer free
        hy.alpha[1, free] = 0.125
        s.set_hyper(hy)
        refused(s, INV, "alpha", target=free)
        assert s.split_topic(0, iterations=0).target == c.free[1]            # and target = -1 passes it over
        reset(s, c)
        hy.alpha[1, c.free[1]] = 0.25
        s.set_hyper(hy)
        refused(s, INV, "no free topic")
        reset(s, c)
        s.set_assignments(0, c.z[0])                                         # the counts are stale
        refused(s, STATE, "not current", target=free)
        s.build_counts()
        s.sweep(0, 9, flags=SWEEP_NO_APPLY)                                  # a NO_APPLY sweep's deltas wait
        refused(s, STATE, "pending", target=free)
        s.apply_delta()
        s.apply_delta_begin()                                                # an open bracket
        refused(s, STATE, "bracket", target=free)
        s.apply_delta_rows(0, sum(c.V)); s.apply_delta_end()
        reset(s, c)
        rng = np.random.default_rng(0)
        e = rng.random((K, c.V[0])) + 0.1
        s.set_vectors_mix(0.25, e, e.sum(1))                                 # a mix: its columns belong to topics
        refused(s, UNSUPPORTED, "mix", target=free)
        s.set_vectors_mix(0.0)
        s.emb_init(EmbConfig.defaults(num_columns=8, num_context_columns=4, sampling_table_size=1000))
        refused(s, UNSUPPORTED, "embeddings", target=free)
        s.emb_release()
        s.emb_init(EmbConfig.defaults(with_topics=False, num_columns=8, sampling_table_size=1000))      # no topic rows: nothing in the way
        assert s.split_topic(0, target=free).moved.sum() > 0
    with load(c, counts=False) as s:                                         # no counts yet
        refused(s, STATE, "not current", target=free)
    with NativeSampler(c.K, c.V) as s:                                       # before set_hyper
        for m in range(c.M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m]); s.set_assignments(m, c.z[m])
        s.build_counts()
        refused(s, STATE, "set_hyper", target=free)
        assert np.array_equal(s.get_assignments(0), c.z[0])
    with NativeSampler(c.K, c.V) as s:                                       # before set_corpus of every view
        s.set_corpus(0, c.doc_off[0], c.tokens[0])
        with pytest.raises(MvhdpError) as e:
            s.split_topic(0, target=free)
        assert e.value.code == STATE and "set_corpus" in str(e.value)


# ---- 5. the library picks the target ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [65, 2048])
def test_the_library_picks_the_first_free_topic(K):
    c = sc.make(K, 3, seed=5)
    with load(c) as s:
        weight = sum(s.get_counts(m)[1].astype(np.int64) for m in range(c.M))
        alpha, off = s.get_alpha()
        free = surgery.free_topics(weight, off, alpha)
        assert free.tolist() == c.free and len(free) == 2
        st = s.split_topic(c.source, iterations=1)
        assert (st.target, st.activated) == (free[0], True)
        weight = sum(s.get_counts(m)[1].astype(np.int64) for m in range(c.M))
        alpha, off = s.get_alpha()
        assert surgery.free_topics(weight, off, alpha).tolist() == [free[1]] and weight[st.target] == st.moved.sum()
        assert s.split_topic(c.source, iterations=2).target == free[1]       # the second free index, then none is left
        with pytest.raises(MvhdpError) as e:
            s.split_topic(c.source)
        assert e.value.code == INV and "no free topic" in str(e.value)
