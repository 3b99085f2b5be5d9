"""Every compiled sweep kernel against its reference, with the launch census (NativeSampler.sweep_census) as witness that it was THAT
kernel whose integers were compared: the recipes of tests/census_cases.py, each three sweeps on its smallest corpus, held to the
reference the way the existing test of its mode holds it; then the census must show launches and tokens in the recipe's row, and its
token total must be the sweeps'.  The census itself: off means nothing is counted, and on means nothing else changes, bit for bit."""
import numpy as np
import pytest

from mvtopicmodel_amd.native import (SWEEP_FROZEN, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_ONLY_SEGMENT, SWEEP_SEGMENT_APPLY,
                                     SWEEP_SEGMENT_OVERLAP, Hyper)
from tests import census_cases as cc
from tests.helpers import assert_same_state, make_native, make_oracle, same_statistics

pytestmark = pytest.mark.gpu
SEED = 0xC0FFEE
SWEEPS = 3


def census_text(rows):
    """the non-zero rows, one a line: where a recipe that drifted went"""
    return "\n".join(f"  {r.key}: {r.launches} launches, {r.tokens} tokens" for r in rows if r.launches or r.tokens) or "  (empty)"


def check_census(r, s, sampled):
    rows = s.sweep_census()
    text = census_text(rows)
    print(f"[census] {r.name}\n{text}")
    by_key = {row.key: row for row in rows}
    assert len(rows) == 60 and len(by_key) == 60
    mine = by_key[r.key]
    assert mine.launches >= 1 and mine.tokens > 0, f"{r.name}: the kernel {r.key} it is written for sampled nothing; the census:\n{text}"
    assert sum(row.tokens for row in rows) == sampled, f"{r.name}: the census counted other tokens than the sweeps' {sampled}:\n{text}"
    # a recipe's entities all fit its forced variant and nothing moves its flavour between the sweeps (census_cases.py): every integer
    # compared above was that kernel's
    assert mine.tokens == sampled, f"{r.name}: some of the {sampled} tokens were sampled by another kernel than {r.key}:\n{text}"


def debug_rows_as_the_oracle(ro, rs, M, where):
    """tests/test_gpu_parity.py::test_one_sweep_bit_exact: newTopicMass and tree[1] bit for bit, the two masses within the scan's reordering"""
    for m in range(M):
        a, b = ro["dbg"][m], rs.dbg[m]
        assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 2], b[:, 2]), where
        assert np.allclose(a[:, 1], b[:, 1], rtol=1e-12, atol=0) and np.allclose(a[:, 3], b[:, 3], rtol=1e-12, atol=0), where


def run_against_the_oracle(r, c, hy):
    from oracle.binding import SWEEP_FROZEN as ORC_FROZEN
    from tests.near_ties import longest_first
    from tests.test_gpu_segmented import oracle_segmented_sweep
    o = make_oracle(c, hy)
    s = make_native(c, hy, [o.get_assignments(m) for m in range(c.M)])
    s.set_tuning(**r.tuning)
    s.sweep_census(enable=True, reset=True)
    if r.mode == "frozen":
        o.build_trees(); s.build_trees()
    order = longest_first(c.doc_off)
    sampled = 0
    for it in range(SWEEPS):
        where = f"{r.name} sweep {it}"
        if r.mode == "live":
            # tests/test_gpu_live.py::_one_wave_against_the_oracle
            ro = o.sweep_live_seq(it, SEED, order, nseg=1, rows=1, cell16=r.tuning["live16"])["stats"]
            st = s.sweep(it, SEED, flags=r.flags)
            assert (st.tokens, st.changed) == (ro["tokens"], ro["changed"]), f"{where}: {st.changed} changed against the oracle's {ro['changed']}"
            assert (st.new_mass_cnt, st.topic_doc_mass_cnt, st.word_ftree_mass_cnt) == (ro["new_mass_cnt"], ro["topic_doc_mass_cnt"], ro["word_ftree_mass_cnt"]), where
            assert st.word_ftree_mass_cnt > 0, where
        else:
            if r.mode == "segmented":
                ref, first = oracle_segmented_sweep(o, c, it, SEED, cc.SEGMENTS)
                ref = dict(ref, activated_topic=first[1], activated_modality=first[2])
            else:
                ro = o.sweep(it, SEED, flags=ORC_FROZEN if r.mode == "frozen" else 0, want_dbg=r.dbg)
                ref = ro["stats"]
            st = s.sweep(it, SEED, flags=r.flags, want_dbg=r.dbg)
            same_statistics(st, ref, where)
            if r.dbg:
                debug_rows_as_the_oracle(ro, st, c.M, where)
        try:
            assert_same_state(o, s, c.M)
        except AssertionError as e:
            raise AssertionError(f"{where}: {e}\n{census_text(s.sweep_census())}") from None
        sampled += st.tokens
    check_census(r, s, sampled)
    s.close(); o.close()


def run_against_the_mix_restatement(r, c, hy):
    """tests/test_gpu_vectors_mix.py::sweeps_against_ref, with the census switched on between the handle and its sweeps"""
    from mvtopicmodel_amd.native import SWEEP_GENERIC_KERNEL
    from tests.mix_cases import same_state, same_stats, table
    from tests.test_gpu_vectors_mix import check_debug, pair, trace_of
    e, S = table(c.K, c.V[0], 7)
    ref, s = pair(c, hy, None, cc.MIX_LAMBDA, e, S, **r.tuning)
    s.sweep_census(enable=True, reset=True)
    trace = trace_of(c) if r.dbg else None
    sampled = 0
    for it in range(SWEEPS):
        where = f"{r.name} sweep {it}"
        rr = ref.sweep(it, SEED, want_dbg=r.dbg, trace=trace, trace_product=not (r.flags & SWEEP_GENERIC_KERNEL))
        rs = s.sweep(it, SEED, flags=r.flags, want_dbg=r.dbg, trace=trace)
        assert rr["stats"]["aborted_docs"] == 0, where
        same_stats(rr["stats"], rs, where)
        same_state(ref, s, c.M, where)
        if r.dbg:
            check_debug(c, rr, rs, trace, False, where)
        sampled += rs.tokens
    check_census(r, s, sampled)
    ref.close(); s.close()


@pytest.mark.parametrize("r", cc.RECIPES, ids=lambda r: r.name)
def test_the_recipes_kernel_ran_and_its_integers_are_the_references(r, monkeypatch):
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    c, hy = cc.corpus(r.K, r.R), cc.hyper(r.K)
    (run_against_the_mix_restatement if r.mode == "mix" else run_against_the_oracle)(r, c, hy)


# ---- the census itself ----
def routed_corpus():
    """K beyond 512, entities from 25 to 1100 tokens and nothing forced: a primary kernel and wider classes beside it on the side streams,
    so a segment's fold has several blocks to add"""
    from mvtopicmodel_amd.synth import Corpus
    K, V = 600, [2000, 60]
    rng = np.random.RandomState(19)
    lens0 = np.array([700, 1100, 40, 300, 560, 130, 90, 260] + [25] * 40, dtype=np.int64)
    lens1 = rng.randint(0, 9, len(lens0)).astype(np.int64)
    off = [np.concatenate([[0], np.cumsum(l)]) for l in (lens0, lens1)]
    return Corpus(K, V, off, [rng.randint(0, V[m], off[m][-1]).astype(np.int32) for m in range(2)])


STAT_FIELDS = ("tokens", "changed", "new_mass_cnt", "topic_doc_mass_cnt", "word_ftree_mass_cnt", "oov_skipped", "aborted_docs",
               "exact_fallbacks", "activated_topic", "activated_modality", "activation_key", "activations")


def chain(c, hy, z0, mode, census):
    """four sweeps of one handle; everything they returned and left behind"""
    s = make_native(c, hy, z0)
    if census:
        s.sweep_census(enable=True, reset=True)
    if mode == "many":
        sts = s.sweep_many(0, 4, SEED)
    else:
        flags = {"deferred": [0], "segmented": [SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(3)],
                 "overlapped": [SWEEP_SEGMENT_APPLY | SWEEP_SEGMENT_OVERLAP | SWEEP_LIVE_SEGMENTS(4)],
                 "only_segment": [SWEEP_LIVE_SEGMENTS(2) | SWEEP_ONLY_SEGMENT(0), SWEEP_LIVE_SEGMENTS(2) | SWEEP_ONLY_SEGMENT(1)]}[mode]
        sts = [s.sweep(it, SEED, flags=flags[it % len(flags)]) for it in range(4)]
    out = dict(stats=[tuple(getattr(st, f) for f in STAT_FIELDS) for st in sts],
               z=[s.get_assignments(m) for m in range(c.M)], counts=[s.get_counts(m) for m in range(c.M)],
               shares=list(s.get_tuning().tree_branch_share), steps=list(s.get_tuning().learnt_walk_step),
               census=s.sweep_census())
    s.close()
    return out


@pytest.mark.parametrize("mode", ["deferred", "segmented", "overlapped", "many", "only_segment"])
def test_the_census_changes_nothing_else(mode):
    """The same chain on a handle with the census off and on one with it on: every statistic a sweep returns, what the walk search
    learnt from the per-view counters, every assignment and every count, bit for bit; and the census' tokens are the sweeps'."""
    c = routed_corpus()
    hy = Hyper.defaults(c.K, c.V)
    o = make_oracle(c, hy)
    z0 = [o.get_assignments(m) for m in range(c.M)]
    o.close()
    off, on = chain(c, hy, z0, mode, False), chain(c, hy, z0, mode, True)
    assert off["stats"] == on["stats"]
    assert off["shares"] == on["shares"] and off["steps"] == on["steps"]
    for m in range(c.M):
        assert np.array_equal(off["z"][m], on["z"][m]), f"z of view {m}"
        assert np.array_equal(off["counts"][m][0], on["counts"][m][0]) and np.array_equal(off["counts"][m][1], on["counts"][m][1]), f"counts of view {m}"
    text = census_text(on["census"])
    print(f"[census] identity {mode}\n{text}")
    assert all(r.launches == 0 and r.tokens == 0 for r in off["census"])
    assert sum(r.tokens for r in on["census"]) == sum(st[0] for st in on["stats"]), text
    assert sum(1 for r in on["census"] if r.tokens) >= 2, f"one kernel only: nothing was routed\n{text}"


def test_a_census_never_switched_on_counts_nothing():
    c, hy = cc.corpus(100, 1), cc.hyper(100)
    o = make_oracle(c, hy)
    s = make_native(c, hy, [o.get_assignments(m) for m in range(c.M)])
    assert s.sweep(0, SEED).tokens == c.total_tokens
    rows = s.sweep_census()
    assert len(rows) == 60 and len({r.key for r in rows}) == 60
    assert [r.key[0] for r in rows[56:]] == [0] * 4 and all(r.key[0] in (1, 2, 4, 8, 16) for r in rows[:56])
    assert all(r.launches == 0 and r.tokens == 0 for r in rows)
    # switched on, off again, and read with a reset: the tallies of the sweep in between, then none
    s.sweep_census(enable=True)
    st = s.sweep(1, SEED)
    rows = s.sweep_census(enable=False)
    assert sum(r.tokens for r in rows) == st.tokens and sum(r.launches for r in rows) >= 1
    s.sweep(2, SEED)
    assert sum(r.tokens for r in s.sweep_census()) == st.tokens
    assert all(r.launches == 0 and r.tokens == 0 for r in s.sweep_census(reset=True))
    s.close(); o.close()


def test_two_live_segments_in_flight_are_counted_once_each():
    """a live sweep with overlapped segments (two in flight, each on its own set of blocks): racy integers, exact totals"""
    c = routed_corpus()
    hy = Hyper.defaults(c.K, c.V)
    o = make_oracle(c, hy)
    s = make_native(c, hy, [o.get_assignments(m) for m in range(c.M)])
    o.close()
    s.set_tuning(live_rows=0, live_overlap=1)
    s.sweep_census(enable=True, reset=True)
    sts = [s.sweep(it, SEED, flags=SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(5)) for it in range(3)]
    rows = s.sweep_census()
    assert all(st.tokens == c.total_tokens for st in sts)
    assert sum(r.tokens for r in rows) == 3 * c.total_tokens, census_text(rows)
    s.close()
