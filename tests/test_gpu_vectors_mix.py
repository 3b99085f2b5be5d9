"""The sweep with the embeddings' p(w|t) mixed in (mvhdp_set_vectors_mix; WRK:504-507, PTM:2673-2678) on the device, against the
sequential restatement tests/native/mix_ref.c: every deferred mode and every kernel class gives its integers, the debug doubles
follow it, the trees are its trees bit for bit; live sweeps keep their invariants; off is off.

Debug doubles.  Wherever the device sums sequentially (MVHDP_SWEEP_EXACT_CHAIN, every kernel class) tok_dbg AND the traced
conditionals are compared bit for bit.  The traced conditional of a listed topic is leaf / total + term / total; the generic kernel
(like the oracle) takes the term as the difference of two running sums, the register kernels as the product itself, and the
restatement gives either form (MixRef.sweep(trace_product=)): each kernel class is held to its own form, bit for bit.
In the other modes the document-term sum of the debug flavour is the wave's prefix scan, which differs from the sequential sum of the
same non-negative terms by less than 2n ulp of the total (the bound the kernels certify their decisions with, n = the length of the
list <= K; tests/test_gpu_parity.py holds the sweep without a mix to the same): newMass and tree[1] are compared bit for bit, the
mass and the sample within (4 K + 16) 2^-53 relative, the traced probabilities (<= 1, each a quotient by that total) within twice
that, absolute."""
import numpy as np
import pytest

from mvtopicmodel_amd.native import (SWEEP_EXACT_CHAIN, SWEEP_FROZEN, SWEEP_GENERIC_KERNEL, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY,
                                     SWEEP_REUSE_TREES, SWEEP_SEGMENT_APPLY, EmbConfig, Hyper, MvhdpError, NativeGroup)
from tests import mix_near_ties, near_ties
from tests.helpers import After, make_native, make_oracle, rung_name, served_class, small_corpus
from tests.mix_cases import inactive_case, make_ref, ragged_corpus, same_state, same_stats, table
from tests.mix_ref import make_mix

pytestmark = pytest.mark.gpu

def _codes():
    """mvhdp_status of include/mvhdp.h"""
    return {"MVHDP_ERR_INVALID_ARG": -1, "MVHDP_ERR_STATE": -2, "MVHDP_ERR_UNSUPPORTED": -6}


def pair(c, hy, z0, lam, e, S, **tuning):
    """the restatement and a sampler in the same state, the same mix set on both"""
    r = make_ref(c, hy, z0)
    z = [r.get_assignments(m) for m in range(c.M)]
    s = make_native(c, hy, z)
    if tuning:
        s.set_tuning(**tuning)
    r.set_vectors_mix(lam, e, S); s.set_vectors_mix(lam, e, S)
    return r, s


def trace_of(c, step=3):
    out = []
    for d in range(0, c.D, step):
        for m in range(c.M):
            L = int(c.doc_off[m][d + 1] - c.doc_off[m][d])
            for pos in sorted({0, L // 2, L - 1}):
                if 0 <= pos < L and c.tokens[m][c.doc_off[m][d] + pos] < c.V[m]:
                    out.append((d, m, pos))
    return out


def check_debug(c, rr, rs, trace, exact, where):
    visited = [c.tokens[m] < c.V[m] for m in range(c.M)]
    rtol = (4 * c.K + 16) * 2.0 ** -53
    for m in range(c.M):
        a, b = rr["dbg"][m][visited[m]], rs.dbg[m][visited[m]]
        if exact:
            assert np.array_equal(a, b), f"{where}: tok_dbg of view {m}"
        else:
            assert np.array_equal(a[:, 0], b[:, 0]) and np.array_equal(a[:, 2], b[:, 2]), f"{where}: newMass / tree[1] of view {m}"
            assert np.allclose(a[:, 1], b[:, 1], rtol=rtol, atol=0) and np.allclose(a[:, 3], b[:, 3], rtol=rtol, atol=0), f"{where}: masses of view {m}"
    if trace and exact:
        assert np.array_equal(rr["trace"], rs.trace), f"{where}: traced conditionals"
    elif trace:
        assert np.max(np.abs(rr["trace"] - rs.trace)) <= 2 * rtol, f"{where}: traced conditionals"


def sweeps_against_ref(c, hy, z0, lam, flags=0, tuning=None, n=3, table_seed=7, debug=True):
    e, S = table(c.K, c.V[0], table_seed)
    r, s = pair(c, hy, z0, lam, e, S, **(tuning or {}))
    trace = trace_of(c) if debug else None
    fb = 0
    for it in range(n):
        where = f"lambda {lam} flags {flags:#x} tuning {tuning} sweep {it}"
        rr = r.sweep(it, 0xC0FFEE, want_dbg=debug, trace=trace, trace_product=not (flags & SWEEP_GENERIC_KERNEL))
        rs = s.sweep(it, 0xC0FFEE, flags=flags, want_dbg=debug, trace=trace)
        assert rr["stats"]["aborted_docs"] == 0, where
        same_stats(rr["stats"], rs, where)
        same_state(r, s, c.M, where)
        if debug:
            check_debug(c, rr, rs, trace, bool(flags & SWEEP_EXACT_CHAIN), where)
        fb += rs.exact_fallbacks
    r.close(); s.close()
    print(f"[vectors mix] lambda {lam} flags {flags:#x} tuning {tuning} debug {debug}: exact_fallbacks {fb} in {n} sweeps of {c.total_tokens} tokens")
    return fb


CORPUS = dict(K=100, V=[1500, 200, 200], D=64, lam=[90, 6, 9], seed=31)


def _corpus():
    k = CORPUS
    return small_corpus(k["K"], k["V"], k["D"], k["lam"], k["seed"]), Hyper.defaults(k["K"], k["V"])


@pytest.mark.parametrize("lam", [0.25, 1.0])
@pytest.mark.parametrize("debug", [False, True], ids=["screened", "debug"])
@pytest.mark.parametrize("mode", ["default", "generic", "exact", "exact_generic", "walk0", "walk0.5", "walk2", "narrow0", "segments3"])
def test_deferred_sweeps_equal_the_restatement(lam, mode, debug):
    c, hy = _corpus()
    flags = {"generic": SWEEP_GENERIC_KERNEL, "exact": SWEEP_EXACT_CHAIN, "exact_generic": SWEEP_EXACT_CHAIN | SWEEP_GENERIC_KERNEL,
             "segments3": SWEEP_LIVE_SEGMENTS(3)}.get(mode, 0)
    tuning = {"walk0": dict(walk_fixed=1, walk_theta=[0.0] * 3), "walk0.5": dict(walk_fixed=1, walk_theta=[0.5] * 3),
              "walk2": dict(walk_fixed=1, walk_theta=[2.0] * 3), "narrow0": dict(narrow=0)}.get(mode)
    sweeps_against_ref(c, hy, None, lam, flags=flags, tuning=tuning, debug=debug)


@pytest.mark.parametrize("lam", [0.25, 1.0])
@pytest.mark.parametrize("name,R", [(n, R) for n, (_, forced, _, _) in mix_near_ties.PLAN.items() for R in forced])
def test_every_register_variant_forced(name, R, lam):
    """set_tuning(force_primary=R) on a case whose every entity that variant serves (the planner's own word, helpers.served_class)"""
    case = mix_near_ties.PLAN[name][0]()
    assert served_class(case, R) == R.bit_length() - 1, f"force_primary {R} would not be what serves the entities of {case.name}"
    for debug in (False, True):
        sweeps_against_ref(case, case.hy, case.z0, lam, tuning=dict(force_primary=R), n=2, debug=debug)
    # ... and under the sequential sum, where that variant's debug doubles and traces are the restatement's bit for bit
    sweeps_against_ref(case, case.hy, case.z0, lam, flags=SWEEP_EXACT_CHAIN, tuning=dict(force_primary=R), n=1, debug=True)
    # ... and with the mirror switched off: the variant's mix flavour on the 32-bit table
    sweeps_against_ref(case, case.hy, case.z0, lam, tuning=dict(force_primary=R, narrow=0), n=1, debug=False)


@pytest.mark.parametrize("narrow", [-1, 0])
@pytest.mark.parametrize("lam", [0.25, 1.0])
def test_heavy_word_and_the_mirror(narrow, lam):
    """a type above 65534 tokens (a HEAVY row: 32-bit counts), one between 32768 and 65534, the rest small: the 16-bit mirror and the table"""
    from mvtopicmodel_amd.synth import Corpus
    K, V, D = 24, [40, 7], 2500
    rng = np.random.RandomState(12)
    lens0 = np.full(D, 200, dtype=np.int64); lens1 = rng.randint(0, 5, D).astype(np.int64)
    off = [np.concatenate([[0], np.cumsum(l)]) for l in (lens0, lens1)]
    u = rng.rand(off[0][-1])
    t0 = rng.randint(2, 40, off[0][-1]).astype(np.int32)
    t0[u < 0.5] = 0; t0[(u >= 0.5) & (u < 0.59)] = 1
    c = Corpus(K, V, off, [t0, rng.randint(0, 7, off[1][-1]).astype(np.int32)])
    hy = Hyper.defaults(K, V)
    e, S = table(K, V[0], 4)
    r, s = pair(c, hy, None, lam, e, S, narrow=narrow, walk_fixed=1, walk_theta=[0.3, 0.3])
    tot = s.get_counts(0)[0].sum(axis=1)
    assert tot[0] > 65534 and 32767 < tot[1] <= 65534
    for it in range(3):
        rr = r.sweep(it, 33); rs = s.sweep(it, 33)
        same_stats(rr["stats"], rs, f"sweep {it}"); same_state(r, s, c.M, f"narrow {narrow} sweep {it}")
    r.close(); s.close()


@pytest.mark.parametrize("kflag", [0, SWEEP_GENERIC_KERNEL])
@pytest.mark.parametrize("lam", [0.25, 1.0])
def test_inactive_topics_and_an_activation(lam, kflag):
    c, hy, z0 = inactive_case()
    e, S = table(c.K, c.V[0], 8)
    r, s = pair(c, hy, z0, lam, e, S)
    acts = []
    for it in range(3):
        rr = r.sweep(it, 3, want_dbg=True); rs = s.sweep(it, 3, flags=kflag, want_dbg=True)
        same_stats(rr["stats"], rs, f"sweep {it}"); same_state(r, s, c.M, f"sweep {it}")
        assert rr["stats"]["activation_key"] == rs.activation_key or rs.activated_topic < 0
        a_s, ina_s = s.get_alpha()
        assert np.array_equal(r.get_alpha(), a_s) and np.array_equal(r.get_inactive(), ina_s)
        acts.append(rs.activated_topic)
        # the rebuilt trees after the activation carry the mix, an inactive topic's leaf is 0
        r.build_trees(); s.build_trees()
        for w in (0, 1, 17, c.V[0] - 1):
            t = s.get_tree(0, w)
            assert np.array_equal(r.get_tree(0, w), t)
            assert not t[c.K:][ina_s.astype(bool)].any()
    assert acts[0] == 33 and rs.new_mass_cnt > 0
    r.close(); s.close()


@pytest.mark.parametrize("kflag", [0, SWEEP_GENERIC_KERNEL])
@pytest.mark.parametrize("lam", [0.25, 1.0])
def test_oov_types_missing_views_and_unassigned_tokens(lam, kflag):
    """entities without view 0, with view 0 only, empty ones; OOV tokens (WRK:427-428); unassigned ones"""
    c, z0 = ragged_corpus(K=30)
    hy = Hyper.defaults(c.K, c.V)
    e, S = table(c.K, c.V[0], 6)
    r, s = pair(c, hy, z0, lam, e, S)
    for it in range(3):
        rr = r.sweep(it, 77, want_dbg=True); rs = s.sweep(it, 77, flags=kflag, want_dbg=True)
        assert rs.oov_skipped == 3
        same_stats(rr["stats"], rs, f"sweep {it}"); same_state(r, s, c.M, f"sweep {it}")
    r.close(); s.close()


@pytest.mark.parametrize("lam", [0.25, 1.0])
def test_segment_apply_no_apply_rows_and_sweep_many(lam):
    c, hy = _corpus()
    e, S = table(c.K, c.V[0], 7)
    # SEGMENT_APPLY with 3 segments: the restatement's list sweeps over the segments of the longest-first order, applied in between
    r, s = pair(c, hy, None, lam, e, S)
    order = near_ties.longest_first(c.doc_off)
    for it in range(2):
        tok = 0
        for seg in range(3):
            tok += r.sweep_list(it, 21, order[seg::3])["stats"]["tokens"]
        rs = s.sweep(it, 21, flags=SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(3))
        assert rs.tokens == tok == c.total_tokens and rs.aborted_docs == 0
        same_state(r, s, c.M, f"SEGMENT_APPLY sweep {it}")
    # NO_APPLY + the row pipeline in two row ranges: counts updated and the trees of those rows rebuilt WITH the mix
    nrows = sum(c.V)
    for it in range(2, 4):
        rr = r.sweep(it, 21); rs = s.sweep(it, 21, flags=SWEEP_NO_APPLY)
        same_stats(rr["stats"], rs, f"NO_APPLY sweep {it}")
        s.apply_delta_begin(); s.apply_delta_rows(0, 700); s.apply_delta_rows(700, nrows); s.apply_delta_end(-1, -1)
        same_state(r, s, c.M, f"NO_APPLY sweep {it}")
        assert s.trees_current() == 1
        r.build_trees()
        for m, w in [(0, 0), (0, 699), (0, 700), (0, 1499), (1, 3), (2, 199)]:
            assert np.array_equal(r.get_tree(m, w), s.get_tree(m, w)), (m, w)
    # the next sweep may start from those trees
    rr = r.sweep(4, 21); rs = s.sweep(4, 21, flags=SWEEP_REUSE_TREES)
    same_stats(rr["stats"], rs, "REUSE_TREES"); same_state(r, s, c.M, "REUSE_TREES after the row pipeline")
    # sweep_many of 4 = 4 single sweeps
    s2 = make_native(c, hy, [s.get_assignments(m) for m in range(c.M)])
    s2.set_vectors_mix(lam, e, S)
    sts = s.sweep_many(5, 4, 21)
    for i in range(4):
        rr = r.sweep(5 + i, 21); r2 = s2.sweep(5 + i, 21)
        same_stats(rr["stats"], sts[i], f"sweep_many {i}"); same_stats(rr["stats"], r2, f"single {i}")
    same_state(r, s, c.M, "sweep_many"); same_state(r, s2, c.M, "single sweeps")
    r.close(); s.close(); s2.close()


@pytest.mark.parametrize("lam", [0.25, 1.0])
def test_only_segment_cut(lam):
    """ONLY_SEGMENT: the three segments of the longest-first order one call each, every call applying its deltas (what one SEGMENT_APPLY
    call does): the restatement's list sweeps, segment by segment"""
    from mvtopicmodel_amd.native import SWEEP_ONLY_SEGMENT
    c, hy = _corpus()
    e, S = table(c.K, c.V[0], 7)
    r, s = pair(c, hy, None, lam, e, S)
    order = near_ties.longest_first(c.doc_off)
    for it in range(2):
        for seg in range(3):
            rr = r.sweep_list(it, 9, order[seg::3])
            rs = s.sweep(it, 9, flags=SWEEP_LIVE_SEGMENTS(3) | SWEEP_ONLY_SEGMENT(seg))
            same_stats(rr["stats"], rs, f"sweep {it} segment {seg}")
            same_state(r, s, c.M, f"sweep {it} segment {seg}")
    r.close(); s.close()


@pytest.mark.parametrize("nseg", [3, 4])
@pytest.mark.parametrize("lam", [0.25, 1.0])
def test_overlapped_segments(lam, nseg):
    """SEGMENT_APPLY | SEGMENT_OVERLAP with a mix: the lag-two schedule of tests/test_gpu_segmented.py, followed by the restatement (the
    trees, with the mix, are those of the sweep start for every segment)"""
    from mvtopicmodel_amd.native import SWEEP_SEGMENT_OVERLAP
    from tests.test_gpu_segmented import oracle_overlapped_sweep
    K, V = 300, [2000, 200, 150]
    c = small_corpus(K, V, 157, [200, 9, 12], 33)
    hy = Hyper.defaults(K, V)
    e, S = table(K, V[0], 5)
    r, s = pair(c, hy, None, lam, e, S)
    for it in range(3):
        so = oracle_overlapped_sweep(r, c, it, 5, nseg)
        st = s.sweep(it, 5, flags=SWEEP_SEGMENT_APPLY | SWEEP_SEGMENT_OVERLAP | SWEEP_LIVE_SEGMENTS(nseg))
        assert (st.tokens, st.changed, st.topic_doc_mass_cnt, st.word_ftree_mass_cnt) == \
               (so["tokens"], so["changed"], so["topic_doc_mass_cnt"], so["word_ftree_mass_cnt"])
        same_state(r, s, c.M, f"overlapped sweep {it}")
    rr = r.sweep(9, 5); rs = s.sweep(9, 5)                              # the handle is in an ordinary state afterwards
    same_stats(rr["stats"], rs, "after the overlapped sweeps"); same_state(r, s, c.M, "after the overlapped sweeps")
    r.close(); s.close()


def test_trees_equal_the_restatement():
    K, V = 200, [700, 90]
    c = small_corpus(K, V, 50, [60, 6], 21)
    hy = Hyper.defaults(K, V)
    hy.alpha[:] = np.linspace(0.01, 0.3, K + 1)[None, :]
    hy.alpha_sum[:] = hy.alpha[:, :K].sum(axis=1)
    hy.gamma[:] = [1.0, 0.7]
    e, S = table(K, V[0], 2)
    r, s = pair(c, hy, None, 0.25, e, S)
    off = make_native(c, hy, [r.get_assignments(m) for m in range(2)])
    assert s.trees_current() == 0
    r.build_trees(); s.build_trees(); off.build_trees()
    for w in range(V[0]):
        assert np.array_equal(r.get_tree(0, w), s.get_tree(0, w)), w
    assert not np.array_equal(s.get_tree(0, 5), off.get_tree(0, 5))
    for w in range(V[1]):                                               # views m > 0: the trees without a mix
        assert np.array_equal(off.get_tree(1, w), s.get_tree(1, w)), w
    r.close(); s.close(); off.close()


def test_argument_and_state_errors_leave_the_mix_in_force():
    c, hy = _corpus()
    K, V0 = c.K, c.V[0]
    e, S = table(K, V0, 7)
    r, s = pair(c, hy, None, 0.25, e, S)
    want = make_mix(0.25, e, S)
    lam, got = s.get_vectors_mix()
    assert lam == 0.25 and np.array_equal(got, want)                    # the same two operations, correctly rounded
    codes = _codes()

    def refused(code, *args):
        with pytest.raises(MvhdpError) as ei:
            s.set_vectors_mix(*args)
        assert ei.value.code == codes[code], (ei.value.code, code)
        lam2, got2 = s.get_vectors_mix()
        assert lam2 == 0.25 and np.array_equal(got2, want)

    for bad in (-0.125, 1.5, float("nan"), float("inf")):
        refused("MVHDP_ERR_INVALID_ARG", bad, e, S)
    for val in (-1.0, float("nan"), float("inf")):
        e2 = e.copy(); e2[3, 5] = val
        refused("MVHDP_ERR_INVALID_ARG", 0.5, e2, S)
    for val in (0.0, -2.0, float("nan")):
        S2 = S.copy(); S2[7] = val
        refused("MVHDP_ERR_INVALID_ARG", 0.5, e, S2)
    S2 = S.copy(); S2[7] = 1e-320                                       # every entry passes, the quotient does not
    refused("MVHDP_ERR_INVALID_ARG", 0.5, e, S2)
    refused("MVHDP_ERR_STATE", 0.5)                                     # NULL tables without a softmax
    rr = r.sweep(0, 5); rs = s.sweep(0, 5)                              # ... and the sweep still samples with the mix that was set
    same_stats(rr["stats"], rs, "after the refusals"); same_state(r, s, c.M, "after the refusals")
    r.close(); s.close()


def test_cells_below_fp32s_normal_range():
    """lambda = 1 with p_emb(w|k) of 1e-40 and less for whole words: the screening's masses would be denormal or flushed; such tokens are
    decided in fp64, as the restatement decides them"""
    c, hy = _corpus()
    e, S = table(c.K, c.V[0], 7)
    rng = np.random.RandomState(3)
    tiny = rng.rand(c.V[0]) < 0.4
    e[:, tiny] *= 1e-40
    e[:, rng.rand(c.V[0]) < 0.1] = 0.0
    for flags, tuning in ((0, None), (0, dict(force_primary=2)), (SWEEP_GENERIC_KERNEL, None)):
        r, s = pair(c, hy, None, 1.0, e, S, **(tuning or {}))
        for it in range(3):
            rr = r.sweep(it, 17); rs = s.sweep(it, 17, flags=flags)
            if rr["stats"]["aborted_docs"]:                             # (every mass zero: the reference throws, Q11; nothing to compare)
                break
            same_stats(rr["stats"], rs, f"tiny cells flags {flags:#x} sweep {it}"); same_state(r, s, c.M, f"tiny cells flags {flags:#x} sweep {it}")
        r.close(); s.close()


def test_table_from_the_device():
    """emb_init -> count_words -> train(serial) -> softmax twice (the accumulating sumExpValues) -> set_vectors_mix(lambda) with NULL tables
    = set_vectors_mix(lambda, e, S) with the arrays emb_softmax returned"""
    K, V = 20, [300, 40]
    c = small_corpus(K, V, 120, [40, 5], 13)
    hy = Hyper.defaults(K, V)
    o = make_ref(c, hy)
    z0 = [o.get_assignments(m) for m in range(2)]
    a, b = make_native(c, hy, z0), make_native(c, hy, z0)
    cfg = EmbConfig.defaults(num_columns=16, num_context_columns=4, sampling_table_size=10 ** 5, min_doc_length=2)
    a.emb_init(cfg, seed=5); a.emb_count_words(); a.emb_train(2, seed=9, serial=True)
    a.emb_softmax()
    e, S = a.emb_softmax()
    a.set_vectors_mix(0.25)
    b.set_vectors_mix(0.25, e, S)
    la, ta = a.get_vectors_mix(); lb, tb = b.get_vectors_mix()
    assert la == lb == 0.25 and np.array_equal(ta, tb) and np.array_equal(ta, make_mix(0.25, e, S))
    # a later softmax does not move what the samplers read; releasing the embeddings leaves the mix standing
    a.emb_train(1, seed=10, serial=True); a.emb_softmax()
    assert np.array_equal(a.get_vectors_mix()[1], ta)
    a.emb_release()
    assert np.array_equal(a.get_vectors_mix()[1], ta)
    o.set_vectors_mix(0.25, e, S)
    for it in range(2):
        rr = o.sweep(it, 4); ra = a.sweep(it, 4); rb = b.sweep(it, 4)
        same_stats(rr["stats"], ra, "own table"); same_stats(rr["stats"], rb, "host table")
        same_state(o, a, 2, "own table"); same_state(o, b, 2, "host table")
    o.close(); a.close(); b.close()


def test_off_is_off_and_frozen_ignores_the_mix():
    c, hy = _corpus()
    e, S = table(c.K, c.V[0], 7)
    o = make_oracle(c, hy)
    z0 = [o.get_assignments(m) for m in range(c.M)]
    s = make_native(c, hy, z0)
    s.set_vectors_mix(0.4, e, S)
    s.set_vectors_mix(0.0)
    assert s.get_vectors_mix() == (0.0, None) and s.trees_current() == 0
    for it in range(2):
        ro = o.sweep(it, 8, want_dbg=True); rs = s.sweep(it, 8, want_dbg=True)
        same_stats(ro["stats"], rs, f"off, sweep {it}"); same_state(o, s, c.M, f"off, sweep {it}")
        for m in range(c.M):
            assert np.array_equal(ro["dbg"][m][:, [0, 2]], rs.dbg[m][:, [0, 2]])
    # FROZEN + inference trees with the mix on = the same calls with it off
    t = make_native(c, hy, [s.get_assignments(m) for m in range(c.M)])
    t.set_vectors_mix(0.4, e, S)
    for x in (s, t):
        x.build_inference_trees()
    for w in (0, 9, 1499):
        assert np.array_equal(s.get_tree(0, w), t.get_tree(0, w))
    for x in (s, t):
        x.init_assignments_from_trees(12); x.build_counts(); x.build_inference_trees()
    for it in range(2):
        a = s.sweep(it, 6, flags=SWEEP_FROZEN); b = t.sweep(it, 6, flags=SWEEP_FROZEN)
        assert (a.tokens, a.changed, a.topic_doc_mass_cnt, a.word_ftree_mass_cnt) == (b.tokens, b.changed, b.topic_doc_mass_cnt, b.word_ftree_mass_cnt)
        for m in range(c.M):
            assert np.array_equal(s.get_assignments(m), t.get_assignments(m)), f"FROZEN sweep {it} view {m}"
    o.close(); s.close(); t.close()


@pytest.mark.parametrize("live16", [0, 1])
def test_live_sweeps_keep_their_invariants(live16):
    K, V = 256, [800, 60, 70]
    c = small_corpus(K, V, 300, [80, 6, 8], 19)
    hy = Hyper.defaults(K, V)
    e, S = table(K, V[0], 3)
    o = make_ref(c, hy)
    z0 = [o.get_assignments(m) for m in range(3)]
    o.close()
    runs = []
    for single_wave in (0, 1, 1):
        s = make_native(c, hy, z0)
        s.set_tuning(live16=live16, single_wave=single_wave)
        s.set_vectors_mix(0.25, e, S)
        for it in range(5):
            st = s.sweep(it, 2, flags=SWEEP_LIVE)
            assert st.tokens == c.total_tokens and st.aborted_docs == 0
            for m in range(3):
                z = s.get_assignments(m)
                nwk, nk = s.get_counts(m)
                assert nwk.min() >= 0 and nk.min() >= 0
                want = np.bincount(c.tokens[m].astype(np.int64) * K + z, minlength=V[m] * K).reshape(V[m], K)
                assert np.array_equal(nwk, want), f"live16 {live16} single_wave {single_wave} sweep {it} view {m}: n_wk is not the recount of z"
                assert np.array_equal(nk, want.sum(axis=0))
        runs.append([s.get_assignments(m) for m in range(3)])
        s.close()
    for m in range(3):                                                  # one resident wave: the sequential algorithm, so two runs agree
        assert np.array_equal(runs[1][m], runs[2][m])


def test_group_of_two_members_and_members_that_disagree():
    c, hy = _corpus()
    e, S = table(c.K, c.V[0], 7)
    r, one = pair(c, hy, None, 0.25, e, S)
    z0 = [r.get_assignments(m) for m in range(c.M)]
    cut = c.D // 2
    shards = []
    for lo, hi in ((0, cut), (cut, c.D)):
        sub = c.slice_docs(lo, hi)
        sh = make_native(sub, hy, [z0[m][c.doc_off[m][lo]:c.doc_off[m][hi]] for m in range(c.M)], doc_id_base=lo)
        shards.append(sh)
    codes = _codes()
    with NativeGroup(shards) as g:
        g.build_counts()
        shards[0].set_vectors_mix(0.25, e, S)
        with pytest.raises(MvhdpError) as ei:                           # on / off
            g.sweep(0, 5)
        assert ei.value.code == codes["MVHDP_ERR_STATE"]
        shards[1].set_vectors_mix(0.5, e, S)
        with pytest.raises(MvhdpError) as ei:                           # two lambdas
            g.sweep(0, 5)
        assert ei.value.code == codes["MVHDP_ERR_STATE"]
        g.set_vectors_mix(0.25, e, S)
        for it in range(3):
            rr = r.sweep(it, 5); one.sweep(it, 5); sts = g.sweep(it, 5)
            assert sum(st.tokens for st in sts) == c.total_tokens
            for m in range(c.M):
                zg = np.concatenate([sh.get_assignments(m) for sh in shards])
                assert np.array_equal(zg, r.get_assignments(m)), f"group sweep {it} view {m}"
                for sh in shards:
                    a, b = sh.get_counts(m), one.get_counts(m)
                    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        from mvtopicmodel_amd.native import SWEEP_ASYNC_EXCHANGE
        with pytest.raises(MvhdpError) as ei:
            g.sweep(9, 5, flags=SWEEP_LIVE | SWEEP_ASYNC_EXCHANGE)
        assert ei.value.code == codes["MVHDP_ERR_UNSUPPORTED"]
    for x in shards + [one]:
        x.close()
    r.close()


# ---- near ties (tests/mix_near_ties.py builds them with the restatement) ----
@pytest.mark.parametrize("name", sorted(mix_near_ties.PLAN))
def test_near_ties_decided_as_the_restatement_does(name):
    ev, flips, forced = mix_near_ties.flips_of(name)
    mix_near_ties.check_quotas(name, flips)
    case = ev.case
    flav = {}
    for R in forced:
        assert served_class(case, R) == R.bit_length() - 1
        s = make_native(case, case.hy, case.z0); s.set_tuning(force_primary=R)
        flav["rmax%d" % R] = (s, 0)
    for nm, fl in (("default", 0), ("generic", SWEEP_GENERIC_KERNEL), ("exact", SWEEP_EXACT_CHAIN)):
        flav[nm] = (make_native(case, case.hy, case.z0), fl)
    wide = case.K > 256
    fb = {nm: {} for nm in flav}
    dropped, kept = [0], 0
    for fi, f in enumerate(flips):
        for rung in near_ties.ladder(ev, f, mix_near_ties.JS, dropped):
            kept += 1
            after = After(ev.o, case.M)
            for nm, (s, flags) in flav.items():
                if wide and ((nm == "exact" and rung.j != -1) or (nm == "generic" and 16 < rung.j < near_ties.J_MAX)):
                    continue                                            # (as helpers.wide_rungs: neither decides by a tolerance out there)
                where = f"{case.name} {f.param} = {float(rung.x).hex()} (flip {fi} kind {f.kind}, {rung_name(rung)}) seed {f.seed} {nm}"
                s.set_hyper(case.hy)
                ev.prepare(s, f.param, rung.x)
                rs = s.sweep(ev.sweep_idx, f.seed, flags=flags)
                same_stats(rung.stats, rs, where)
                same_state(after, s, case.M, where)
                fb[nm][(fi, rung.j, rung.side)] = rs.exact_fallbacks
    for s, _ in flav.values():
        s.close()
    assert dropped[0] * 20 <= kept + dropped[0], f"{dropped[0]} rungs of {kept + dropped[0]} abandoned by the restatement"
    for nm, got in fb.items():
        if nm == "exact":
            continue
        for fi, f in enumerate(flips):
            if f.kind in "ABC":                                         # a comparison against the document-term sums (WRK:522, 529, 531)
                for side in ("lo", "hi"):
                    assert got[(fi, -1, side)] >= 1, f"{nm}: flip {fi} kind {f.kind} of {f.param} (seed {f.seed}): not handed to the sequential sum at the {side} end"


def test_full_size_leg_c4_prefix():
    """C4's corpus, K = 400, a seeded low-rank table, lambda = 0.25: one deferred sweep at the default plan; the restatement follows the
    first 2000 entities against the same global counts (as tests/test_gpu_full_size.py's prefix check)."""
    from mvtopicmodel_amd import NativeSampler, synth
    from mvtopicmodel_amd.java_init import init_assignments
    from tests.mix_ref import MixRef
    PREFIX = 2000
    cfg = synth.CONFIGS["C4"]
    K, V = cfg["K"], cfg["V"]
    M = len(V)
    c = synth.make_config("C4")
    _, K_init = synth.config_inactive("C4")
    z0 = init_assignments(K_init, c.doc_off, seed=1)
    hy = Hyper.defaults(K, V)
    e, S = table(K, V[0], 11, rank=4, scale=1.0)
    s = NativeSampler(K, V)
    for m in range(M):
        s.set_corpus(m, c.doc_off[m], c.tokens[m]); s.set_assignments(m, z0[m])
    s.set_hyper(hy); s.build_counts()
    s.set_vectors_mix(0.25, e, S)
    counts = [s.get_counts(m) for m in range(M)]
    st = s.sweep(0, 1)
    assert st.tokens == c.total_tokens and st.aborted_docs == 0
    assert st.new_mass_cnt + st.topic_doc_mass_cnt + st.word_ftree_mass_cnt == st.tokens
    print(f"C4 with the mix: sweep kernel {st.sweep_kernel_ms:.2f} ms, exact_fallbacks {st.exact_fallbacks}")
    sub = c.slice_docs(0, PREFIX)
    r = MixRef(K, V)
    for m in range(M):
        r.set_corpus(m, sub.doc_off[m], sub.tokens[m])
        r.set_assignments(m, z0[m][:int(c.doc_off[m][PREFIX])])
        r.set_counts(m, *counts[m])
    r.set_hyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, None)
    r.set_vectors_mix(0.25, e, S)
    r.sweep(0, 1, flags=2)
    for m in range(M):
        zg = s.get_assignments(m)[:int(c.doc_off[m][PREFIX])]
        zo = r.get_assignments(m)
        assert np.array_equal(zg, zo), f"view {m}: {np.count_nonzero(zg != zo)} of {len(zo)} prefix assignments differ from the restatement"
    for m in range(M):
        z = s.get_assignments(m)
        nwk, nk = s.get_counts(m)
        assert np.array_equal(nwk, np.bincount(c.tokens[m].astype(np.int64) * K + z, minlength=V[m] * K).reshape(V[m], K))
    r.close(); s.close()
