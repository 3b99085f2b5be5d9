"""Shared test helpers: build the same small model in the oracle and in the product."""
import ctypes as C

import numpy as np

from mvtopicmodel_amd.native import Hyper
from mvtopicmodel_amd import synth
from tests import near_ties


def small_corpus(K, V, D, lam, seed, **kw):
    return synth.generate(K, V, D, lam, seed, chunk_docs=4096, **kw)


def make_oracle(corpus, hyper, init_seed=1):
    from oracle.binding import Oracle
    o = Oracle(corpus.K, corpus.V)
    for m in range(corpus.M):
        o.set_corpus(m, corpus.doc_off[m], corpus.tokens[m])
    o.set_hyper(hyper.alpha, hyper.alpha_sum, hyper.beta, hyper.beta_sum, hyper.gamma,
                hyper.p_a, hyper.p_b, hyper.inactive)
    o.init_assignments(init_seed)
    o.build_counts()
    return o


def make_native(corpus, hyper, z_init, doc_id_base=0):
    from mvtopicmodel_amd import NativeSampler
    s = NativeSampler(corpus.K, corpus.V, device=0, doc_id_base=doc_id_base)
    for m in range(corpus.M):
        s.set_corpus(m, corpus.doc_off[m], corpus.tokens[m])
        s.set_assignments(m, z_init[m])
    s.set_hyper(hyper)
    s.build_counts()
    return s


def assert_same_state(o, s, M):
    for m in range(M):
        zo, zs = o.get_assignments(m), s.get_assignments(m)
        assert np.array_equal(zo, zs), f"z differs in view {m}: {np.count_nonzero(zo != zs)} of {len(zo)}"
        nwk_o, nk_o = o.get_counts(m)
        nwk_s, nk_s = s.get_counts(m)
        assert np.array_equal(nk_o, nk_s), f"n_k differs in view {m}"
        assert np.array_equal(nwk_o, nwk_s), f"n_wk differs in view {m}"


# VGPRs of the sweep kernels as hipcc allocates them (what tests/test_plan.py hands the planner)
PLAN_REGS = [(70, 72, 96), (72, 72, 104), (125, 128, 160), (207, 226, 256), (256, 256, 256), (96, 96, 128)]


def served_class(case, force_primary, flags=0, every=True):
    """The planner's own word (mvhdp_plan_probe) on which kernel class serves the entities of `case` under set_tuning(
    force_primary=...): the primary class if that register-resident variant serves EVERY entity (every=False: at least one), both
    in the first sweep after build_counts (list lengths unknown) and in the following ones (known), else -1.  A forced primary gets
    no more rounds than the longest entity could need, and longer lists are routed to wider classes."""
    from mvtopicmodel_amd import _lib
    L = _lib.load_library()
    tot = sum(np.diff(np.asarray(o)) for o in case.doc_off)
    lists = np.asarray(case.list_lengths())
    cls = [int(min(5, max(0, int(np.ceil(np.log2(max(n, 1) / 64.0)))))) if n <= 1024 else 5 for n in lists]
    got = set()
    for known in (False, True):
        pi = _lib.PlanInputC()
        pi.num_topics, pi.num_modalities, pi.num_entities, pi.max_entity_tokens = case.K, case.M, case.D, int(tot.max())
        for c in range(5):
            pi.entities_longer_than[c] = int((tot > (64 << c)).sum())
        if known:
            for d, c in enumerate(cls):
                pi.entities_by_class[c] += 1
                pi.tokens_by_list_rounds[min(16, (int(lists[d]) + 63) // 64 - 1)] += int(tot[d])
        pi.flags, pi.num_cus = flags, 256
        pi.inactive_topics = 0 if case.hy.inactive is None else int(np.count_nonzero(case.hy.inactive))
        for c in range(6):
            for f in range(3):
                pi.kernel_registers[c][f] = PLAN_REGS[c][f]
        t = _lib.TuningC()
        t.narrow = t.live16 = t.live_rows = t.live_overlap = -1
        for g in range(4):
            t.learnt_walk_step[g] = -1
        t.force_primary = force_primary
        po = _lib.PlanOutputC()
        assert L.mvhdp_plan_probe(C.byref(pi), C.byref(t), C.byref(po)) == 0 and po.status == 0
        pc = po.primary_class
        ok = po.register_resident == 1 and po.class_register_resident[pc] == 1 and (all if every else any)(po.class_map[c] == pc for c in set(cls))
        got.add(pc if ok else -1)
    return got.pop() if len(got) == 1 else -1


# ---- near-tie ladders on the device (tests/near_ties.py builds them with the oracle) ----
class After:
    """the oracle's state after a sweep, read once and compared with every flavour"""

    def __init__(self, o, M):
        self.z = [o.get_assignments(m) for m in range(M)]
        self.c = [o.get_counts(m) for m in range(M)]

    def get_assignments(self, m):
        return self.z[m]

    def get_counts(self, m):
        return self.c[m]


def same_statistics(rs, st, where):
    assert (rs.tokens, rs.changed, rs.new_mass_cnt, rs.topic_doc_mass_cnt, rs.word_ftree_mass_cnt, rs.aborted_docs) == \
           (st["tokens"], st["changed"], st["new_mass_cnt"], st["topic_doc_mass_cnt"], st["word_ftree_mass_cnt"], 0), where
    assert (rs.activated_topic, rs.activated_modality) == (st["activated_topic"], st["activated_modality"]), where


def rung_name(rung):
    return f"the flip's {rung.side} end" if rung.j < 0 else f"{rung.side} end {'-' if rung.side == 'lo' else '+'} 2^{rung.j} ulp"


def every_rung(flavour, rung):
    return True


def wide_rungs(flavour, rung):
    """Lists of a hundred topics and more: the exact chain walks every one of them for every token in one wavefront (15 ms to
    0.24 s a sweep) and takes no decision by a tolerance, so it runs at the flip's own ends; the generic kernel (7 to 14 ms a sweep) has
    no fp32 screen, so past the certified tolerance (2^16 ulp) only the outermost rung is left to it."""
    if flavour == "exact":
        return rung.j == -1
    if flavour == "generic":
        return rung.j <= 16 or rung.j == near_ties.J_MAX
    return True


def run_deferred_ladders(ev, flips, forced, js=near_ties.THIN_JS, runs=every_rung, others=("default", "generic", "exact")):
    """Every flip, every rung, every flavour against the oracle; returns {flavour: {(flip index, j, side): exact_fallbacks}}
    and the numbers of rungs kept and dropped.  A forced variant must be the one the planner lets serve every entity."""
    from mvtopicmodel_amd.native import SWEEP_EXACT_CHAIN, SWEEP_GENERIC_KERNEL
    case = ev.case
    flags_of = {"default": 0, "generic": SWEEP_GENERIC_KERNEL, "exact": SWEEP_EXACT_CHAIN}
    flav = {}
    for R in forced:                                         # (first: a wrong decision is then reported against the variant named)
        assert served_class(case, R) == R.bit_length() - 1, f"force_primary {R} would not be what serves the entities of {case.name}"
        s = make_native(case, case.hy, case.z0)
        s.set_tuning(force_primary=R)
        s.sweep_census(enable=True, reset=True)
        flav["rmax%d" % R] = (s, 0)
    for name in others:
        flav[name] = (make_native(case, case.hy, case.z0), flags_of[name])
    fb = {name: {} for name in flav}
    sampled = {name: 0 for name in flav}
    dropped, kept = [0], 0
    for fi, f in enumerate(flips):
        for rung in near_ties.ladder(ev, f, js, dropped):
            kept += 1
            after = After(ev.o, case.M)
            hy = ev.hyper_at(f.param, rung.x)
            for name, (s, flags) in flav.items():
                if not runs(name, rung):
                    continue
                where = f"{case.name} {f.param} = {float(rung.x).hex()} (flip {fi} kind {f.kind}, {rung_name(rung)}) seed {f.seed} {name}"
                ev.prepare(s, hy, s.set_hyper)
                rs = s.sweep(ev.sweep_idx, f.seed, flags=flags)
                same_statistics(rs, rung.stats, where)
                try:
                    assert_same_state(after, s, case.M)
                except AssertionError as e:
                    raise AssertionError(f"{where}: {e}") from None
                fb[name][(fi, rung.j, rung.side)] = rs.exact_fallbacks
                sampled[name] += rs.tokens
    # the launch census of every forced variant: it was the R-round kernel that sampled every token of every comparison above
    for R in forced:
        rows = flav["rmax%d" % R][0].sweep_census()
        by_rounds = {}
        for r in rows:
            by_rounds[r.key[0]] = by_rounds.get(r.key[0], 0) + r.tokens
        assert by_rounds.get(R, 0) == sampled["rmax%d" % R] == sum(by_rounds.values()), \
            f"force_primary {R} on {case.name}: {sampled['rmax%d' % R]} tokens sampled, by kernel rounds {by_rounds}"
    for s, _ in flav.values():
        s.close()
    assert dropped[0] * 20 <= kept + dropped[0], f"{dropped[0]} rungs of {kept + dropped[0]} abandoned by the oracle"
    return fb, kept, dropped[0]


def check_fallback_counters(flips, fb):
    """The sequential sum decided at the flip; it is not simply always on."""
    for name, got in fb.items():
        if name == "exact":                                  # (the chain is forced there: the counter says nothing)
            continue
        quiet = 0
        for fi, f in enumerate(flips):
            if f.kind in "ABC":
                for side in ("lo", "hi"):
                    assert got[(fi, -1, side)] >= 1, \
                        f"{name}: flip {fi} kind {f.kind} of {f.param} at {float(f.lo).hex()} | {float(f.hi).hex()} (seed {f.seed}): " \
                        f"a comparison a few ulps from a tie was not handed to the sequential sum at the {side} end"
            far = [got.get((fi, near_ties.J_MAX, side)) for side in ("lo", "hi")]
            quiet += all(x == 0 for x in far)
        assert 2 * quiet >= len(flips), f"{name}: exact_fallbacks is zero 2^{near_ties.J_MAX} ulp away from only {quiet} of {len(flips)} flips"
