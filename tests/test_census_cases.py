"""tests/census_cases.py held to the planner's own word, without a device: every recipe's kernel is the one mvhdp_plan_probe and the
resolve rule of mvhdp_flavour.h give for its corpus, tuning and flags, with list sizes unknown and known; and every compiled sweep kernel
has a recipe, unless no request resolves to it (NEVER_RESOLVED of tests/test_flavour_resolve.py) or no plan asks for it (NEVER_PLANNED,
which a sweep of the planner over its whole domain has to bear out)."""
import ctypes as C
import itertools

import pytest

from mvtopicmodel_amd.native import SWEEP_FROZEN, SWEEP_GENERIC_KERNEL, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_SEGMENT_APPLY, SWEEP_SEGMENT_OVERLAP
from tests import census_cases as cc
from tests.test_flavour_resolve import NEVER_RESOLVED, compiled_keys, resolve, shim  # noqa: F401  (shim: the fixture that compiles the header)

GENERIC_KEYS = {(0, d, 0, 0, 0, 0, mx) for d in (0, 1) for mx in (0, 1)}


def probe(pi, t):
    from mvtopicmodel_amd import _lib
    po = _lib.PlanOutputC()
    assert _lib.load_library().mvhdp_plan_probe(C.byref(pi), C.byref(t), C.byref(po)) == 0
    return po


_z0 = {}


def initial_lists(K, R):
    """the corpus of a recipe and the topic lists of the oracle's initial assignments (what make_native is handed)"""
    if (K, R) not in _z0:
        from tests.helpers import make_oracle
        c = cc.corpus(K, R)
        o = make_oracle(c, cc.hyper(K))
        _z0[(K, R)] = (c, cc.list_lengths(c, [o.get_assignments(m) for m in range(c.M)]))
        o.close()
    return _z0[(K, R)]


@pytest.mark.parametrize("r", cc.RECIPES, ids=lambda r: r.name)
def test_the_planner_gives_a_recipe_the_kernel_it_is_written_for(r, shim):  # noqa: F811
    c, lists = initial_lists(r.K, r.R)
    long_ones = [0, 2, 3]                                       # (census_cases.corpus)
    lengths = [sum(int(c.doc_off[m][d + 1] - c.doc_off[m][d]) for m in range(c.M)) for d in range(c.D)]
    assert max(lengths) == lengths[0] and 40 * r.R <= min(lengths[d] for d in long_ones) and lengths[0] < 64 * r.R
    if r.key[0]:
        assert 32 * r.R < lists[0] <= 64 * r.R, f"the longest entity's list of {lists[0]} topics is not one for the {r.R}-round variant"
    mix = r.mode == "mix"
    t = cc.probe_tuning(r.tuning, r.env)
    for known in (False, True):
        po = probe(cc.plan_input(c, lists, known, r.flags, r.dbg, mix), t)
        assert po.status == 0, r.name
        keys = cc.keys_of_plan(po, r.K, r.mode == "live", r.dbg, mix and not r.flags & SWEEP_FROZEN, t.narrow == 2, lambda q: resolve(shim, q))
        for d in long_ones:
            launched = po.class_map[cc.class_of_list(lists[d])]
            assert keys.get(launched) == r.key, f"{r.name}, list sizes {'known' if known else 'unknown'}: entity {d} (list {lists[d]}) goes to class {launched}: {keys}"
        if r.mode == "live":
            assert po.live_rows == 1 and po.segments == 1


def test_every_compiled_kernel_has_a_recipe(shim):  # noqa: F811
    compiled = set(compiled_keys(shim)) | GENERIC_KEYS
    assert len(compiled) == 60
    have = {r.key for r in cc.RECIPES}
    assert have <= compiled
    assert not (set(cc.NEVER_PLANNED) & have) and set(cc.NEVER_PLANNED) <= compiled - NEVER_RESOLVED
    missing = compiled - NEVER_RESOLVED - set(cc.NEVER_PLANNED) - have
    assert not missing, f"compiled, resolvable, planned -- and no recipe: {sorted(missing)}"


def planned_keys(shim):  # noqa: F811
    """Every key some plan asks for: mvhdp_plan_probe over the K at which the rule or the planner switches, every force_primary, narrow,
    live16, live_rows, walk_fixed, debug and mix, thresholds searched and handed back as 0, entities up to every variant's slots, and the
    deferred, live, segmented, overlapped, frozen and generic-kernel flag sets; list sizes unknown, so that a plan launches every class
    it can reach."""
    from mvtopicmodel_amd import _lib
    from tests.helpers import PLAN_REGS
    flag_sets = [0, SWEEP_GENERIC_KERNEL, SWEEP_SEGMENT_APPLY, SWEEP_SEGMENT_APPLY | SWEEP_SEGMENT_OVERLAP, SWEEP_FROZEN,
                 SWEEP_LIVE, SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(3)]
    seen = set()
    res = {}

    def res_of(q):
        if q not in res:
            res[q] = resolve(shim, q)
        return res[q]

    for K, mdt, flags in itertools.product((85, 255, 256, 340, 341, 511, 512, 513, 1024, 1025), (60, 120, 250, 500, 1000), flag_sets):
        live = bool(flags & SWEEP_LIVE)
        pi = _lib.PlanInputC()
        pi.num_topics, pi.num_modalities, pi.num_entities, pi.max_entity_tokens = K, 2, 100, mdt
        for q in range(5):
            pi.entities_longer_than[q] = 10 if mdt > (64 << q) else 0
        pi.flags, pi.num_cus, pi.trees_current = flags, 256, 1
        for q in range(6):
            for f in range(3):
                pi.kernel_registers[q][f] = PLAN_REGS[q][f]
        lives = list(itertools.product((-1, 0, 1), (-1, 0, 1))) if live else [(-1, -1)]
        for fp, narrow, wf, plain, dbg, mix, (l16, lrows) in itertools.product((0, 1, 2, 4, 8, 16, 32), (-1, 0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), lives):
            pi.debug, pi.vectors_mix = dbg, mix
            tuning = dict(force_primary=fp, narrow=narrow, walk_fixed=wf, live16=l16, live_rows=lrows)
            if wf:
                tuning["walk_theta"] = [0.3, 0.3]
            if plain:
                tuning.update(cc.PLAIN)
            t = cc.probe_tuning(tuning, cc.NO_SLIM)                  # (narrow as the domain names it: 2 is the handle with the 12-bit image)
            po = probe(pi, t)
            if po.status != 0:
                continue
            seen.update(k for k in cc.keys_of_plan(po, K, live, dbg, mix and not flags & SWEEP_FROZEN, narrow == 2, res_of).values() if k is not None)
    return seen


def test_no_plan_asks_for_a_kernel_listed_as_never_planned(shim):  # noqa: F811
    compiled = set(compiled_keys(shim)) | GENERIC_KEYS
    seen = planned_keys(shim)
    assert seen <= compiled
    wrongly = set(cc.NEVER_PLANNED) & seen
    assert not wrongly, f"NEVER_PLANNED names kernels a plan asks for: {sorted(wrongly)}"
    # ... and the sweep is wide enough to be believed: it reaches everything the recipes reach
    assert {r.key for r in cc.RECIPES} <= seen
    assert compiled - NEVER_RESOLVED - seen == set(cc.NEVER_PLANNED)
